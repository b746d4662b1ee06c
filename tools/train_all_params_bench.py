"""Measurements of the all-parameter training backward (DESIGN.md "Training every parameter").

conv:  sfx_subm_conv_wgrad at the five encoder-stage shapes of a 100k-Gaussian scene (the maps, conv inputs and
       output gradients' shapes of a real training forward) against the composition that was possible before it:
       27 index_select gathers of both operands + 27 sfx_linear_wgrad calls.  Same process, same buffers, warm-up,
       medians over the repeats (HIP events around each call), clocks untouched.
step:  one config-C-shaped micro-step (100k Gaussians, 4 views at 800x800) with finetune_list=None against the
       default ('attn.qkv',), in fp32 and amp: median wall time and peak allocated memory.

    python tools/train_all_params_bench.py conv|step [--n 100000] [--reps 20]
Prints one JSON line per row.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatformer_amd import train as strain  # noqa: E402
from splatformer_amd import train_ops as tops  # noqa: E402
from splatformer_amd.feature_predictor import FeaturePredictor  # noqa: E402
from splatformer_amd.scenes import make_cameras, make_scene, to_device  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def conv(args, dev):
    torch.manual_seed(0)
    model = FeaturePredictor(sh_degree=1, zeroinit=False).to(dev)
    strain.select_trainable(model, ("cpe.0",))  # keeps every block's conv input on the tape
    gs = to_device(make_scene(args.n, 1, seed=1), dev)
    _, tape = strain.refine_train(model, gs, strain.pt.device_drop_masks(torch.Generator(device=dev).manual_seed(0)))
    for s, recs in enumerate(tape["bb"]["enc"]):
        rec = next(r for r in recs if r["kind"] == "block")
        x, smap = rec["cpe_in"], rec["smap"]
        n, C = x.shape
        dy = torch.randn(n, C, device=dev)
        off = smap.pair_off
        dw = torch.zeros(C, 27 * C, device=dev)
        db = torch.zeros(C, device=dev)
        ar = torch.arange(n, device=dev, dtype=torch.int32)
        centre_in = smap.nbr[:, 13].contiguous()

        def fused():
            tops.subm_conv_wgrad(dy, x, smap, dw, db)

        def composed():
            for k in range(27):
                if k == 13:
                    i_in, i_out = centre_in, ar
                else:
                    i_in, i_out = smap.pair_in[off[k]:off[k + 1]], smap.pair_out[off[k]:off[k + 1]]
                if i_in.numel() == 0:
                    continue
                tops.linear_wgrad(dy.index_select(0, i_out), x.index_select(0, i_in), dw[:, k * C:(k + 1) * C],
                                  db if k == 13 else None)

        dw.zero_()
        fused()
        a = dw.clone()
        dw.zero_()
        composed()
        agree = float((a - dw).norm() / dw.norm())
        tf, tc = timed(fused, args.reps), timed(composed, args.reps)
        print(json.dumps(dict(kind="conv_wgrad", stage=s, n=n, C=C, pairs=off[27], fused_ms=round(tf[0], 4),
                              fused_min_max=[round(tf[1], 4), round(tf[2], 4)], composed_ms=round(tc[0], 4),
                              composed_min_max=[round(tc[1], 4), round(tc[2], 4)],
                              speedup=round(tc[0] / tf[0], 2), rel_diff=agree)), flush=True)


def step(args, dev):
    gs = to_device(make_scene(args.n, 1, seed=1), dev)
    cams = to_device(make_cameras(800, 800, n_views=4), dev)
    gt = [torch.rand(800, 800, 3, device=dev) for _ in range(4)]
    for prec in ("fp32", "amp"):
        for name, fl in (("attn.qkv", ("attn.qkv",)), ("all", None)):
            torch.manual_seed(0)
            model = FeaturePredictor(sh_degree=1, zeroinit=False).to(dev)
            tr = strain.Trainer(model, finetune_list=fl, precision=prec,
                                generator=torch.Generator(device=dev).manual_seed(0))
            tr.micro_step([gs], [cams], [gt])  # warm-up (weight caches, allocator)
            tr.flat_grad.zero_()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            ts = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                tr.micro_step([gs], [cams], [gt])  # (reads the loss: drains the stream)
                ts.append((time.perf_counter() - t0) * 1e3)
                tr.flat_grad.zero_()
            print(json.dumps(dict(kind="micro_step", n=args.n, views=4, res=800, precision=prec, finetune=name,
                                  trainable=sum(p.numel() for p in tr.params), ms=round(statistics.median(ts), 2),
                                  min_max=[round(min(ts), 2), round(max(ts), 2)],
                                  peak_mem_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))), flush=True)
            del tr, model
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("conv", "step"))
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    d = torch.device("cuda:0")
    (conv if a.what == "conv" else step)(a, d)
