"""Time the LPIPS(net='vgg') path (splatformer_amd/lpips.py, csrc/lpips.hip) on one GPU, on seeded weights.

layers: every (Cin, Cout, map size) class of VGG16 at `--views` images of `--size` squared, three ways that
        alternate inside one process: the 3x3 convolution kernel (lpips.conv3x3), the route the library had before
        it -- sfx_linear's gathered-rows form with a [M][9] neighbour table, -1 for an absent neighbour
        (ptv3_ops.linear(gather_idx=...)) -- and, for information only, torch's fp32 F.conv2d (the library takes
        no torch fallback).  Times are device events around `--reps` back-to-back calls, median of `--rounds`
        rounds; TF/s counts 2 * 9 * Cin * Cout useful floating-point operations per output pixel.  The two routes'
        outputs are compared at the timed size (rel-L2).
net:    LPIPS forward (metric path) and value+grad (loss path) at 4 and 9 views.
step:   a Trainer micro-step (100k Gaussians, 4 views at 800 x 800, batched render) with and without the term.

    python tools/lpips_bench.py layers|net|step [--views 4] [--size 800]
Prints one JSON line per row.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatformer_amd import lpips as L  # noqa: E402
from splatformer_amd import ptv3_ops as ops  # noqa: E402

# (Cin, Cout, map size as a divisor of the image size, convs of that class in the network)
LAYERS = [(3, 64, 1, 1), (64, 64, 1, 1), (64, 128, 2, 1), (128, 128, 2, 1), (128, 256, 4, 1), (256, 256, 4, 2),
          (256, 512, 8, 1), (512, 512, 8, 2), (512, 512, 16, 3)]


def seeded_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    convs = []
    for cin, cout in L.CONV_CH:
        convs.append((torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin)),
                      torch.randn(cout, generator=g) * 0.1))
    return convs, [torch.rand(c, generator=g) for c in L.TAP_CH]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # milliseconds per call


def neighbour_table(V, H, W, dev):
    """[V*H*W, 9] int32: the row of pixel (n, y + ky - 1, x + kx - 1), -1 outside the image."""
    y = torch.arange(H, device=dev).view(1, H, 1, 1)
    x = torch.arange(W, device=dev).view(1, 1, W, 1)
    n = torch.arange(V, device=dev).view(V, 1, 1, 1)
    k = torch.arange(9, device=dev).view(1, 1, 1, 9)
    yy, xx = y + k // 3 - 1, x + k % 3 - 1
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    return torch.where(ok, (n * H + yy) * W + xx, -1).to(torch.int32).reshape(V * H * W, 9).contiguous()


def layers(args, dev):
    V = args.views
    for cin, cout, div, count in LAYERS:
        H = W = args.size // div
        g = torch.Generator().manual_seed(cin + cout + div)
        w = (torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))).to(dev)
        b = (torch.randn(cout, generator=g) * 0.1).to(dev)
        x = torch.randn(V, H, W, cin, generator=g).clamp_min(0).to(dev)
        packed = L.pack_conv(w)
        fns = {"conv3x3": lambda: L.conv3x3(x, packed, cout, bias=b, relu=True)}
        x_nchw = x.permute(0, 3, 1, 2).contiguous()
        fns["torch_conv2d_fp32"] = lambda: torch.relu(F.conv2d(x_nchw, w, b, padding=1))
        row = dict(kind="layer", views=V, cin=cin, cout=cout, height=H, width=W, convs_in_net=count)
        if cin % 4 == 0:  # the gathered GEMM wants 16-byte rows: the 3-channel first layer has no such route
            table = neighbour_table(V, H, W, dev)
            wg = w.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()
            rows = x.view(V * H * W, cin)
            fns["gathered_linear"] = lambda: ops.linear(rows, wg, b, act=ops.ACT_RELU, gather_idx=table)
            row["rel_l2_conv_vs_gathered"] = float(
                (fns["conv3x3"]().view(-1, cout).double() - fns["gathered_linear"]().double()).norm()
                / fns["gathered_linear"]().double().norm())
        for fn in fns.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):  # alternate, so drift and neighbours hit every side alike
            for k, fn in fns.items():
                ts[k].append(timed(fn, args.reps))
        flop = 2.0 * 9 * cin * cout * V * H * W
        row["ms_median"] = {k: round(statistics.median(v), 4) for k, v in ts.items()}
        row["ms_min_max"] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ts.items()}
        row["tflops"] = {k: round(flop / statistics.median(v) / 1e9, 2) for k, v in ts.items()}
        print(json.dumps(row), flush=True)
        del fns, x, x_nchw


def net(args, dev):
    model = L.LPIPS(*seeded_weights(), device=dev)
    for V in (4, 9):
        g = torch.Generator().manual_seed(V)
        gt = torch.rand(V, args.size, args.size, 3, generator=g).to(dev)
        pred = (gt + 0.05 * torch.randn(V, args.size, args.size, 3, generator=g).to(dev)).clamp(0, 1)
        fns = {"forward": lambda: model(pred, gt), "forward_u8": lambda: model(pred, gt, quantize_u8=True),
               "value_and_grad": lambda: model.value_and_grad(pred, gt)}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items():
                ts[k].append(timed(fn, max(1, args.reps // 4)))
        mac = 305856.0 * args.size * args.size  # VGG16 up to relu5_3, per image (the pooled sizes divide evenly)
        print(json.dumps(dict(kind="net", views=V, size=args.size,
                              ms_median={k: round(statistics.median(v), 3) for k, v in ts.items()},
                              ms_min_max={k: [round(min(v), 3), round(max(v), 3)] for k, v in ts.items()},
                              forward_tflops=round(2 * mac * 2 * V / statistics.median(ts["forward"]) / 1e9, 2),
                              value_and_grad_tflops=round(2 * mac * 3 * V / statistics.median(ts["value_and_grad"])
                                                          / 1e9, 2),
                              peak_allocated_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 3))), flush=True)
        del gt, pred


def step(args, dev):
    from splatformer_amd import train as strain
    from splatformer_amd.feature_predictor import FeaturePredictor
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    model = L.LPIPS(*seeded_weights(), device=dev)
    gs = to_device(make_scene(args.n, 1, seed=1), dev)
    cams = to_device(make_cameras(args.size, args.size, n_views=4), dev)
    gt = [torch.rand(args.size, args.size, 3, generator=torch.Generator().manual_seed(v)).to(dev) for v in range(4)]
    trainers = {}
    for name, kw in (("l1", {}), ("l1_lpips", dict(lpips_loss_weight=1.0, lpips=model))):
        torch.manual_seed(0)
        fp = FeaturePredictor(sh_degree=1, zeroinit=False).to(dev)
        trainers[name] = strain.Trainer(fp, render="batched", **kw)
        trainers[name].micro_step([gs], [cams], [gt])  # warm-up (weight caches, allocator)
    ts = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.micro_step([gs], [cams], [gt])  # (reads the loss: drains the stream)
            ts[k].append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(kind="micro_step", n=args.n, views=4, size=args.size, render="batched",
                          ms_median={k: round(statistics.median(v), 2) for k, v in ts.items()},
                          ms_min_max={k: [round(min(v), 2), round(max(v), 2)] for k, v in ts.items()})), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["layers", "net", "step"])
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpips_bench needs a GPU")
    dev = torch.device("cuda:0")
    {"layers": layers, "net": net, "step": step}[args.what](args, dev)


if __name__ == "__main__":
    main()
