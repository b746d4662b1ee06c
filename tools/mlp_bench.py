"""Fused Block MLP (sfx_block_mlp) vs the unfused LayerNorm + fc1(GELU) + fc2(+residual) launches on the config-B
stage shapes: per-launch time (HIP events, median of 20) and fp32-equivalent TF/s.
usage: python tools/mlp_bench.py [--fused-only] [--reps N] [M,C ...]
  M,C ...       shapes instead of config B's; M may be written sK or hK (K rounds of whole 128-point / hidden-split
                64-point tiles: K x slots x 128 or 64 points, slots = CUs at C = 256, 2 x CUs below) to time whole
                rounds alone
  --fused-only  skip the unfused launches (and the difference against them)
Each line also shows the launch plan the call ran (sfx_block_mlp_last_plan) and the
bytes its workgroups streamed from L2 into LDS (workgroups x sfx_mlp_stream_floats(C) / split x 4)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatformer_amd import _lib  # noqa: E402
from splatformer_amd import ptv3_ops as ops  # noqa: E402

SHAPES = [(100000, 64), (100000, 96), (90434, 96), (70349, 128), (37759, 256)]


def timeit(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def last_plan(C):
    """(text, L2 -> LDS bytes) of the calling thread's last sfx_block_mlp."""
    p = ops.block_mlp_last_plan()
    kind, split, main, tail, pts = p["kind"], p["split"], p["main_wgs"], p["tail_wgs"], p["pts"]
    if kind < 0:
        return "", None
    stream = 8 * C * C * 4
    byts = main * stream + tail * stream  # tail: tail x split workgroups, each 1 / split of the stream
    return (f" | plan {'hs' if kind else 'whole'} pts {pts} main {main} tail {tail} x{split}, L2->LDS {byts / 1e9:.3f} GB",
            byts)


def main():
    argv = sys.argv[1:]
    fused_only = "--fused-only" in argv
    reps = int(argv[argv.index("--reps") + 1]) if "--reps" in argv else 20
    _lib.load()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = []
    for a in argv:
        if "," in a:
            m, c = a.split(",")
            c = int(c)
            slots = cus if c > 128 else 2 * cus
            shapes.append((int(m[1:]) * slots * (128 if m[0] == "s" else 64) if m[0] in "sh" else int(m), c))
    torch.manual_seed(0)
    for M, C in shapes or SHAPES:
        ln = torch.nn.LayerNorm(C).to(dev)
        fc1, fc2 = torch.nn.Linear(C, 4 * C).to(dev), torch.nn.Linear(4 * C, C).to(dev)
        x = torch.randn(M, C, device=dev)
        fl = 2.0 * M * 4 * C * C * 2
        tf, lo, hi = timeit(lambda: ops.block_mlp(x, ln, fc1, fc2), reps)
        plan, _ = last_plan(C)
        head = (f"M={M:6d} C={C:3d}: fused {tf:8.1f} us [{lo:.1f}, {hi:.1f}] ({fl / tf / 1e6:6.1f} TF/s, "
                f"{2 * M * C * 4 / tf / 1e3:6.0f} GB/s X+Y)")
        if fused_only:
            print(head + plan, flush=True)
            continue

        def unfused():
            h = ops.layernorm(x, ln.weight, ln.bias, ln.eps)
            m = ops.linear(h, fc1.weight, fc1.bias, act=ops.ACT_GELU)
            return ops.linear(m, fc2.weight, fc2.bias, residual=x)
        tu = timeit(unfused, reps)[0]
        y, y0 = ops.block_mlp(x, ln, fc1, fc2), unfused()
        err = float((y - y0).norm() / (y0 - x).norm())
        print(head + f" | unfused {tu:8.1f} us ({fl / tu / 1e6:6.1f} TF/s) | speedup {tu / tf:5.2f} | "
              f"rel diff {err:.1e}" + plan, flush=True)


if __name__ == "__main__":
    main()
