"""Time the two image-quality kernels on one GPU: metrics.eval_stats_u8 (sfx_eval_metrics_u8) on an RGBA and on an
RGB target, and losses.image_loss_and_grad (sfx_image_loss, forward + derivative) on the RGB target.

Times are device events around `--reps` back-to-back calls, median of `--rounds` rounds with the sides alternating
inside the process.  To compare two builds of the library, run this once per build (SFX_LIB, --label) in one
session, alternating the builds.  Bytes are the least each side has to move, computed from the shapes (whole pixels
of an RGBA target count 16 bytes: the lines are fetched whole; the loss reads pred and gt twice and writes and reads
three fp32 maps and d_pred).

    python tools/eval_metrics_bench.py --views 9 --size 800
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatformer_amd import losses, metrics  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--label", default="in-tree", help="name of the library build in the record")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_bench needs a GPU")
    dev = torch.device("cuda:0")
    V, H, W = args.views, args.size, args.size
    g = torch.Generator().manual_seed(0)
    gt = torch.rand(V, H, W, 3, generator=g)
    pred = (gt + 0.05 * torch.randn(V, H, W, 3, generator=g)).clamp(0, 1)
    y = torch.linspace(-1, 1, H).view(1, H, 1)
    x = torch.linspace(-1, 1, W).view(1, 1, W)
    m = (torch.round(((1.0 - torch.sqrt(x * x / 0.5 + y * y / 0.4)) / 0.2 + 0.5).clamp(0, 1) * 255) / 255.0).expand(V, H, W)
    rgba = torch.cat([gt * m[..., None], m[..., None]], -1).contiguous().to(dev)
    rgb = gt.to(dev)
    pred = pred.to(dev)

    fns = {
        "masked_fused": lambda: metrics.eval_stats_u8(pred, rgba, clamp_pred=False),
        "rgb_fused": lambda: metrics.eval_stats_u8(pred, rgb, clamp_pred=False),
        "image_loss_grad": lambda: losses.image_loss_and_grad(pred, rgb, 0.8, 0.2),
    }
    for fn in fns.values():  # warm every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.rounds):  # alternate, so drift and neighbours hit every side alike
        for k, fn in fns.items():
            times[k].append(timed(fn, args.reps))
    px = V * H * W
    out = {
        "library": args.label,
        "views": V, "height": H, "width": W, "reps": args.reps, "rounds": args.rounds,
        "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
        "us_rounds": {k: [round(t, 2) for t in v] for k, v in times.items()},
        "min_bytes": {"masked_fused": 28 * px, "rgb_fused": 24 * px, "image_loss_grad": (24 + 36 + 36 + 24 + 12) * px},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
