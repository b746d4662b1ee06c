"""Time metrics.eval_metrics_u8 (one fused kernel) against the calls it replaces, on one GPU.

Masked case (RGBA target): the composed sequence is what evaluation had to run for the same result before the fused
kernel: slice copy of gt[..., :3], pred * mask, image_stats_u8, ssim(quantize_u8=True).  Unmasked case (RGB target):
image_stats_u8 + ssim(quantize_u8=True) alone.  The two sides alternate inside one process; times are device
events around `--reps` back-to-back calls, median of `--rounds` rounds.  Bytes are the least each side has to
move, computed from the shapes (whole pixels of an RGBA target count 16 bytes: the lines are fetched whole).

    python tools/eval_metrics_bench.py --views 9 --size 800
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from splatformer_amd import metrics  # noqa: E402


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

    def composed_masked():
        gt3 = rgba[..., :3].contiguous()
        pm = pred * rgba[..., 3:]
        return metrics.image_stats_u8(pm, gt3, clamp_pred=False), metrics.ssim(pm, gt3, quantize_u8=True)

    parts = {
        "slice_copy": lambda: rgba[..., :3].contiguous(),
        "pred_times_mask": lambda: pred * rgba[..., 3:],
        "image_stats_u8": lambda: metrics.image_stats_u8(pred, rgb, clamp_pred=False),
        "ssim_quantized": lambda: metrics.ssim(pred, rgb, quantize_u8=True),
    }
    sides = {
        "masked_fused": lambda: metrics.eval_stats_u8(pred, rgba, clamp_pred=False),
        "masked_composed": composed_masked,
        "rgb_fused": lambda: metrics.eval_stats_u8(pred, rgb, clamp_pred=False),
        "rgb_composed": lambda: (parts["image_stats_u8"](), parts["ssim_quantized"]()),
    }
    # the two sides compute the same thing at this size
    f = metrics.eval_metrics_u8(pred, rgba, clamp_pred=False)
    (s, mx), ss = composed_masked()
    assert torch.equal(f["sums"], s) and torch.equal(f["maxes"], mx)
    ssim_diff = float((f["ssim"] - ss).abs().max())

    fns = {**sides, **parts}
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
        "views": V, "height": H, "width": W, "reps": args.reps, "rounds": args.rounds,
        "us_median": {k: round(statistics.median(v), 2) for k, v in times.items()},
        "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
        "ssim_max_abs_diff_fused_vs_composed": ssim_diff,
        # least bytes: fused reads pred (12 B/px) and the target once; composed: slice (16 in, 12 out), multiply
        # (12 + 16 in, 12 out), stats (24 in), ssim (24 in)
        "min_bytes": {"masked_fused": 28 * px, "masked_composed": (28 + 40 + 24 + 24) * px,
                      "rgb_fused": 24 * px, "rgb_composed": 48 * px},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
