"""Seeded fp32 inputs of the render-gradient edge tests, shared by tests/test_oracle_render_grad.py (which shows on
the CPU that the restatements equal fp64 autograd and that wrong formulas miss the bars on exactly these inputs)
and tests/test_gpu_render_edges.py.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Rasterizer cases are built in screen space (xys, conics, opacities, radii, depths): no projection involved.  The
backward is discontinuous, once final_idx is given, only where alpha crosses 1/255 or sigma crosses 0; every
case's seed is advanced until no (pixel, Gaussian) pair lies within NEAR of either threshold in fp64
(near_threshold_pairs), so fp32 and fp64 take the same branch everywhere and nothing has to be excluded from a
comparison.
"""
from __future__ import annotations

import functools
import math
from typing import Dict

import numpy as np
import torch

from . import gsplat_ref

f32, f64 = torch.float32, torch.float64
NEAR = 1e-4
BG = (0.3, 0.2, 0.1)

RASTER_CASES = ["partial_40x24", "px_1x1", "px_16x16", "px_17x17", "batch_8", "batch_9", "batch_17", "batch_255",
                "batch_256", "batch_257", "batch_512", "batch_513", "saturated", "stack_early", "empty_positions",
                "indefinite", "cross_tile"]


def gen(*key: int) -> torch.Generator:
    seed = 0
    for k in key:
        seed = seed * 100003 + int(k)
    return torch.Generator().manual_seed(seed)


def _u(g, n, lo, hi):
    return lo + (hi - lo) * torch.rand(n, generator=g)


def _conics_from_sigmas(s1, s2, theta):
    """Conic (inverse covariance, packed a, b, c) of a Gaussian with principal std-devs s1, s2 (pixels) at angle
    theta, and gsplat's radius ceil(3 sqrt(lambda_max))."""
    c, s = torch.cos(theta), torch.sin(theta)
    i1, i2 = 1.0 / (s1 * s1), 1.0 / (s2 * s2)
    a = c * c * i1 + s * s * i2
    b = c * s * (i1 - i2)
    cc = s * s * i1 + c * c * i2
    radius = torch.ceil(3.0 * torch.maximum(s1, s2))
    return torch.stack([a, b, cc], -1).to(f32), radius.to(torch.int32)


def _blobs(g, n, W, H, smin, smax, omin, omax, margin=4.0):
    xys = torch.stack([_u(g, n, -margin, W + margin), _u(g, n, -margin, H + margin)], -1)
    conics, radii = _conics_from_sigmas(_u(g, n, smin, smax), _u(g, n, smin, smax), _u(g, n, 0.0, math.pi))
    return xys, conics, radii, _u(g, n, omin, omax)


def _faint_wide(g, n, W, H):
    """Gaussians far wider than the image and faint enough that hundreds of them leave T above the 1e-4 stop:
    every one contributes at every pixel (alpha in about [0.005, 0.014], clear of 1/255).  Centres 4 to 8 pixels
    outside the image, so sigma stays clear of 0 at every pixel centre."""
    side = torch.rand(n, generator=g) < 0.5
    off = torch.where(side, -_u(g, n, 4.0, 8.0), W + _u(g, n, 4.0, 8.0))
    xys = torch.stack([off, _u(g, n, 0.0, H)], -1)
    conics, radii = _conics_from_sigmas(_u(g, n, 40.0, 80.0), _u(g, n, 40.0, 80.0), _u(g, n, 0.0, math.pi))
    return xys, conics, radii, _u(g, n, 0.008, 0.014)


def _cat(parts):
    return [torch.cat([p[i] for p in parts], 0) for i in range(4)]


def _build_raster(name: str, seed: int) -> Dict:
    g = gen(31, RASTER_CASES.index(name), seed)
    depths = None
    if name == "partial_40x24":
        # partial tiles right and bottom at block width 16; the right column's right quadrants and the bottom
        # row's bottom quadrants lie wholly outside the image.  Opacities <= 0.95: the alpha clamp never binds.
        W, H = 40, 24
        xys, conics, radii, op = _blobs(g, 300, W, H, 1.0, 5.0, 0.05, 0.95)
    elif name.startswith("px_"):
        W = H = int(name.split("x")[-1])
        xys, conics, radii, op = _blobs(g, 40, W, H, 1.0, 5.0, 0.05, 0.95, margin=2.0)
    elif name.startswith("batch_"):
        # one 16x16 tile whose list has exactly K records, all contributing at all pixels: the 256-record batches
        # of the three kernels at 255 / 256 / 257 / 512 / 513, the quad kernel's ring of 8 at 8 / 9 / 17
        W = H = 16
        xys, conics, radii, op = _faint_wide(g, int(name.split("_")[1]), W, H)
    elif name == "saturated":
        W = H = 32
        xys, conics, radii, op = _blobs(g, 48, W, H, 8.0, 30.0, 0.0, 0.0, margin=0.0)
        xys = torch.round(xys)  # on pixel corners: sigma >= 0.25 / 30^2 > NEAR at every pixel centre
        op = torch.where(torch.arange(48) % 2 == 0, torch.tensor(0.999), torch.tensor(1.0))
    elif name == "stack_early":
        # front to back: 12 opaque Gaussians stacked on quadrant 0 of tile 0 (every pixel there stops within the
        # first records), 40 small opaque blobs (final_idx differs from lane to lane), then 560 faint wide ones:
        # 612 records = 3 batches per tile, and the waves that stopped in front skip the rear batches
        W, H = 32, 16
        n1, n2, n3 = 12, 40, 560
        x1 = torch.stack([_u(g, n1, 3.0, 5.0), _u(g, n1, 3.0, 5.0)], -1)
        c1, r1 = _conics_from_sigmas(_u(g, n1, 9.0, 11.0), _u(g, n1, 9.0, 11.0), _u(g, n1, 0.0, math.pi))
        p1 = (x1, c1, torch.full_like(r1, 100), _u(g, n1, 0.85, 0.95))
        p2 = _blobs(g, n2, W, H, 1.0, 2.5, 0.8, 0.95, margin=0.0)
        p2 = (p2[0], p2[1], torch.full_like(p2[2], 100), p2[3])
        p3 = _faint_wide(g, n3, W, H)
        xys, conics, radii, op = _cat([p1, p2, p3])
        depths = torch.cat([_u(g, n1, 1.0, 2.0), _u(g, n2, 2.0, 3.0), _u(g, n3, 3.0, 9.0)])
    elif name == "empty_positions":
        # 3x2 tiles at block width 16: small Gaussians in tile 0's lower right corner only (most of its pixels
        # have no contributor, final_idx == 0 == the position of the list's first record), tiles 1 and 2 empty,
        # the second row's lists start at non-zero offsets
        W, H = 48, 32
        pa = _blobs(g, 6, 4, 4, 0.8, 1.5, 0.3, 0.9, margin=0.0)
        pa = (pa[0] + torch.tensor([11.0, 11.0]), pa[1], torch.clamp(pa[2], max=4), pa[3])
        pb = _blobs(g, 30, 48, 10, 1.0, 2.5, 0.3, 0.9, margin=0.0)
        pb = (pb[0] + torch.tensor([0.0, 21.0]), pb[1], torch.clamp(pb[2], max=4), pb[3])
        xys, conics, radii, op = _cat([pa, pb])
    elif name == "indefinite":
        # b^2 > ac on half the Gaussians: sigma < 0 on two sectors of the plane, >= 0 on the others
        W = H = 32
        n = 24
        xys, conics, radii, op = _blobs(g, 2 * n, W, H, 2.0, 6.0, 0.3, 0.9, margin=0.0)
        a, c = _u(g, n, 0.01, 0.05), _u(g, n, 0.01, 0.05)
        b = _u(g, n, 1.5, 3.0) * torch.sqrt(a * c) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
        conics[:n] = torch.stack([a, b, c], -1)
        radii[:n] = 64
    elif name == "cross_tile":
        # one Gaussian over every tile of a 4x3 (8x6 at block width 8) grid, in front of 60 small ones
        W, H = 64, 48
        # (centred on a pixel corner: sigma >= 0.25 / 40^2 > NEAR at every pixel centre)
        pa = (torch.tensor([[30.0, 23.0]]), *_conics_from_sigmas(torch.tensor([40.0]), torch.tensor([30.0]),
                                                                 torch.tensor([0.4])), torch.tensor([0.5]))
        pb = _blobs(g, 60, W, H, 1.0, 4.0, 0.1, 0.95)
        xys, conics, radii, op = _cat([pa, pb])
        depths = torch.cat([torch.tensor([0.5]), _u(g, 60, 1.0, 5.0)])
    else:
        raise KeyError(name)
    n = xys.shape[0]
    if depths is None:
        depths = _u(g, n, 1.0, 5.0)
    # Upstream gradients: standard normal, except where hundreds of image-wide Gaussians weigh all pixels of a
    # tile almost equally -- there a zero-mean v_out cancels in the pixel sum to 1/16 of its terms and the fp32
    # error relative to the result measures that cancellation (5e-6 at 512 records), not the formula; a mean of
    # 1 (0.5 for v_out_alpha) keeps the sums at the size of their terms.
    mu, sd = (1.0, 0.5) if name.startswith("batch_") or name == "stack_early" else (0.0, 1.0)
    vo = lambda *s: mu + sd * torch.randn(*s, generator=g)
    return dict(name=name, seed=seed, W=W, H=H, n=n, xys=xys.to(f32).contiguous(), conics=conics.contiguous(),
                radii=radii.contiguous(), opacities=op.to(f32).reshape(n, 1).contiguous(),
                depths=depths.to(f32).contiguous(), colors=torch.rand(n, 3, generator=g),
                background=torch.tensor(BG), v_out=vo(H, W, 3), v_out_alpha=0.5 * vo(H, W), v_out2=vo(H, W, 3),
                v_out_alpha2=0.5 * vo(H, W))


def pair_terms(case: Dict, dtype=f64):
    """sigma and unclamped alpha = o exp(-sigma) of every (pixel, Gaussian) pair of the image, [H*W, n]."""
    W, H = case["W"], case["H"]
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    pxf, pyf = px.reshape(-1).to(dtype) + 0.5, py.reshape(-1).to(dtype) + 0.5
    xy, con = case["xys"].to(dtype), case["conics"].to(dtype)
    dx, dy = xy[:, 0][None] - pxf[:, None], xy[:, 1][None] - pyf[:, None]
    sigma = 0.5 * (con[:, 0][None] * dx * dx + con[:, 2][None] * dy * dy) + con[:, 1][None] * dx * dy
    alpha = case["opacities"].reshape(-1).to(dtype)[None] * torch.exp(-sigma.clamp(min=-700.0))
    return sigma, alpha


def near_threshold_pairs(case: Dict) -> int:
    """(pixel, Gaussian) pairs within NEAR of a discontinuity of the backward: |255 alpha - 1| or |sigma|."""
    sigma, alpha = pair_terms(case)
    return int(((255.0 * alpha - 1.0).abs() < NEAR).sum() + (sigma.abs() < NEAR).sum())


@functools.lru_cache(maxsize=None)
def raster_case(name: str) -> Dict:
    """The case at its first seed with no pair near a threshold (deterministic; tests assert the count is 0)."""
    for seed in range(64):
        case = _build_raster(name, seed)
        if near_threshold_pairs(case) == 0:
            return case
    raise RuntimeError(f"{name}: no seed below 64 is clear of the thresholds")


@functools.lru_cache(maxsize=None)
def raster_state(name: str, bw: int) -> Dict:
    """The oracle's fp32 binning and forward state of a case at block width bw: what every backward
    implementation, HIP or restatement, is handed."""
    c = raster_case(name)
    W, H = c["W"], c["H"]
    tx, ty = (W + bw - 1) // bw, (H + bw - 1) // bw
    x0, y0, x1, y1 = gsplat_ref.tile_bbox(c["xys"], c["radii"], tx, ty, bw)
    tiles = torch.where(c["radii"] > 0, (x1 - x0) * (y1 - y0), torch.zeros_like(x0)).to(torch.int32)
    _, gids, bins = gsplat_ref.bin_and_sort_gaussians(c["xys"], c["depths"], c["radii"], tiles, tx, ty, bw)
    img, fT, fidx = gsplat_ref.rasterize_forward(tx, ty, bw, H, W, gids, bins, c["xys"], c["conics"], c["colors"],
                                                 c["opacities"], c["background"])
    return dict(tx=tx, ty=ty, bw=bw, tiles=tiles, gids=gids.contiguous(), bins=bins.contiguous(), img=img,
                final_Ts=fT.contiguous(), final_idx=fidx.contiguous())


def raster_backward_ref(name: str, bw: int, dtype, v_out=None, v_out_alpha=None, **kw):
    """(v_xy, v_conic, v_rgb, v_opacity, v_xy_abs) of the restatement in `dtype` on the fp32 state."""
    c, s = raster_case(name), raster_state(name, bw)
    v_out = c["v_out"] if v_out is None else v_out
    v_out_alpha = c["v_out_alpha"] if v_out_alpha is None else v_out_alpha
    return gsplat_ref.rasterize_backward(s["tx"], s["ty"], bw, c["H"], c["W"], s["gids"], s["bins"], c["xys"],
                                         c["conics"], c["colors"], c["opacities"], c["background"], s["final_Ts"],
                                         s["final_idx"], v_out, v_out_alpha, dtype=dtype, return_abs=True, **kw)


def raster_coverage(name: str, bw: int = 16) -> Dict[str, int]:
    """What the case reaches, from the fp64 pair terms and the oracle's state (for the coverage assertions)."""
    c, s = raster_case(name), raster_state(name, bw)
    W, H = c["W"], c["H"]
    sigma, alpha = pair_terms(c)
    fidx, bins, gids = s["final_idx"].long(), s["bins"].long(), s["gids"].long()
    out = dict(near=near_threshold_pairs(c), contrib_above_099=0, contrib_above_0999=0, sigma_neg=0, sigma_pos=0,
               max_list=int((bins[:, 1] - bins[:, 0]).max()), empty_tiles=int((bins[:, 1] == bins[:, 0]).sum()),
               tiles=int(bins.shape[0]), lane_varied_waves=0, quadrant_varied_tiles=0, waves_skipping_a_batch=0,
               pixels_no_contributor_tile0=0, tiles_offset_start=int(((bins[:, 0] > 0)).sum()),
               gaussians_in_all_tiles=0, early_pixels=0)
    hit = torch.zeros(c["n"], dtype=torch.long)
    for t in range(bins.shape[0]):
        r0, r1 = int(bins[t, 0]), int(bins[t, 1])
        hit[gids[r0:r1].unique()] += 1
        tyi, txi = divmod(t, s["tx"])
        ys = torch.arange(tyi * bw, min((tyi + 1) * bw, H))
        xs = torch.arange(txi * bw, min((txi + 1) * bw, W))
        if r1 <= r0 or not len(ys) or not len(xs):
            continue
        pix = (ys[:, None] * W + xs[None, :])
        f = fidx.reshape(-1)[pix]  # [h, w]
        g = gids[r0:r1]
        pos = torch.arange(r0, r1)
        pp = pix.reshape(-1)
        sg, al = sigma[pp][:, g], alpha[pp][:, g]
        valid = (pos[None] <= f.reshape(-1)[:, None]) & (sg >= 0) & (al >= 1.0 / 255.0)
        out["contrib_above_099"] += int((valid & (al > 0.99)).sum())
        out["contrib_above_0999"] += int((valid & (al > 0.999)).sum())
        seen = pos[None] <= f.reshape(-1)[:, None]
        out["sigma_neg"] += int((seen & (sg < 0)).sum())
        out["sigma_pos"] += int((seen & (sg >= 0)).sum())
        out["early_pixels"] += int((f < r1 - 1).sum())
        if t == 0:
            out["pixels_no_contributor_tile0"] = int((~valid.any(1)).sum())
        if bw == 16:  # the quad kernels' waves are the 8x8 quadrants
            qmax = []
            for qy in (0, 8):
                for qx in (0, 8):
                    fq = f[qy:qy + 8, qx:qx + 8]
                    if fq.numel() == 0:
                        continue
                    qmax.append(int(fq.max()))
                    out["lane_varied_waves"] += int(fq.min() != fq.max())
                    out["waves_skipping_a_batch"] += int(int(fq.max()) < r1 - 1 - 256)
            out["quadrant_varied_tiles"] += int(len(set(qmax)) > 1)
    out["gaussians_in_all_tiles"] = int((hit == bins.shape[0]).sum())
    return out


# ---------------------------------------------------------------------------------------------------------------
# Projection cases: n Gaussians whose row i carries feature i % len(PROJ_FEATURES); errors are measured per
# feature group, so the huge gradients of a near-plane row cannot hide a wrong term on an ordinary one.
PROJ_FEATURES = ["ordinary", "beyond_clamp", "near_plane", "behind", "tiny_scale", "needle", "qnorm_1e-3",
                 "qnorm_1e3", "negative_pixels", "covers_all_tiles", "area_culled", "bad_quat"]
# (n, W, H, block width, glob_scale, clip_thresh): n = 1 is run once per feature (proj_case(cfg, feature))
PROJ_CONFIGS = {
    "n255_17x33_bw8": (255, 17, 33, 8, 0.5, 0.2),
    "n256_160x120_bw16": (256, 160, 120, 16, 1.7, 0.01),
    "n257_1x1_bw16": (257, 1, 1, 16, 1.0, 0.01),
    "n2000_160x120_bw16": (2000, 160, 120, 16, 1.7, 0.2),
    "n1_17x33_bw8": (1, 17, 33, 8, 0.5, 0.2),
}


def _next(x: float, up: bool) -> float:
    return float(np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf)))


@functools.lru_cache(maxsize=None)
def proj_case(config: str, only_feature: str = None) -> Dict:
    """Means are laid out in camera space and mapped to the world by the camera's inverse.  The camera is an axis
    permutation (x_cam = y_w, y_cam = z_w, z_cam = x_w, no translation): not symmetric, so a transposed W shows,
    and exact in fp32, so tz lands on, one ulp above and one ulp below clip_thresh as designed."""
    n, W, H, bw, glob, clip = PROJ_CONFIGS[config]
    g = gen(47, list(PROJ_CONFIGS).index(config), PROJ_FEATURES.index(only_feature) if only_feature else 99)
    clip32 = float(np.float32(clip))
    side = max(W, H)
    fx, fy, cx, cy = 1.1 * side, 0.8 * side, 0.45 * W, 0.56 * H
    lim_x, lim_y = gsplat_ref.fov_limits(fx, fy, W, H)
    feat = torch.arange(n) % len(PROJ_FEATURES)
    if only_feature is not None:
        feat = torch.full((n,), PROJ_FEATURES.index(only_feature))
    F = lambda nm: feat == PROJ_FEATURES.index(nm)
    r = lambda lo, hi: _u(g, n, lo, hi)
    tz = r(2.0, 4.0)
    ax, ay = r(-0.9, 0.9) * (0.5 * W / fx), r(-0.9, 0.9) * (0.5 * H / fy)  # tx / tz, ty / tz inside the image
    scales = torch.stack([r(0.02, 0.1), r(0.02, 0.1), r(0.02, 0.1)], -1) / glob
    quats = torch.randn(n, 4, generator=g)
    quats = quats / quats.norm(dim=-1, keepdim=True)
    # a live Gaussian whose centre is beyond 1.3 tan(fov) on x, y or both, large enough to reach the image
    m = F("beyond_clamp")
    k = torch.arange(n) // len(PROJ_FEATURES) % 3
    ax = torch.where(m & (k != 1), lim_x * r(1.2, 1.8) * torch.where(r(0, 1) < 0.5, -1.0, 1.0), ax)
    ay = torch.where(m & (k != 0), lim_y * r(1.2, 1.8) * torch.where(r(0, 1) < 0.5, -1.0, 1.0), ay)
    scales = torch.where(m[:, None], torch.stack([r(1.0, 2.0), r(1.0, 2.0), r(1.0, 2.0)], -1) / glob, scales)
    # tz one ulp above, at, one ulp below clip_thresh, then a few just above it; small enough to stay on screen
    m = F("near_plane")
    k = torch.arange(n) // len(PROJ_FEATURES) % 5
    near = torch.tensor([_next(clip32, True), clip32, _next(clip32, False), clip32 * 1.01, clip32 * 1.5])[k]
    tz = torch.where(m, near, tz)
    scales = torch.where(m[:, None], scales * clip32 * 0.3, scales)
    tz = torch.where(F("behind"), -r(0.1, 3.0), tz)
    # scale 1e-6 (the blur is all there is: compensation near 0) and exactly 0 (compensation 0)
    m = F("tiny_scale")
    scales = torch.where(m[:, None], torch.where((k % 2 == 0)[:, None], torch.tensor(1e-6), torch.tensor(0.0)) / glob
                         * torch.ones(n, 3), scales)
    scales = torch.where(F("needle")[:, None], torch.tensor([1e-4, 1e-4, 0.5]) / glob * torch.ones(n, 3), scales)
    quats = torch.where(F("qnorm_1e-3")[:, None], quats * 1e-3, quats)
    quats = torch.where(F("qnorm_1e3")[:, None], quats * 1e3, quats)
    # centre left of / above pixel 0 by a few pixels, wide enough (about 0.1 side) to reach back in
    m = F("negative_pixels")
    ax = torch.where(m, (-cx - r(1.0, 0.05 * side + 1.0)) / fx, ax)
    ay = torch.where(m & (k % 2 == 0), (-cy - r(1.0, 0.05 * side + 1.0)) / fy, ay)
    scales = torch.where(m[:, None], (tz * 0.1 * side / fx)[:, None] * torch.stack([r(0.5, 1), r(0.5, 1), r(0.5, 1)], -1)
                         / glob, scales)
    scales = torch.where(F("covers_all_tiles")[:, None], torch.stack([r(3, 5), r(3, 5), r(3, 5)], -1) / glob, scales)
    # far off screen and small: the tile box is empty
    m = F("area_culled")
    ax = torch.where(m, lim_x * r(3.0, 5.0), ax)
    # zero, denormal-norm and NaN quaternions
    m = F("bad_quat")
    bad = torch.stack([torch.zeros(n, 4), quats * 1e-30, quats * float("nan")])[k % 3, torch.arange(n)]
    quats = torch.where(m[:, None], bad, quats)
    cam = torch.stack([ax * tz, ay * tz, tz], -1)
    means = torch.stack([cam[:, 2], cam[:, 0], cam[:, 1]], -1)  # world = P^T cam for the permutation camera
    viewmat = torch.tensor([[0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    v = lambda *s: torch.randn(n, *s, generator=g)
    sgn = lambda t: torch.where(t.abs() < 0.05, torch.full_like(t, 0.05), t)  # "all non-zero"
    return dict(config=config, n=n, W=W, H=H, bw=bw, glob_scale=glob, clip_thresh=clip32, fx=fx, fy=fy, cx=cx, cy=cy,
                feat=feat, means=means.to(f32).contiguous(), scales=scales.to(f32).contiguous(),
                quats=quats.to(f32).contiguous(), viewmat=viewmat, lim=(lim_x, lim_y),
                v_xy=sgn(v(2)), v_depth=sgn(v()), v_conic=sgn(v(3)), v_compensation=sgn(v()))


def proj_forward(c: Dict):
    return gsplat_ref.project_gaussians(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"], c["fx"],
                                        c["fy"], c["cx"], c["cy"], c["H"], c["W"], c["bw"], clip_thresh=c["clip_thresh"])


def proj_backward_ref(c: Dict, fwd, dtype, upstream=None):
    """(v_mean, v_scale, v_quat, v_cov2d, v_cov3d) of the restatement in `dtype` on the fp32 forward outputs."""
    xys, depths, radii, conics, comp, tiles, cov3d = fwd
    u = upstream or (c["v_xy"], c["v_depth"], c["v_conic"], c["v_compensation"])
    return gsplat_ref.project_gaussians_backward(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"],
                                                 c["fx"], c["fy"], cov3d, radii, conics, comp, *u, dtype=dtype,
                                                 return_cov=True)


def clamp_active(c: Dict) -> torch.Tensor:
    """Rows whose camera-space centre lies beyond the 1.3 tan(fov) frustum clamp of the EWA Jacobian."""
    m = c["means"].double()
    tx, ty, tz = m[:, 1], m[:, 2], m[:, 0]
    return ((tx / tz).abs() > c["lim"][0]) | ((ty / tz).abs() > c["lim"][1])


# ---------------------------------------------------------------------------------------------------------------
# fp64 autograd of the plain references on the cases above
def raster_autograd(name: str, bw: int = 16, v_out=None, v_out_alpha=None, drop_batch_last: bool = False,
                    **variant):
    """Gradients of L = sum(rgb v_out) + sum(alpha_out v_out_alpha) through render_grad_ref.composite_masked in
    fp64, tile by tile over the oracle's lists: (v_xy, v_conic, v_rgb, v_opacity[n,1], v_xy_abs, T_last[H,W]).
    The contributing mask is data: valid = not (sigma < 0 or alpha < 1/255) and position <= final_idx, both from
    the fp32 forward state.  `variant` goes to composite_masked (wrong variants); drop_batch_last masks out the
    record a 256-batch loop would lose if it dropped each full batch's last slot."""
    from . import render_grad_ref
    c, s = raster_case(name), raster_state(name, bw)
    W, H = c["W"], c["H"]
    v_out = (c["v_out"] if v_out is None else v_out).to(f64)
    v_out_alpha = (c["v_out_alpha"] if v_out_alpha is None else v_out_alpha).to(f64)
    leaves = [c[k].to(f64).clone().requires_grad_(True) for k in ("xys", "conics", "colors", "opacities")]
    xys, conics, colors, op = leaves
    sig32, al32 = pair_terms(c, f32)
    loss = torch.zeros((), dtype=f64)
    offs, T_img = [], torch.ones(H, W, dtype=f64)
    for t in range(s["bins"].shape[0]):
        r0, r1 = int(s["bins"][t, 0]), int(s["bins"][t, 1])
        px, py, inside = gsplat_ref._tile_pixels(t % s["tx"], t // s["tx"], bw, H, W)
        if r1 <= r0 or not bool(inside.any()):
            continue
        px, py = px[inside], py[inside]
        pp = py * W + px
        g = s["gids"][r0:r1].long()
        pos = torch.arange(r0, r1)
        valid = ~((sig32[pp][:, g] < 0) | (torch.clamp(al32[pp][:, g], max=0.999) < 1.0 / 255.0))
        if drop_batch_last:
            valid = valid & (((r1 - 1 - pos) % 256) != 255)[None]
        off = torch.zeros(pp.numel(), g.numel(), 2, dtype=f64, requires_grad=True)
        pix = torch.stack([px.to(f64) + 0.5, py.to(f64) + 0.5], -1)
        rgb, a_out, T_last = render_grad_ref.composite_masked(
            pix, xys, conics, colors, op, c["background"].to(f64), g, valid, pos, s["final_idx"][py, px],
            pair_offset=off, **variant)
        loss = loss + (rgb * v_out[py, px]).sum() + (a_out * v_out_alpha[py, px]).sum()
        offs.append((g, off))
        T_img[py, px] = T_last.detach()
    grads = torch.autograd.grad(loss, leaves + [o for _, o in offs], allow_unused=True)
    v_xy, v_conic, v_rgb, v_op = [torch.zeros_like(l) if x is None else x for x, l in zip(grads[:4], leaves)]
    v_abs = torch.zeros(c["n"], 2, dtype=f64)
    for (g, _), go in zip(offs, grads[4:]):
        v_abs.index_add_(0, g, go.abs().sum(0))
    return v_xy, v_conic, v_rgb, v_op, v_abs, T_img


def proj_autograd(c: Dict, upstream, normalise_quats: bool = False, frustum_lim=None):
    """fp64 autograd of render_grad_ref.project_smooth on the case's fp32 inputs with the given upstream
    (v_xy, v_depth, v_conic, v_compensation): (v_mean, v_scale, v_quat, v_cov2d, v_cov3d) and the forward outputs.
    The quaternion is normalised in fp64 first and v_quat is the gradient with respect to that unit quaternion;
    normalise_quats instead differentiates through q / |q| (the gradient of the raw quaternion)."""
    from . import render_grad_ref
    m, sc, q = [c[k].to(f64).clone() for k in ("means", "scales", "quats")]
    if not normalise_quats:  # evaluated at the unit quaternion, which is the variable gsplat's v_quat refers to
        q = q / q.norm(dim=-1, keepdim=True)
    m, sc, q = m.requires_grad_(True), sc.requires_grad_(True), q.requires_grad_(True)
    qq = q / q.norm(dim=-1, keepdim=True) if normalise_quats else q
    out = render_grad_ref.project_smooth(m, sc, c["glob_scale"], qq, c["viewmat"], c["fx"], c["fy"], c["cx"], c["cy"],
                                         frustum_lim=frustum_lim)
    xys, depths, conics, comp, cov2d, cov3d = out
    v_xy, v_depth, v_conic, v_comp = [u.to(f64) for u in upstream]
    loss = (xys * v_xy).sum() + (depths * v_depth).sum() + (conics * v_conic).sum() + (comp * v_comp).sum()
    return torch.autograd.grad(loss, [m, sc, q, cov2d, cov3d]), [o.detach() for o in out]


# ---------------------------------------------------------------------------------------------------------------
# The training prep's backward chain (glue + projection + SH over 2 views) from the raw attributes
CHAIN_ATTRS = ["means", "scales", "quats", "opacities", "features_dc", "features_rest"]


def _look_at(eye, target):
    """camera_to_world [4,4], OpenGL axes (the camera looks along -z)."""
    eye, target = torch.tensor(eye, dtype=f64), torch.tensor(target, dtype=f64)
    back = (eye - target) / (eye - target).norm()
    right = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0], dtype=f64), back)
    right = right / right.norm()
    up = torch.linalg.cross(back, right)
    c2w = torch.eye(4, dtype=f64)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, eye
    return c2w.to(f32)


@functools.lru_cache(maxsize=None)
def chain_case() -> Dict:
    """300 Gaussians in the unit cube seen by two zoomed-in cameras 2.2 away (part of the cube outside each image,
    so the per-view masks matter; no live Gaussian beyond the frustum clamp, which gsplat's vjp ignores), SH
    degree 1, raw attributes as the heads emit them: log scales, unnormalised quaternions (norms 0.5 .. 2),
    logits."""
    g = gen(53)
    n, W, H = 300, 64, 48
    r = lambda *s: torch.randn(*s, generator=g)
    s = dict(means=torch.rand(n, 3, generator=g), scales=torch.log(_u(g, n * 3, 0.005, 0.02)).reshape(n, 3),
             quats=r(n, 4) * _u(g, n, 0.5, 2.0)[:, None], opacities=r(n, 1), features_dc=0.5 * r(n, 3),
             features_rest=0.4 * r(n, 3, 3))
    c2ws = torch.stack([_look_at((2.5, 0.0, 1.3), (0.5, 0.5, 0.5)), _look_at((-0.9, 2.1, -0.2), (0.5, 0.5, 0.5))])
    return dict(n=n, W=W, H=H, deg=1, fx=200.0, fy=190.0, cx=30.5, cy=25.0, scene=s, c2ws=c2ws,
                v_xys=r(2, n, 2), v_conics=r(2, n, 3), v_rgbs=r(2, n, 3), v_opacities=r(2, n))


@functools.lru_cache(maxsize=None)
def chain_forward():
    """Per view: the canonical glue and the oracle's fp32 projection (what the prep backward is handed)."""
    from . import render_ref
    c = chain_case()
    views = []
    for v in range(2):
        a = render_ref.glue_args(c["scene"], c["c2ws"][v], canonical=True)
        proj = gsplat_ref.project_gaussians(a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], c["fx"], c["fy"],
                                            c["cx"], c["cy"], c["H"], c["W"], 16)
        views.append((a, proj))
    return views


def chain_restated(dtype) -> Dict[str, torch.Tensor]:
    """The chain through the restatements in `dtype` (project_gaussians_backward, spherical_harmonics_bwd, the
    glue derivatives by torch autograd in `dtype`) on the fp32 forward outputs."""
    c, views = chain_case(), chain_forward()
    n, nb = c["n"], (c["deg"] + 1) ** 2
    Vm, Vs, Vq = torch.zeros(n, 3, dtype=dtype), torch.zeros(n, 3, dtype=dtype), torch.zeros(n, 4, dtype=dtype)
    Vop, Vcol = torch.zeros(n, 1, dtype=dtype), torch.zeros(n, nb, 3, dtype=dtype)
    z = torch.zeros(n)
    for v, (a, proj) in enumerate(views):
        xys, depths, radii, conics, comp, tiles, cov3d = proj
        live = (radii > 0)[:, None]
        vm, vs, vq = gsplat_ref.project_gaussians_backward(
            a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], c["fx"], c["fy"], cov3d, radii, conics, comp,
            c["v_xys"][v], z, c["v_conics"][v], z, dtype=dtype)
        Vm, Vs, Vq = Vm + vm, Vs + vs, Vq + vq
        Vop = Vop + torch.where(live, c["v_opacities"][v][:, None].to(dtype), torch.zeros(n, 1, dtype=dtype))
        pre = gsplat_ref.spherical_harmonics(c["deg"], a["viewdirs"], a["colors"])
        gate = live & (pre + 0.5 >= 0)  # clamp(rgb + 0.5, min=0) passes the gradient where rgb + 0.5 >= 0
        Vcol = Vcol + gsplat_ref.spherical_harmonics_bwd(
            c["deg"], a["viewdirs"], torch.where(gate, c["v_rgbs"][v], torch.zeros(n, 3)), nb, dtype=dtype)
    lv = {k: t.to(dtype).clone().requires_grad_(True) for k, t in c["scene"].items()}
    q = lv["quats"] / lv["quats"].norm(dim=-1, keepdim=True)
    colors = torch.cat([lv["features_dc"].unsqueeze(1), lv["features_rest"]], 1)
    total = (lv["means"] * Vm).sum() + (torch.exp(lv["scales"]) * Vs).sum() + (q * Vq).sum() \
        + (torch.sigmoid(lv["opacities"]) * Vop).sum() + (colors * Vcol).sum()
    total.backward()
    return {k: t.grad for k, t in lv.items()}


@functools.lru_cache(maxsize=None)
def chain_autograd() -> Dict[str, torch.Tensor]:
    """fp64 autograd of glue + render_grad_ref.project_smooth + SH from the raw attributes: no restatement
    involved.  Per view only the Gaussians the fp32 forward kept (radii > 0) enter the loss; view directions are
    detached, as the reference takes them from means.detach()."""
    from . import render_grad_ref
    c, views = chain_case(), chain_forward()
    lv = {k: t.to(f64).clone().requires_grad_(True) for k, t in c["scene"].items()}
    scales, op = torch.exp(lv["scales"]), torch.sigmoid(lv["opacities"])
    q = lv["quats"] / lv["quats"].norm(dim=-1, keepdim=True)
    colors = torch.cat([lv["features_dc"].unsqueeze(1), lv["features_rest"]], 1)
    loss = torch.zeros((), dtype=f64)
    for v, (a, proj) in enumerate(views):
        c2w = c["c2ws"][v].to(f64)
        R = torch.stack([c2w[:3, 0], -c2w[:3, 1], -c2w[:3, 2]], 1)
        vm = torch.cat([R.T, -(R.T @ c2w[:3, 3:4])], 1)
        xys, depths, conics, comp, _, _ = render_grad_ref.project_smooth(lv["means"], scales, 1.0, q, vm, c["fx"],
                                                                         c["fy"], c["cx"], c["cy"])
        dirs = (lv["means"] - c2w[:3, 3]).detach()
        rgb = torch.clamp(render_grad_ref.sh_colors(c["deg"], dirs, colors) + 0.5, min=0.0)
        live = proj[2] > 0
        for val, up in ((xys, c["v_xys"][v]), (conics, c["v_conics"][v]), (rgb, c["v_rgbs"][v]),
                        (op, c["v_opacities"][v][:, None])):
            loss = loss + (val * up.to(f64))[live].sum()
    grads = torch.autograd.grad(loss, [lv[k] for k in CHAIN_ATTRS])
    return dict(zip(CHAIN_ATTRS, grads))
