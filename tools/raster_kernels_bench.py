"""Every rasterizer kernel on one scene, for per-call times under `rocprofv3 --kernel-trace --stats` (no timing of
its own): 100k Gaussians at 800x800, block width 16, `reps` iterations of
  rasterize_gaussians C = 3, forward + backward, culled list   -> rasterize_fwd_quad_kernel, rasterize_bwd_quad_kernel
  the same on gsplat's full list                               -> rasterize_fwd_kernel, rasterize_bwd_kernel
  C = 4 and C = 32, forward + backward, full list              -> rasterize_fwd_nd_kernel / rasterize_bwd_nd_kernel<4 | 32>
  sfx_pack_raster_records + sfx_rasterize_fwd_views_packed     -> rasterize_fwd_packed_kernel
usage: [SFX_LIB=lib.so] rocprofv3 --kernel-trace --stats ... -- python tools/raster_kernels_bench.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import render_ref  # noqa: E402
from splatformer_amd import _lib, gsplat_compat as gc  # noqa: E402
from splatformer_amd.scenes import make_cameras, make_scene  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    dev = torch.device("cuda:0")
    W = H = 800
    bw = 16
    s = make_scene(100_000, 1, seed=0)
    cams = make_cameras(W, H, n_views=2)
    a = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in
         render_ref.glue_args(s, cams["camera_to_worlds"][1], canonical=False).items()}
    g = torch.Generator().manual_seed(5)
    n = a["means"].shape[0]
    colors = torch.rand(n, 32, generator=g).to(dev)
    bg = torch.rand(32, generator=g).to(dev)
    with torch.no_grad():
        xys, depths, radii, conics, _, tiles, _ = gc.project_gaussians(
            a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"], cams["cx"], cams["cy"], H, W,
            bw)
        num, cum = gc.compute_cumulative_intersects(tiles)
        _, _, _, gids, bins = gc.bin_and_sort_gaussians(n, num, xys, depths, radii, cum, ((W + 15) // 16, (H + 15) // 16, 1),
                                                         bw)
    op = a["opacities"].contiguous()
    rec = torch.empty(n, 16, device=dev)
    out = dict(img=torch.empty(H, W, 3, device=dev), al=torch.empty(H, W, device=dev), fT=torch.empty(H, W, device=dev),
               fi=torch.empty(H, W, device=dev, dtype=torch.int32))
    cull0 = gc.CULL
    for _ in range(reps):
        for cull, C in ((True, 3), (False, 3), (False, 4), (False, 32)):
            gc.CULL = cull
            leaves = [t.clone().requires_grad_(True) for t in (xys, conics, colors[:, :C].contiguous(), op)]
            img, alpha = gc.rasterize_gaussians(leaves[0], depths, radii, leaves[1], tiles, leaves[2], leaves[3], H, W, bw,
                                                bg[:C].contiguous(), return_alpha=True)
            (img.sum() + alpha.sum()).backward()
        c3 = colors[:, :3].contiguous()
        _lib.call("sfx_pack_raster_records", n, xys.data_ptr(), conics.data_ptr(), c3.data_ptr(), op.data_ptr(),
                  rec.data_ptr(), _lib.stream())
        _lib.call("sfx_rasterize_fwd_views_packed", 1, (W + 15) // 16, (H + 15) // 16, bw, H, W, gids.data_ptr(),
                  bins.data_ptr(), rec.data_ptr(), bg.data_ptr(), 0, out["fT"].data_ptr(), out["fi"].data_ptr(),
                  out["img"].data_ptr(), out["al"].data_ptr(), _lib.stream())
    gc.CULL = cull0
    torch.cuda.synchronize()
    print(f"{reps} iterations, {n} Gaussians, {num} intersections (library {os.environ.get('SFX_LIB', 'in-tree')})")


if __name__ == "__main__":
    main()
