"""Same bits from two builds of libsfx: every forward tensor of the rasterizer on identical seeded inputs, one
process per library (SFX_LIB), then compared with torch.equal.
    SFX_LIB=/path/parent.so python tools/raster_same_bits.py dump a.pt
    SFX_LIB=/path/new.so    python tools/raster_same_bits.py dump b.pt
    python tools/raster_same_bits.py compare a.pt b.pt
Dumped: the calls of tests/test_gpu_raster_fwd_edges.py (every forward entry point on every oracle case, block
widths 16 and 8); gs_render.render_views_meta culled and unculled on the scene of
test_render_cull_bit_identical_adversarial (seed 0); gsplat_compat.rasterize_gaussians with C = 1, 3, 4, 5 and 32 at
block widths 16 (culled list) and 8 (gsplat's list).  Backward outputs go through float atomics and are not
reproducible run to run: they are not compared."""
import importlib.util
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def dump(path):
    from oracle import render_cases as rc, render_ref
    from splatformer_amd import gs_render, gsplat_compat
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    spec = importlib.util.spec_from_file_location("fwd_edges", os.path.join(ROOT, "tests", "test_gpu_raster_fwd_edges.py"))
    edges = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(edges)
    dev = torch.device("cuda:0")
    out = {}
    for name in rc.RASTER_CASES:
        for bw in (16, 8):
            for tag, o in edges.forward_entries(name, bw, dev).items():
                for nm, t in o.items():
                    out[f"edges/{name}@{bw}/{tag}/{nm}"] = t

    n = 6000  # the scene of tests/test_gpu_render.py test_render_cull_bit_identical_adversarial, seed 0
    g = torch.Generator().manual_seed(100)
    s = make_scene(n, 1, seed=0)
    logit = lambda p: math.log(p / (1.0 - p))
    k = torch.randint(0, 4, (n,), generator=g)
    op = s["opacities"].clone()
    near = torch.tensor([logit(1 / 255.0)]) + 1e-4 * torch.randn(n, 1, generator=g)
    op[k == 0] = near[k == 0]
    op[k == 1] = logit(0.999)
    s["opacities"] = op
    sc = s["scales"].clone()
    sc[k == 2, 0] = sc[k == 2, 0] + 3.0
    sc[k == 2, 1] = sc[k == 2, 1] - 3.0
    s["scales"] = sc
    sd, cd = to_device(s, dev), to_device(make_cameras(200, 136, n_views=3), dev)
    cull0 = gs_render.RENDER_CULL
    with torch.no_grad():
        for cull in (True, False):
            gs_render.RENDER_CULL = cull
            rgbs, alphas, meta = gs_render.render_views_meta(sd, cd)
            for v in range(3):
                out[f"views/cull{int(cull)}/rgb{v}"] = rgbs[v].cpu()
                out[f"views/cull{int(cull)}/alpha{v}"] = alphas[v].cpu()
            for nm in ("final_Ts", "final_idx", "gids_sorted", "isect_sorted"):
                if nm in meta:
                    out[f"views/cull{int(cull)}/{nm}"] = meta[nm].cpu()
    gs_render.RENDER_CULL = cull0

    W, H = 100, 70  # the scene of tests/test_gpu_render_nd.py
    s = make_scene(3000, 1, seed=31)
    s["scales"] = s["scales"] + 1.5
    cams = make_cameras(W, H, n_views=2)
    a = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in
         render_ref.glue_args(s, cams["camera_to_worlds"][1]).items()}
    g = torch.Generator().manual_seed(77)
    colors = torch.rand(a["means"].shape[0], 32, generator=g).to(dev)
    bg = torch.rand(32, generator=g).to(dev)
    with torch.no_grad():
        for bw in (16, 8):
            xys, depths, radii, conics, _, tiles, _ = gsplat_compat.project_gaussians(
                a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"], cams["cx"], cams["cy"],
                H, W, bw)
            for C in (1, 3, 4, 5, 32):
                img, alpha = gsplat_compat.rasterize_gaussians(xys, depths, radii, conics, tiles,
                                                               colors[:, :C].contiguous(), a["opacities"], H, W, bw,
                                                               bg[:C].contiguous(), return_alpha=True)
                out[f"compat/bw{bw}/C{C}/img"], out[f"compat/bw{bw}/C{C}/alpha"] = img.cpu(), alpha.cpu()
    torch.cuda.synchronize()
    torch.save(out, path)
    print(f"{len(out)} tensors -> {path} (library {os.environ.get('SFX_LIB', 'in-tree')})")


def compare(pa, pb):
    A, B = torch.load(pa), torch.load(pb)
    assert set(A) == set(B), sorted(set(A) ^ set(B))
    eq = lambda x, y: x.shape == y.shape and x.dtype == y.dtype and (
        torch.equal(x.view(torch.int32), y.view(torch.int32)) if x.dtype == torch.float32 else torch.equal(x, y))
    bad = [k for k in sorted(A) if not eq(A[k], B[k])]
    groups = {}
    for k in A:
        groups[k.split("/")[0]] = groups.get(k.split("/")[0], 0) + 1
    print(f"{len(A)} tensors ({', '.join(f'{v} {k}' for k, v in sorted(groups.items()))}): "
          f"{'all bit-identical' if not bad else f'{len(bad)} DIFFER: {bad[:10]}'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
