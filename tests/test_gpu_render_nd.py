"""N-channel rasterizer (sfx_rasterize_fwd_nd / sfx_rasterize_bwd_nd, gsplat_compat.rasterize_gaussians with
C != 3, gs_render.rasterize_gaussians_to_rgbd) vs the gsplat v0.1.11 CPU oracle.

The oracle (oracle/gsplat_ref.py) is 3-channel; compositing is linear per channel, so it is an exact reference
for any C run once per channel triple: colours, background and v_out zero-padded to the triple, outputs and v_rgb
concatenated, v_xy / v_conic / v_opacity summed over the triples, v_out_alpha passed with the first triple only
(its own summation noise at C = 32: 5e-7 of the gradients' maximum).  Every channel count of this file is a
prefix of ONE set of 35 random channels, so a triple is computed once and shared between the cases.

Bars: the 3-channel tests' (tests/test_gpu_render.py) -- images and alphas 2e-4 absolute and mean |err| < 1e-6,
gradients max |err| / max |value| < 2e-4.
"""
import functools

import pytest
import torch

from oracle import gsplat_ref, render_ref
from splatformer_amd import gs_render, gsplat_compat
from splatformer_amd.scenes import make_cameras, make_scene, to_device

pytestmark = pytest.mark.gpu

W, H = 100, 70
CMAX = 35


class _Case:
    """The scene of this file projected by the oracle at one block width, its oracle binning, and the oracle's
    forward / backward per channel triple (cached)."""

    def __init__(self, bw):
        s = make_scene(3000, 1, seed=31)
        s["scales"] = s["scales"] + 1.5
        cams = make_cameras(W, H, n_views=2)
        a = render_ref.glue_args(s, cams["camera_to_worlds"][1])
        self.bw = bw
        self.proj = gsplat_ref.project_gaussians(a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"],
                                                 cams["fy"], cams["cx"], cams["cy"], H, W, bw)
        self.xys, self.depths, self.radii, self.conics, _, self.tiles, _ = self.proj
        self.opac = a["opacities"]
        self.tx, self.ty = (W + bw - 1) // bw, (H + bw - 1) // bw
        _, self.gids, self.bins = gsplat_ref.bin_and_sort_gaussians(self.xys, self.depths, self.radii, self.tiles,
                                                                    self.tx, self.ty, bw)
        g = torch.Generator().manual_seed(77)
        n = self.xys.shape[0]
        self.colors = torch.rand(n, CMAX, generator=g)
        self.bg = torch.rand(CMAX, generator=g)
        self.v_out = torch.randn(H, W, CMAX, generator=g)
        self.v_alpha = torch.randn(H, W, generator=g)

    @staticmethod
    def _pad3(t, s, e):
        out = t.new_zeros(*t.shape[:-1], 3)
        out[..., :e - s] = t[..., s:e]
        return out

    @functools.lru_cache(maxsize=None)
    def fwd_triple(self, s, e):
        """-> (out [H,W,e-s], final_T, final_idx) of channels [s, e), e - s <= 3."""
        out, fT, fidx = gsplat_ref.rasterize_forward(self.tx, self.ty, self.bw, H, W, self.gids, self.bins, self.xys,
                                                     self.conics, self._pad3(self.colors, s, e), self.opac,
                                                     self._pad3(self.bg, s, e))
        return out[..., :e - s], fT, fidx

    @functools.lru_cache(maxsize=None)
    def bwd_triple(self, s, e):
        _, fT, fidx = self.fwd_triple(0, min(3, CMAX))  # the geometry does not depend on the colours
        va = self.v_alpha if s == 0 else torch.zeros_like(self.v_alpha)
        v_xy, v_conic, v_rgb, v_op = gsplat_ref.rasterize_backward(
            self.tx, self.ty, self.bw, H, W, self.gids, self.bins, self.xys, self.conics,
            self._pad3(self.colors, s, e), self.opac, self._pad3(self.bg, s, e), fT, fidx,
            self._pad3(self.v_out, s, e), va)
        return v_xy, v_conic, v_rgb[:, :e - s], v_op

    @staticmethod
    def _triples(C):
        return [(s, min(s + 3, C)) for s in range(0, C, 3)]

    def forward(self, C):
        parts = [self.fwd_triple(s, e) for s, e in self._triples(C)]
        return torch.cat([p[0] for p in parts], -1), 1 - parts[0][1], parts[0][1]

    def backward(self, C):
        parts = [self.bwd_triple(s, e) for s, e in self._triples(C)]
        return (sum(p[0] for p in parts), sum(p[1] for p in parts), torch.cat([p[2] for p in parts], -1),
                sum(p[3] for p in parts))

    def hip(self, device, C, grad=False, v_alpha=True):
        """gsplat_compat.rasterize_gaussians on the first C channels -> (img, alpha, leaves)."""
        t = lambda x: x.to(device).clone().requires_grad_(grad)
        leaves = [t(self.xys), t(self.conics), t(self.colors[:, :C].contiguous()), t(self.opac)]
        img, alpha = gsplat_compat.rasterize_gaussians(
            leaves[0], self.depths.to(device), self.radii.to(device), leaves[1], self.tiles.to(device), leaves[2],
            leaves[3], H, W, self.bw, background=self.bg[:C].to(device), return_alpha=True)
        if grad:
            loss = (img * self.v_out[..., :C].to(device)).sum()
            if v_alpha:
                loss = loss + (alpha * self.v_alpha.to(device)).sum()
            loss.backward()
        return img, alpha, leaves


@functools.lru_cache(maxsize=None)
def _case(bw):
    return _Case(bw)


def _check_forward(case, img, alpha, C):
    exp_img, exp_alpha, _ = case.forward(C)
    img, alpha = img.detach().cpu(), alpha.detach().cpu()
    assert img.shape == (H, W, C) and alpha.shape == (H, W)
    print(f"C={C} bw={case.bw}: img max|err| {float((img - exp_img).abs().max()):.3e} "
          f"mean {float((img - exp_img).abs().mean()):.3e}, alpha max|err| {float((alpha - exp_alpha).abs().max()):.3e}")
    torch.testing.assert_close(img, exp_img, rtol=0, atol=2e-4)
    torch.testing.assert_close(alpha, exp_alpha, rtol=0, atol=2e-4)
    assert (img - exp_img).abs().mean() < 1e-6


def _check_backward(case, leaves, C):
    errs = {}
    for nm, leaf, exp in zip(["v_xy", "v_conic", "v_colors", "v_opacity"], leaves, case.backward(C)):
        got = leaf.grad.cpu()
        assert got.shape == exp.shape
        errs[nm] = float((got - exp).abs().max() / exp.abs().max().clamp_min(1e-6))
    print(f"C={C} bw={case.bw}: " + ", ".join(f"{k} rel err {v:.3e}" for k, v in errs.items()))
    for nm, err in errs.items():
        assert err < 2e-4, f"{nm}: rel err {err}"


def test_scene_exercises_the_kernel_paths(device):
    """What the cases below rely on: partial edge tiles, tile lists spanning several LDS batches, and pixels
    that stop early."""
    case = _case(16)
    assert W % 16 and H % 16
    lens = (case.bins[:, 1] - case.bins[:, 0])
    assert int(lens.max()) > 512
    _, _, fT = case.forward(1)
    assert int((fT < 1e-3).sum()) >= 100


@pytest.mark.parametrize("C", [1, 2, 4, 5, 8, 17, 32])
def test_forward_matches_oracle_culled_list(device, C):
    assert gsplat_compat.CULL
    case = _case(16)
    img, alpha, _ = case.hip(device, C)
    _check_forward(case, img, alpha, C)


@pytest.mark.parametrize("C", [1, 2, 4, 5, 8, 17, 32])
def test_forward_matches_oracle_full_list_bw8(device, C):
    case = _case(8)  # block_width 8 never culls: gsplat's full 3-sigma list, one wave per tile
    img, alpha, _ = case.hip(device, C)
    _check_forward(case, img, alpha, C)


def test_forward_full_list_bw16_equals_culled(device, monkeypatch):
    """The culled list drops only records every pixel skips: the outputs do not depend on the list."""
    case = _case(16)
    img_c, alpha_c, _ = case.hip(device, 8)
    monkeypatch.setattr(gsplat_compat, "CULL", False)
    img_f, alpha_f, _ = case.hip(device, 8)
    _check_forward(case, img_f, alpha_f, 8)
    assert torch.equal(img_c, img_f) and torch.equal(alpha_c, alpha_f)


def test_four_channels_with_zero_fourth_match_three_channel_kernels(device):
    case = _case(16)
    d = lambda x: x.to(device)
    col4 = torch.cat([case.colors[:, :3], torch.zeros(case.colors.shape[0], 1)], 1)
    bg4 = torch.cat([case.bg[:3], torch.zeros(1)])
    args = (d(case.xys), d(case.depths), d(case.radii), d(case.conics), d(case.tiles))
    img4, a4 = gsplat_compat.rasterize_gaussians(*args, d(col4), d(case.opac), H, W, 16, background=d(bg4),
                                                 return_alpha=True)
    img3, a3 = gsplat_compat.rasterize_gaussians(*args, d(case.colors[:, :3].contiguous()), d(case.opac), H, W, 16,
                                                 background=d(case.bg[:3]), return_alpha=True)
    assert img4.shape == (H, W, 4)
    torch.testing.assert_close(img4[..., :3], img3, rtol=0, atol=2e-4)
    torch.testing.assert_close(a4, a3, rtol=0, atol=2e-4)
    assert float(img4[..., 3].abs().max()) == 0.0


@pytest.mark.parametrize("C", [1, 4, 8, 32])
def test_backward_matches_oracle(device, C):
    case = _case(16)
    img, alpha, leaves = case.hip(device, C, grad=True)
    _check_forward(case, img, alpha, C)
    _check_backward(case, leaves, C)
    assert leaves[0].absgrad.shape == (case.xys.shape[0], 2)
    # sum of |terms| >= |sum of terms| (two summation orders: up to rounding relative to the larger side)
    assert bool((leaves[0].absgrad * (1 + 1e-4) >= leaves[0].grad.abs()).all())
    assert float(leaves[0].absgrad.max()) > 0


@pytest.mark.parametrize("C", [2, 8])
def test_backward_matches_oracle_full_list_bw8(device, C):
    """One wave per tile over gsplat's full list; C = 2 takes the per-channel wave reduction, C = 8 the
    transposed one."""
    case = _case(8)
    _, _, leaves = case.hip(device, C, grad=True)
    _check_backward(case, leaves, C)


def test_slabs_35_channels(device):
    case = _case(16)
    img, alpha, leaves = case.hip(device, CMAX, grad=True)
    _check_forward(case, img, alpha, CMAX)
    _check_backward(case, leaves, CMAX)


def test_odd_block_width_partial_waves(device):
    """block_width 5: 25 pixels per tile in one wave whose other 39 lanes own no pixel."""
    case = _case(5)
    img, alpha, leaves = case.hip(device, 4, grad=True)
    _check_forward(case, img, alpha, 4)
    _check_backward(case, leaves, 4)


def test_uint8_colors_and_default_background(device):
    case = _case(16)
    d = lambda x: x.to(device)
    u8 = (case.colors[:, :4] * 255).to(torch.uint8)
    args = (d(case.xys), d(case.depths), d(case.radii), d(case.conics), d(case.tiles))
    img_u8 = gsplat_compat.rasterize_gaussians(*args, d(u8), d(case.opac), H, W, 16)
    img_f = gsplat_compat.rasterize_gaussians(*args, d(u8).float() / 255, d(case.opac), H, W, 16,
                                              background=torch.ones(4, device=device))
    assert img_u8.shape == (H, W, 4)
    assert torch.equal(img_u8, img_f)


def test_empty_and_culled(device):
    cams = make_cameras(32, 32, n_views=1)
    s = make_scene(50, 1, seed=1)
    s["means"] = s["means"] + 10.0  # far outside the frustum / behind: all culled
    a = render_ref.glue_args(s, cams["camera_to_worlds"][0])
    xys, depths, radii, conics, _, tiles, _ = gsplat_ref.project_gaussians(
        a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"], cams["cx"], cams["cy"], 32,
        32, 16)
    assert int(tiles.sum()) == 0
    g = torch.Generator().manual_seed(3)
    bg = torch.rand(5, generator=g)
    t = lambda x: x.to(device).clone().requires_grad_(True)
    leaves = [t(xys), t(conics), t(torch.rand(50, 5, generator=g)), t(a["opacities"])]
    img, alpha = gsplat_compat.rasterize_gaussians(leaves[0], depths.to(device), radii.to(device), leaves[1],
                                                   tiles.to(device), leaves[2], leaves[3], 32, 32, 16,
                                                   background=bg.to(device), return_alpha=True)
    assert torch.equal(img.cpu(), torch.ones(32, 32, 5) * bg)
    assert torch.equal(alpha.cpu(), torch.ones(32, 32))  # gsplat empty-branch quirk
    (img.sum() + alpha.sum()).backward()
    for leaf in leaves:
        assert leaf.grad is not None and float(leaf.grad.abs().max()) == 0.0


# ---- RGB-D ----------------------------------------------------------------------------------------------------
RW, RH = 96, 80


@functools.lru_cache(maxsize=None)
def _rgbd_ref():
    s = make_scene(1500, 1, seed=31)
    cams = make_cameras(RW, RH, n_views=2)
    cams["background_color"] = torch.tensor([0.3, 0.2, 0.1])
    c2w = cams["camera_to_worlds"][1]
    rgb, alpha, m = render_ref.rasterize_gaussians_to_singleimg(s, c2w, return_meta=True, **cams)
    tx, ty = (RW + 15) // 16, (RH + 15) // 16
    zcol = torch.cat([m["depths"][:, None], torch.zeros(m["depths"].shape[0], 2)], 1)
    dep, _, _ = gsplat_ref.rasterize_forward(tx, ty, 16, RH, RW, m["gids_sorted"], m["tile_bins"], m["xys"],
                                             m["conics"], zcol, m["opacities"], torch.zeros(3))
    return s, cams, c2w, rgb, alpha, dep[..., :1], float(m["depths"][m["radii"] > 0].max())


def test_rgbd_matches_oracle(device):
    s, cams, c2w, rgb_r, alpha_r, dep_r, zmax = _rgbd_ref()
    sd, cd = to_device(s, device), to_device(cams, device)
    with torch.no_grad():
        rgb, alpha, dep = gs_render.rasterize_gaussians_to_rgbd(sd, cd["camera_to_worlds"][1], **cd)
        _, _, dep_e = gs_render.rasterize_gaussians_to_rgbd(sd, cd["camera_to_worlds"][1], depth_mode="expected", **cd)
    assert rgb.shape == (RH, RW, 3) and alpha.shape == (RH, RW, 1) and dep.shape == (RH, RW, 1)
    torch.testing.assert_close(rgb.cpu(), rgb_r, rtol=0, atol=2e-4)
    torch.testing.assert_close(alpha.cpu(), alpha_r, rtol=0, atol=2e-4)
    tol = 2e-4 * max(1.0, zmax)
    print(f"depth max|err| {float((dep.cpu() - dep_r).abs().max()):.3e} (bar {tol:.3e}, max z {zmax:.3f})")
    torch.testing.assert_close(dep.cpu(), dep_r, rtol=0, atol=tol)
    live = alpha_r > 1e-3
    # expected = accumulated / alpha of the same pass (one rounding of the division)
    torch.testing.assert_close(dep_e[live.to(device)], (dep / alpha)[live.to(device)], rtol=1e-6, atol=0)
    assert float(dep_e[(alpha == 0)].abs().max() if bool((alpha == 0).any()) else 0.0) == 0.0
    with pytest.raises(ValueError):
        gs_render.rasterize_gaussians_to_rgbd(sd, cd["camera_to_worlds"][1], depth_mode="median", **cd)


def test_multirgbd_equals_per_view(device):
    s, cams, *_ = _rgbd_ref()
    sd, cd = to_device(s, device), to_device(cams, device)
    with torch.no_grad():
        rgbs, alphas, deps = gs_render.rasterize_gaussians_to_multirgbd(sd, cd)
        assert len(rgbs) == len(alphas) == len(deps) == 2
        for v in range(2):
            rgb, alpha, dep = gs_render.rasterize_gaussians_to_rgbd(sd, cd["camera_to_worlds"][v], **cd)
            assert torch.equal(rgbs[v], rgb) and torch.equal(alphas[v], alpha) and torch.equal(deps[v], dep)


def test_rgbd_depth_gradient_reaches_means(device):
    """d(depth.sum()) / d(means) through the 4-channel backward (v_xy, v_conic and v_depth = v_colors[:, 3]) and the
    projection backward, against the oracle chain on the oracle's forward state."""
    s, cams, c2w, *_ = _rgbd_ref()
    a = render_ref.glue_args(s, c2w)
    xys, depths, radii, conics, comp, tiles, cov3d = gsplat_ref.project_gaussians(
        a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"], cams["cx"], cams["cy"], RH,
        RW, 16)
    tx, ty = (RW + 15) // 16, (RH + 15) // 16
    _, gids, bins = gsplat_ref.bin_and_sort_gaussians(xys, depths, radii, tiles, tx, ty, 16)
    zcol = torch.cat([depths[:, None], torch.zeros(depths.shape[0], 2)], 1)
    bg0 = torch.zeros(3)
    _, fT, fidx = gsplat_ref.rasterize_forward(tx, ty, 16, RH, RW, gids, bins, xys, conics, zcol, a["opacities"], bg0)
    v_out = torch.zeros(RH, RW, 3)
    v_out[..., 0] = 1.0
    v_xy, v_conic, v_rgb, _ = gsplat_ref.rasterize_backward(tx, ty, 16, RH, RW, gids, bins, xys, conics, zcol,
                                                           a["opacities"], bg0, fT, fidx, v_out, torch.zeros(RH, RW))
    v_mean, _, _ = gsplat_ref.project_gaussians_backward(a["means"], a["scales"], 1.0, a["quats"], a["viewmat"],
                                                         cams["fx"], cams["fy"], cov3d, radii, conics, comp, v_xy,
                                                         v_rgb[:, 0].contiguous(), v_conic, torch.zeros_like(depths))
    sd, cd = to_device(s, device), to_device(cams, device)
    sd["means"] = sd["means"].clone().requires_grad_(True)
    rgb, alpha, dep = gs_render.rasterize_gaussians_to_rgbd(sd, cd["camera_to_worlds"][1], **cd)
    dep.sum().backward()
    got = sd["means"].grad.cpu()
    err = float((got - v_mean).abs().max() / v_mean.abs().max().clamp_min(1e-6))
    print(f"means.grad rel err {err:.3e}")
    assert float(v_mean.abs().max()) > 0
    assert err < 2e-4, f"means.grad: rel err {err}"
