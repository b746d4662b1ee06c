"""The render backward kernels (sfx_rasterize_bwd / _bwd_quad / _bwd_views_quad, sfx_project_bwd, sfx_sh_bwd) and
the projection forward at their edges, against the fp64 restatements of oracle/gsplat_ref.py, which
tests/test_oracle_render_grad.py pins to fp64 autograd on the same inputs (oracle/render_cases.py).

Bars.  For each case and output, e32 = max |oracle_fp32 - oracle_fp64| / max |oracle_fp64|, computed here on the CPU
as the test runs; the kernel has to stay within FACTOR * e32 of the fp64 restatement (same norm), and FACTOR * e32
itself has to stay below a cap so the bar cannot drift loose: 2e-5 for the rasterizer, 5e-5 for projection outputs
of the near-plane and needle groups, 3e-5 elsewhere.  e32 enters the bar no smaller than 2^-24: a correctly rounded
fp32 result already lies up to 2^-24 from the exact one, and where the sequential fp32 sum happens to land closer
(1.6e-8 .. 2.1e-8 on the saturated case's v_xy_abs) another summation order cannot be asked to repeat the luck: the
kernels measured 1.2e-7 .. 2.5e-7 there, 6.3 to 12.0 x e32 depending on the order a run's atomics arrived in.
Measured on MI355X (two runs, profiles/render_grad_edges.txt): where e32 >= 2^-24 the kernels sit at most 3.7 x
e32 (rasterizer), 4.1 x (one projection row), 1.2 x (prep chain), 2.0 x (SH).  Nothing is excluded from a comparison: every rasterizer case
is clear of the backward's two discontinuities (asserted).  rel-L2 is printed next to every figure; run with -s.

Two cancellations in gsplat's projection vjp, both measured on the CPU, limit where the
projection caps can hold: `1 - compensation^2` and `one_m X - 0.3 inv_det` lose their digits as the fp32-rounded
compensation approaches 1 or 0 (e32 up to 1e-2 with v_compensation != 0), and a needle's v_scale / v_quat are the
difference of terms lambda_long / 0.3 times larger (e32 up to 2e-4 without it).  So the backward runs twice per
case: with all four upstream gradients non-zero, where the caps are asserted on the groups whose compensation
lies in [0.05, 0.995], and with v_compensation = 0, where they are asserted on every group (needle v_scale /
v_quat: NEEDLE_CAP, from the condition number).  The bar FACTOR * e32 applies to every group in both runs.
"""
import functools

import pytest
import torch

from oracle import gsplat_ref, render_cases as rc
from splatformer_amd import _lib, gsplat_compat

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
FACTOR = 8.0
EPS32 = 2.0 ** -24
RASTER_CAP = 2e-5
RASTER_OUT = ["v_xy", "v_conic", "v_rgb", "v_opacity", "v_xy_abs"]
PROJ_OUT = ["v_mean", "v_scale", "v_quat", "v_cov2d", "v_cov3d"]
# needle (1e-4, 1e-4, 0.5) at fx = 176, tz >= 2: lambda_long <= (0.5 * 176 / 2)^2 = 1936 against the 0.3 blur, so
# v_scale / v_quat cancel by up to 6.5e3; FACTOR * 6.5e3 * 2^-24 = 3.1e-3
NEEDLE_CAP = 5e-3


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def report(tag, nm, e32, err, l2, bar):
    print(f"\n[render-edges] {tag} {nm}: e32 {e32:.2e} kernel {err:.2e} ratio {err / max(e32, 1e-300):.2f} "
          f"rel-L2 {l2:.2e} bar {bar:.2e}", end="")


# ---- rasterizer backward -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raster_refs(name, bw, second=False):
    c = rc.raster_case(name)
    vo, va = (c["v_out2"], c["v_out_alpha2"]) if second else (c["v_out"], c["v_out_alpha"])
    return rc.raster_backward_ref(name, bw, f32, vo, va), rc.raster_backward_ref(name, bw, f64, vo, va)


def _check_raster(tag, got, r32, r64, extra=0.0, outputs=RASTER_OUT):
    bad = []
    for nm, o, a, b in zip(RASTER_OUT, got, r32, r64):
        if nm not in outputs:
            continue
        e32, err, l2 = rel(a, b), rel(o.cpu(), b), rel_l2(o.cpu(), b)
        bar = FACTOR * max(e32, EPS32) + extra
        report(tag, nm, e32, err, l2, bar)
        assert FACTOR * e32 <= RASTER_CAP, f"{tag} {nm}: the bar drifted loose, {FACTOR * e32:.2e}"
        if not err <= bar:
            bad.append(f"{nm}: {err:.2e} > {bar:.2e}")
    assert not bad, f"{tag}: {bad}"


def _dev(c, s, device):
    t = lambda x: x.to(device).contiguous()
    return dict(gids=t(s["gids"]), bins=t(s["bins"]), xys=t(c["xys"]), conics=t(c["conics"]), colors=t(c["colors"]),
                op=t(c["opacities"]), bg=t(c["background"]), fT=t(s["final_Ts"]), fidx=t(s["final_idx"]))


def _call_bwd(entry, c, s, d, v_out, v_out_alpha, outs, views=None):
    head = (views,) if views else ()
    _lib.call(entry, *head, s["tx"], s["ty"], s["bw"], c["H"], c["W"], d["gids"].data_ptr(), d["bins"].data_ptr(),
              d["xys"].data_ptr(), d["conics"].data_ptr(), d["colors"].data_ptr(), d["op"].data_ptr(),
              d["bg"].data_ptr(), d["fT"].data_ptr(), d["fidx"].data_ptr(), v_out.data_ptr(),
              None if v_out_alpha is None else v_out_alpha.data_ptr(), outs[0].data_ptr(),
              None if outs[4] is None else outs[4].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
              outs[3].data_ptr(), _lib.stream())
    torch.cuda.synchronize()


def _outs(n, device, fill=0.0, with_abs=True):
    mk = lambda *s: torch.full(s, fill, device=device, dtype=f32)
    return [mk(n, 2), mk(n, 3), mk(n, 3), mk(n, 1), mk(n, 2) if with_abs else None]


ENTRIES = [("sfx_rasterize_bwd", 16), ("sfx_rasterize_bwd", 8), ("sfx_rasterize_bwd_quad", 16)]


@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_rasterize_backward_entries(device, name):
    """The two single-view entries (block width 16 and 8 / the quad kernel) on the oracle's fp32 forward state."""
    c = rc.raster_case(name)
    for entry, bw in ENTRIES:
        s = rc.raster_state(name, bw)
        d = _dev(c, s, device)
        outs = _outs(c["n"], device)
        _call_bwd(entry, c, s, d, c["v_out"].to(device), c["v_out_alpha"].to(device), outs)
        _check_raster(f"{name} {entry}@{bw}", outs, *_raster_refs(name, bw))


@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_rasterize_backward_views_entry(device, name):
    """sfx_rasterize_bwd_views_quad over 3 views of one list: the case, an empty view (its v_out is random and
    must reach nothing), the case again with other upstream gradients.  Per-Gaussian operands and gradients are
    per (view, Gaussian); view 2's list positions and ids are offset as the batched forward lays them out."""
    c, s = rc.raster_case(name), rc.raster_state(name, 16)
    n, L, T = c["n"], s["gids"].numel(), s["bins"].shape[0]
    rep = lambda x: torch.cat([x, x, x], 0).to(device).contiguous()
    bins2 = torch.where(s["bins"][:, 1:2] > s["bins"][:, 0:1], s["bins"] + L, s["bins"])
    fidx2 = torch.where(s["final_Ts"] < 1, s["final_idx"] + L, s["final_idx"])  # untouched pixels keep 0
    g = rc.gen(77, rc.RASTER_CASES.index(name))
    d = dict(gids=torch.cat([s["gids"], s["gids"] + 2 * n]).to(device), xys=rep(c["xys"]), conics=rep(c["conics"]),
             bins=torch.cat([s["bins"], torch.zeros_like(s["bins"]), bins2]).to(device).contiguous(),
             colors=rep(c["colors"]), op=rep(c["opacities"]), bg=c["background"].to(device),
             fT=torch.stack([s["final_Ts"], torch.ones_like(s["final_Ts"]), s["final_Ts"]]).to(device),
             fidx=torch.stack([s["final_idx"], torch.zeros_like(fidx2), fidx2]).to(device).contiguous())
    v_out = torch.stack([c["v_out"], torch.randn(c["H"], c["W"], 3, generator=g), c["v_out2"]]).to(device)
    v_oa = torch.stack([c["v_out_alpha"], torch.randn(c["H"], c["W"], generator=g), c["v_out_alpha2"]]).to(device)
    outs = _outs(3 * n, device)
    _call_bwd("sfx_rasterize_bwd_views_quad", c, s, d, v_out.contiguous(), v_oa.contiguous(), outs, views=3)
    view = lambda v: [o[v * n:(v + 1) * n] for o in outs]
    for o in view(1):
        assert float(o.abs().max()) == 0.0, "the empty view received a gradient"
    _check_raster(f"{name} views_quad view0", view(0), *_raster_refs(name, 16))
    _check_raster(f"{name} views_quad view2", view(2), *_raster_refs(name, 16, True))


@pytest.mark.parametrize("entry,bw", ENTRIES)
@pytest.mark.parametrize("alpha_mode,with_abs,fill", [("null", True, 0.0), ("zeros", False, 0.0),
                                                      ("random", False, 0.5), ("random", True, 0.5)])
def test_rasterize_backward_nullable_and_accumulating_buffers(device, entry, bw, alpha_mode, with_abs, fill):
    """v_out_alpha NULL == zeros; v_xy_abs NULL leaves the other outputs as they are; outputs accumulate: buffers
    pre-filled with 0.5 end as 0.5 + gradient.  Each atomicAdd onto a pre-filled slot rounds at the size of
    0.5 + gradient; at most 64 land on one slot here (24 tile-waves at width 16, 15 tiles at width 8), so the
    pre-filled runs get 64 * 2^-24 * (0.5 + max|ref|) / max|ref| on top of the bar."""
    name = "partial_40x24"
    c, s = rc.raster_case(name), rc.raster_state(name, bw)
    d = _dev(c, s, device)
    va = None if alpha_mode == "null" else (torch.zeros_like(c["v_out_alpha"]) if alpha_mode == "zeros"
                                            else c["v_out_alpha"])
    ref_va = torch.zeros_like(c["v_out_alpha"]) if va is None else va
    r32 = rc.raster_backward_ref(name, bw, f32, c["v_out"], ref_va)
    r64 = rc.raster_backward_ref(name, bw, f64, c["v_out"], ref_va)
    outs = _outs(c["n"], device, fill, with_abs)
    _call_bwd(entry, c, s, d, c["v_out"].to(device), None if va is None else va.to(device), outs)
    got = [None if o is None else o.cpu().double() - fill for o in outs]
    small = min(float(b.abs().max()) for b in r64)
    extra = 64 * EPS32 * (fill + small) / small if fill else 0.0
    outputs = RASTER_OUT if with_abs else RASTER_OUT[:4]
    got = [torch.zeros_like(r64[4]) if o is None else o for o in got]
    _check_raster(f"{name} {entry}@{bw} alpha={alpha_mode} abs={with_abs} fill={fill}", got, r32, r64, extra, outputs)


def test_raster_cases_reach_the_paths_they_are_named_for():
    """From the oracle's fp64 pair terms and fp32 forward state (no GPU involved)."""
    cov = {name: rc.raster_coverage(name) for name in rc.RASTER_CASES}
    for name, v in cov.items():
        assert v["near"] == 0, f"{name}: {v['near']} pairs within {rc.NEAR} of a threshold"
        assert v["max_list"] <= 1100
    assert cov["partial_40x24"]["tiles"] == 6 and cov["px_17x17"]["tiles"] == 4 and cov["px_1x1"]["tiles"] == 1
    for k in (8, 9, 17, 255, 256, 257, 512, 513):  # every record of the list contributes at every pixel
        v = cov[f"batch_{k}"]
        assert v["max_list"] == k and v["sigma_pos"] == 256 * k and v["early_pixels"] == 0, (k, v)
    v = cov["saturated"]
    assert v["contrib_above_099"] >= 40 and v["contrib_above_0999"] >= 3, v
    v = cov["stack_early"]  # 3 batches; waves whose last contributor lies more than a batch before the list's end
    assert v["max_list"] > 512 and v["waves_skipping_a_batch"] >= 2 and v["lane_varied_waves"] >= 4, v
    assert v["quadrant_varied_tiles"] >= 1
    v = cov["empty_positions"]
    assert v["pixels_no_contributor_tile0"] >= 100 and v["empty_tiles"] >= 1 and v["tiles_offset_start"] >= 3, v
    v = cov["indefinite"]
    assert v["sigma_neg"] >= 1000 and v["sigma_pos"] >= 1000, v
    v = cov["cross_tile"]
    assert v["gaussians_in_all_tiles"] == 1 and v["tiles"] == 12, v
    assert rc.raster_coverage("cross_tile", 8)["gaussians_in_all_tiles"] == 1


def test_rasterize_operator_on_the_saturated_case(device):
    """gsplat_compat.rasterize_gaussians forward then backward on HIP's own forward state (plumbing: the culled
    list, the autograd Function, xys.absgrad), at the whole-operator bar of tests/test_gpu_render.py."""
    name = "saturated"
    c, s = rc.raster_case(name), rc.raster_state(name, 16)
    t = lambda x: x.to(device).clone().requires_grad_(True)
    xd, cd, rd, od = t(c["xys"]), t(c["conics"]), t(c["colors"]), t(c["opacities"])
    img, alpha = gsplat_compat.rasterize_gaussians(xd, c["depths"].to(device), c["radii"].to(device), cd,
                                                   s["tiles"].to(device), rd, od, c["H"], c["W"], 16,
                                                   background=c["background"].to(device), return_alpha=True)
    torch.testing.assert_close(img.detach().cpu(), s["img"], rtol=0, atol=2e-4)
    torch.testing.assert_close(alpha.detach().cpu(), 1 - s["final_Ts"], rtol=0, atol=2e-4)
    (img * c["v_out"].to(device)).sum().add_((alpha * c["v_out_alpha"].to(device)).sum()).backward()
    r32, r64 = _raster_refs(name, 16)
    for nm, got, exp in zip(RASTER_OUT, [xd.grad, cd.grad, rd.grad, od.grad, xd.absgrad], r64):
        err = rel(got.cpu(), exp)
        print(f"\n[render-edges] {name} operator {nm}: kernel {err:.2e} rel-L2 {rel_l2(got.cpu(), exp):.2e}", end="")
        assert err < 2e-4, f"{nm}: rel err {err}"


# ---- projection ----------------------------------------------------------------------------------------------------
PROJ_RUNS = [(cfg, None) for cfg in rc.PROJ_CONFIGS if not cfg.startswith("n1_")] + \
            [("n1_17x33_bw8", f) for f in rc.PROJ_FEATURES]


def _project_fwd(c, device):
    n = c["n"]
    t = lambda x: x.to(device).contiguous()
    m, sc, q, vm = t(c["means"]), t(c["scales"]), t(c["quats"]), t(c["viewmat"])
    e = lambda *s, dt=f32: torch.full((n, *s), -7, device=device, dtype=dt)  # every element must be written
    xys, depths, radii, conics, comp, tiles, cov3d = e(2), e(), e(dt=torch.int32), e(3), e(), e(dt=torch.int32), e(6)
    _lib.call("sfx_project_fwd", n, m.data_ptr(), sc.data_ptr(), c["glob_scale"], q.data_ptr(), vm.data_ptr(),
              c["fx"], c["fy"], c["cx"], c["cy"], c["H"], c["W"], c["bw"], c["clip_thresh"], xys.data_ptr(),
              depths.data_ptr(), radii.data_ptr(), conics.data_ptr(), comp.data_ptr(), tiles.data_ptr(),
              cov3d.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    return (m, sc, q, vm), (xys, depths, radii, conics, comp, tiles, cov3d)


@pytest.mark.parametrize("config,feature", PROJ_RUNS)
def test_project_forward_bit_equal(device, config, feature):
    """Every output bit-equal to the oracle (NaNs, which only the conics / cov3d of a culled non-finite quaternion
    carry, at the same places), on inputs that reach the frustum clamp, the near plane from both sides, both
    glob_scales, tiny and needle scales, scaled and non-finite quaternions."""
    c = rc.proj_case(config, feature)
    ref = rc.proj_forward(c)
    _, out = _project_fwd(c, device)
    names = ["xys", "depths", "radii", "conics", "comp", "num_tiles_hit", "cov3d"]
    for nm, r, o in zip(names, ref, out):
        o = o.cpu()
        assert r.dtype == o.dtype and r.shape == o.shape, nm
        if r.dtype == f32:
            assert torch.equal(torch.isnan(r), torch.isnan(o)), f"{nm}: NaNs at different places"
            r, o = torch.nan_to_num(r, nan=0.0), torch.nan_to_num(o, nan=0.0)
        mism = int((r != o).sum())
        assert mism == 0, f"{nm}: {mism} mismatches (max |d| {(r.double() - o.double()).abs().max().item():.3e})"
    live, feat = ref[2] > 0, c["feat"]
    F = lambda nm: feat == rc.PROJ_FEATURES.index(nm)
    if feature is None:  # the mixed configurations reach every path (counted on the oracle's outputs)
        assert int((live & rc.clamp_active(c) & F("beyond_clamp")).sum()) >= c["n"] // 13, "frustum clamp not active"
        assert int((live & F("near_plane")).sum()) > 0 and int((~live & F("near_plane")).sum()) > 0
        assert int((live & F("behind")).sum()) == 0 and int((live & F("bad_quat")).sum()) == 0
        assert bool((ref[0][live & F("negative_pixels")] < 0).any(1).all())
        tiles_all = ((c["W"] + c["bw"] - 1) // c["bw"]) * ((c["H"] + c["bw"] - 1) // c["bw"])
        assert bool((ref[5][F("covers_all_tiles")] == tiles_all).all())
        tiny = F("tiny_scale") & live
        assert float(ref[4][tiny].max()) < 1e-6 and float(ref[4][tiny].min()) == 0.0  # compensation near and at 0
    bad = F("bad_quat")
    if bool(bad.any()):  # the settled behaviour: culled, every output zero but the NaN conics / cov3d
        for nm, o in zip(names, out):
            o = o.cpu()[bad]
            if nm in ("conics", "cov3d"):
                assert bool(torch.isnan(o).all()), nm
            else:
                assert float(o.double().abs().max()) == 0.0, nm


def _proj_cap(feature, output):
    if feature == "needle" and output in ("v_scale", "v_quat"):
        return NEEDLE_CAP
    return 5e-5 if feature in ("near_plane", "needle") else 3e-5


@pytest.mark.parametrize("with_comp", [True, False], ids=["all_upstream", "no_v_compensation"])
@pytest.mark.parametrize("config,feature", PROJ_RUNS)
def test_project_backward(device, config, feature, with_comp):
    c = rc.proj_case(config, feature)
    fwd = rc.proj_forward(c)
    n, live = c["n"], fwd[2] > 0
    up = [c["v_xy"], c["v_depth"], c["v_conic"], c["v_compensation"] if with_comp else torch.zeros(n)]
    r32, r64 = rc.proj_backward_ref(c, fwd, f32, tuple(up)), rc.proj_backward_ref(c, fwd, f64, tuple(up))
    (m, sc, q, vm), out = _project_fwd(c, device)
    # culled rows: NaN upstream gradients, which the kernel must not read
    nan_rows = lambda u: torch.where(live.reshape(-1, *([1] * (u.dim() - 1))), u, torch.full_like(u, float("nan")))
    upd = [nan_rows(u).to(device).contiguous() for u in up]
    res = [torch.full((n, k), float("nan"), device=device) for k in (3, 3, 4, 3, 6)]
    _lib.call("sfx_project_bwd", n, m.data_ptr(), sc.data_ptr(), c["glob_scale"], q.data_ptr(), vm.data_ptr(),
              c["fx"], c["fy"], out[6].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
              *[u.data_ptr() for u in upd], *[r.data_ptr() for r in res], _lib.stream())
    torch.cuda.synchronize()
    res = [r.cpu() for r in res]
    for onm, o in zip(PROJ_OUT, res):
        assert not bool(torch.isnan(o).any()), f"{onm}: NaN or unwritten element"
        assert float(o[~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, f"{onm}: culled row not zero"
    bad = []
    for k, fnm in enumerate(rc.PROJ_FEATURES):
        rows = live & (c["feat"] == k)
        if not bool(rows.any()):
            continue
        well = bool(((fwd[4][rows] >= 0.05) & (fwd[4][rows] <= 0.995)).all())
        for onm, o, a, b in zip(PROJ_OUT, res, r32, r64):
            e32, err, l2 = rel(a[rows], b[rows]), rel(o[rows], b[rows]), rel_l2(o[rows], b[rows])
            bar = FACTOR * max(e32, EPS32)
            report(f"{config} {'all' if with_comp else 'nocomp'} {fnm}", onm, e32, err, l2, bar)
            if well or not with_comp:
                assert bar <= _proj_cap(fnm, onm), f"{fnm} {onm}: the bar drifted loose, {bar:.2e}"
            if not err <= bar:
                bad.append(f"{fnm} {onm}: {err:.2e} > {bar:.2e}")
    assert not bad, bad


# ---- the training prep's backward chain -------------------------------------------------------------------------------
def test_prep_views_backward_chain_against_fp64_autograd(device):
    """sfx_render_prep_project_views_bwd (project_bwd_point<false>, the SH backward and the glue derivatives in one
    kernel) over 2 views against fp64 autograd of glue + project_smooth + SH from the raw attributes -- no
    restatement in the reference.  The quaternion goes through q / |q|: the radial part of gsplat's v_quat has to
    vanish.  e32 is the fp32 restatement chain's error against the same reference."""
    c, views = rc.chain_case(), rc.chain_forward()
    ref, r32 = rc.chain_autograd(), rc.chain_restated(f32)
    n, nb = c["n"], (c["deg"] + 1) ** 2
    radii = torch.stack([p[2] for _, p in views])
    lim = gsplat_ref.fov_limits(c["fx"], c["fy"], c["W"], c["H"])
    for v, (a, p) in enumerate(views):  # coverage: per-view masks differ, the clamp gsplat's vjp ignores is inactive
        t = a["means"].double() @ a["viewmat"].double()[:, :3].T + a["viewmat"].double()[:, 3]
        act = ((t[:, 0] / t[:, 2]).abs() > lim[0]) | ((t[:, 1] / t[:, 2]).abs() > lim[1])
        assert int((act & (p[2] > 0)).sum()) == 0
    live = radii > 0
    assert int((live[0] != live[1]).sum()) >= 30 and int((~live.any(0)).sum()) >= 30
    sd = {k: t.to(device).contiguous() for k, t in c["scene"].items()}
    out = {k: torch.full_like(sd[k].reshape(n, -1), float("nan")) for k in rc.CHAIN_ATTRS}
    io = []
    for d in (sd, out):
        for k in rc.CHAIN_ATTRS:
            io += [d[k].data_ptr(), d[k].reshape(n, -1).shape[1]]
    conics = torch.stack([p[3] for _, p in views]).to(device).contiguous()
    dev = [c[k].to(device).contiguous() for k in ("v_xys", "v_conics", "v_rgbs", "v_opacities")]
    c2ws, rd = c["c2ws"].to(device).contiguous(), radii.to(device).contiguous()
    _lib.call("sfx_render_prep_project_views_bwd", n, 2, nb, *io[:12], c2ws.data_ptr(), c["fx"], c["fy"],
              rd.data_ptr(), conics.data_ptr(), *[g.data_ptr() for g in dev], *io[12:], _lib.stream())
    torch.cuda.synchronize()
    bad = []
    for k in rc.CHAIN_ATTRS:
        o, exp = out[k].cpu().reshape(ref[k].shape), ref[k]
        assert not bool(torch.isnan(o).any()), f"{k}: an element was not stored"
        assert float(o[~live.any(0)].abs().max()) == 0.0, f"{k}: a Gaussian dead in both views has a gradient"
        e32, err = rel(r32[k], exp), rel(o, exp)
        bar = FACTOR * max(e32, EPS32)
        report("chain", k, e32, err, rel_l2(o, exp), bar)
        assert bar <= 3e-5, f"{k}: the bar drifted loose, {bar:.2e}"
        if not err <= bar:
            bad.append(f"{k}: {err:.2e} > {bar:.2e}")
    q = c["scene"]["quats"].double()
    radial = (out["quats"].cpu().double() * q).sum(-1).abs() / q.norm(dim=-1)
    assert float(radial.max()) <= 1e-5 * float(ref["quats"].abs().max()), "v_quats keeps a radial part"
    assert not bad, bad


# ---- SH ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,deg,use", [(1, 4, 4), (1, 2, 0), (257, 4, 2), (257, 3, 1), (257, 1, 0), (2000, 4, 3)])
def test_sh_backward_below_the_allowed_degree(device, n, deg, use):
    """degrees_to_use below what num_bases allows: the unused coefficient rows get exactly zero (the buffer is
    pre-filled with NaN: every element is stored); the used ones match the fp64 restatement."""
    g = rc.gen(9, n, deg, use)
    nb = (deg + 1) ** 2
    dirs, v = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    out = torch.full((n, nb, 3), float("nan"), device=device)
    dd, vd = dirs.to(device), v.to(device)
    _lib.call("sfx_sh_bwd", n, nb, use, dd.data_ptr(), vd.data_ptr(), out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    out = out.cpu()
    r32 = gsplat_ref.spherical_harmonics_bwd(use, dirs, v, nb)
    r64 = gsplat_ref.spherical_harmonics_bwd(use, dirs, v, nb, dtype=f64)
    used = (use + 1) ** 2
    assert not bool(torch.isnan(out).any())
    assert float(out[:, used:].abs().max() if used < nb else 0.0) == 0.0
    # degree 0's basis is a constant: e32 can be 0 there; one rounding of the product is the floor
    e32 = max(rel(r32, r64), EPS32)
    err = rel(out, r64)
    report(f"sh n={n} deg={deg} use={use}", "v_coeffs", e32, err, rel_l2(out, r64), FACTOR * e32)
    assert FACTOR * e32 <= 3e-5 and err <= FACTOR * e32
