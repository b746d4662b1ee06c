"""The render oracle's three hand-written backward restatements (oracle/gsplat_ref.py rasterize_backward,
project_gaussians_backward, spherical_harmonics_bwd) pinned to fp64 autograd of plain forwards
(oracle/render_grad_ref.py) on the inputs of oracle/render_cases.py -- host only, no GPU.

1. Pins: where nothing non-smooth binds (opacities <= 0.95, no frustum clamp, unit quaternions, compensation away
   from 0, the contributing mask taken from the fp32 forward state) the fp64 restatement IS the autograd gradient
   (1e-9), and the fp32 restatement sits within the bars' caps of it.
2. The four places where gsplat's backward deliberately is not the autograd gradient, each shown on a case built
   for it, so nobody later "fixes" it.
3. Sensitivity: ten wrong variants of the backward each miss the bar tests/test_gpu_render_edges.py applies to the
   HIP kernels (8 x the fp32 restatement's own error, per case and output) on at least one of its cases.
"""
import pytest
import torch

from oracle import gsplat_ref, render_cases as rc, render_grad_ref as rg

f32, f64 = torch.float32, torch.float64
BAR_FACTOR = 8.0  # the GPU tests' bar: BAR_FACTOR * e32
RASTER_CAP = 2e-5
RASTER_OUT = ["v_xy", "v_conic", "v_rgb", "v_opacity", "v_xy_abs"]
PROJ_OUT = ["v_mean", "v_scale", "v_quat", "v_cov2d", "v_cov3d"]


def rel(a, b):
    """max |a - b| / max |b|"""
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


# ---- 1. pins ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bw", [("partial_40x24", 16), ("partial_40x24", 8), ("px_17x17", 16),
                                     ("empty_positions", 16), ("cross_tile", 16), ("batch_257", 16)])
def test_rasterize_backward_is_autograd_of_the_composite(name, bw):
    c, s = rc.raster_case(name), rc.raster_state(name, bw)
    assert float(c["opacities"].max()) <= 0.95  # the 0.99 clamp cannot bind
    *auto, T_last = rc.raster_autograd(name, bw)
    # fp64 restatement on the composite's own fp64 T: the same function, to rounding
    r64 = gsplat_ref.rasterize_backward(s["tx"], s["ty"], bw, c["H"], c["W"], s["gids"], s["bins"], c["xys"],
                                        c["conics"], c["colors"], c["opacities"], c["background"], T_last,
                                        s["final_idx"], c["v_out"], c["v_out_alpha"], dtype=f64, return_abs=True)
    # fp32 and fp64 restatement on the fp32 forward state (what the kernels are handed)
    s32 = rc.raster_backward_ref(name, bw, f32)
    s64 = rc.raster_backward_ref(name, bw, f64)
    assert rel(s["final_Ts"], T_last) < 1e-6
    for nm, a, x64, y32, y64 in zip(RASTER_OUT, auto, r64, s32, s64):
        assert float(a.abs().max()) > 0, nm
        assert rel(x64, a) < 1e-9, f"{nm}: fp64 restatement vs autograd {rel(x64, a):.2e}"
        assert rel(y64, a) < RASTER_CAP / BAR_FACTOR, f"{nm}: fp64 restatement on the fp32 T {rel(y64, a):.2e}"
        assert rel(y32, a) < RASTER_CAP / BAR_FACTOR, f"{nm}: fp32 restatement vs autograd {rel(y32, a):.2e}"


def _smooth_rows(c, fwd):
    """Live rows where nothing non-smooth binds: no frustum clamp, compensation in [0.05, 1) (the plain reference is evaluated at
    the normalised quaternion, so scaled quaternions are smooth rows too)."""
    return (fwd[2] > 0) & ~rc.clamp_active(c) & (fwd[4] >= 0.05)


@pytest.mark.parametrize("config", ["n255_17x33_bw8", "n2000_160x120_bw16"])
def test_project_backward_is_autograd_of_project_smooth(config):
    c = rc.proj_case(config)
    fwd = rc.proj_forward(c)
    rows = _smooth_rows(c, fwd)
    assert int(rows.sum()) >= c["n"] // 4
    up = (c["v_xy"], c["v_depth"], c["v_conic"], c["v_compensation"])
    # gsplat's 0.5 / (compensation + 1e-6) is autograd's 0.5 / compensation with v_compensation scaled
    _, out = rc.proj_autograd(c, up)
    comp64 = out[3]
    scaled = (c["v_xy"], c["v_depth"], c["v_conic"], c["v_compensation"].double() * comp64 / (comp64 + 1e-6))
    auto, out = rc.proj_autograd(c, scaled)
    xys, depths, conics, comp, cov2d, cov3d = out
    # fp64 restatement on project_smooth's own fp64 outputs: the same function
    r64 = gsplat_ref.project_gaussians_backward(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"],
                                                c["fx"], c["fy"], cov3d, fwd[2], conics, comp, *up, dtype=f64,
                                                return_cov=True)
    s32 = rc.proj_backward_ref(c, fwd, f32)
    # the forward agrees too (smooth rows): the plain reference describes the oracle's forward
    assert rel(fwd[0][rows], xys[rows]) < 1e-5 and rel(fwd[3][rows], conics[rows]) < 1e-4
    for k, nm in enumerate(rc.PROJ_FEATURES):
        m = rows & (c["feat"] == k)
        if not bool(m.any()):
            continue
        for onm, a, x64, y32 in zip(PROJ_OUT, auto, r64, s32):
            assert rel(x64[m], a[m]) < 1e-9, f"{nm} {onm}: fp64 restatement vs autograd {rel(x64[m], a[m]):.2e}"
            # fp32 restatement on the fp32 forward's rounded conics / cov3d / compensation, where 1 - comp^2
            # keeps its digits (as compensation -> 1 the fp32-rounded compensation itself loses them)
            w = m & (fwd[4] <= 0.995)
            if bool(w.any()):
                assert rel(y32[w], a[w]) < 5e-5, f"{nm} {onm}: fp32 restatement vs autograd {rel(y32[w], a[w]):.2e}"


@pytest.mark.parametrize("deg,use", [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (4, 2), (3, 0)])
def test_sh_backward_is_autograd_of_the_sh_forward(deg, use):
    g = rc.gen(5, deg, use)
    n, nb = 257, (deg + 1) ** 2
    dirs, v = torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g)
    coeffs = torch.randn(n, nb, 3, generator=g).double().requires_grad_(True)
    (rg.sh_colors(use, dirs, coeffs) * v.double()).sum().backward()
    b64 = gsplat_ref.spherical_harmonics_bwd(use, dirs, v, nb, dtype=f64)
    b32 = gsplat_ref.spherical_harmonics_bwd(use, dirs, v, nb)
    assert rel(b64, coeffs.grad) < 1e-14 and rel(b32, coeffs.grad) < 1e-6
    assert float(b32[:, (use + 1) ** 2:].abs().max() if use < deg else 0.0) == 0.0  # unused rows: exactly zero
    # the forward in fp64 is the oracle's forward
    assert rel(gsplat_ref.spherical_harmonics(use, dirs, coeffs.detach().float()),
               rg.sh_colors(use, dirs, coeffs.detach().float().double())) < 1e-5


def test_prep_chain_restated_is_autograd_from_the_raw_attributes():
    """glue + projection + SH over 2 views: the restatement chain on the fp32 forward's rounded conics / cov3d
    against fp64 autograd of the plain forwards from the raw attributes (q / |q| included)."""
    ref, r64, r32 = rc.chain_autograd(), rc.chain_restated(f64), rc.chain_restated(f32)
    for k in rc.CHAIN_ATTRS:
        assert float(ref[k].abs().max()) > 0
        assert rel(r64[k], ref[k]) < 3e-6 and rel(r32[k], ref[k]) < 3e-5 / BAR_FACTOR, k
    q = rc.chain_case()["scene"]["quats"].double()
    assert float((ref["quats"] * q).sum(-1).abs().max() / ref["quats"].abs().max()) < 1e-12  # no radial part


# ---- 2. the deliberate deviations from autograd -------------------------------------------------------------------
def test_deviation_backward_clamps_alpha_at_099_and_does_not_gate_v_sigma():
    """One pixel, one Gaussian with o exp(-sigma) > 0.999.  Forward: alpha = 0.999, T_final = 0.001.  gsplat's
    backward replays with alpha = 0.99: T = T_final / (1 - 0.99) = 0.1 instead of 1, so v_rgb = 0.99 * 0.1 * v_out
    (autograd: 0.999 * v_out), and it sends v_alpha on to sigma and the opacity although the clamp is active
    (autograd: exactly zero)."""
    xys, conics = torch.tensor([[0.75, 0.25]]), torch.tensor([[1e-3, 0.0, 2e-3]])
    colors, op, bg = torch.tensor([[0.2, 0.5, 0.9]]), torch.tensor([[1.0]]), torch.tensor([0.3, 0.2, 0.1])
    gids, bins = torch.zeros(1, dtype=torch.int32), torch.tensor([[0, 1]], dtype=torch.int32)
    img, fT, fidx = gsplat_ref.rasterize_forward(1, 1, 16, 1, 1, gids, bins, xys, conics, colors, op, bg)
    assert abs(float(fT) - 0.001) < 1e-7 and int(fidx) == 0
    v_out, v_oa = torch.tensor([[[1.0, -2.0, 0.5]]]), torch.tensor([[0.7]])
    v_xy, v_conic, v_rgb, v_op = gsplat_ref.rasterize_backward(1, 1, 16, 1, 1, gids, bins, xys, conics, colors, op,
                                                               bg, fT, fidx, v_out, v_oa, dtype=f64)
    assert rel(v_rgb[0], 0.99 * (float(fT) / 0.01) * v_out[0, 0].double()) < 1e-12
    leaves = [t.double().requires_grad_(True) for t in (xys, conics, colors, op)]
    for clamp in (0.99, 0.999):
        rgb, a_out, _ = rg.composite_masked(torch.tensor([[0.5, 0.5]], dtype=f64), *leaves, bg.double(), gids,
                                            torch.ones(1, 1, dtype=torch.bool), torch.zeros(1, dtype=torch.long),
                                            fidx.reshape(1), alpha_clamp=clamp)
        a = torch.autograd.grad((rgb * v_out[0].double()).sum() + (a_out * v_oa[0].double()).sum(), leaves)
        assert rel(a[2][0], clamp * v_out[0, 0].double()) < 1e-12
        assert float(a[0].abs().max()) == 0 and float(a[1].abs().max()) == 0 and float(a[3].abs().max()) == 0
    assert float(v_xy.abs().max()) > 1e-5 and float(v_conic.abs().max()) > 1e-3 and float(v_op.abs().max()) > 1e-2


def test_deviation_ewa_vjp_ignores_the_frustum_clamp():
    """Where the centre lies beyond 1.3 tan(fov) the forward builds J from the clamped tx/tz, ty/tz; the backward
    builds it from the unclamped ones.  v_cov2d (conic -> cov2d, no J involved) still is the gradient of the
    clamped forward; v_cov3d = T^T G T is not, on exactly the clamped rows."""
    c = rc.proj_case("n2000_160x120_bw16")
    fwd = rc.proj_forward(c)
    live = (fwd[2] > 0) & (fwd[4] >= 0.05)
    act = live & rc.clamp_active(c)
    free = live & ~rc.clamp_active(c)
    assert int(act.sum()) >= 50 and int(free.sum()) >= 200
    up = (c["v_xy"], c["v_depth"], c["v_conic"], torch.zeros(c["n"]))
    auto, out = rc.proj_autograd(c, up, frustum_lim=c["lim"])
    assert rel(fwd[3][act], out[2][act]) < 1e-4  # the clamped plain forward is the oracle's forward there
    r64 = gsplat_ref.project_gaussians_backward(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"],
                                                c["fx"], c["fy"], out[5], fwd[2], out[2], out[3], *up, dtype=f64,
                                                return_cov=True)
    for onm, a, x in zip(PROJ_OUT, auto, r64):
        assert rel(x[free], a[free]) < 1e-9, onm
    assert rel(r64[3][act], auto[3][act]) < 1e-9           # v_cov2d
    per_row = (r64[4][act] - auto[4][act]).abs().amax(1) / auto[4][act].abs().amax(1)
    assert float(per_row.min()) > 1e-2                    # v_cov3d: every clamped row deviates
    assert rel(r64[1][act], auto[1][act]) > 1e-3           # and v_scale with it


def test_deviation_v_quat_keeps_its_radial_part():
    """gsplat's v_quat is dL/d(q_hat) of R(q_hat) with q_hat = q / |q| treated as free; the gradient of the raw
    quaternion is its projection (I - q_hat q_hat^T) v / |q| -- the radial part is not removed by gsplat."""
    c = rc.proj_case("n2000_160x120_bw16")
    fwd = rc.proj_forward(c)
    live = (fwd[2] > 0) & ~rc.clamp_active(c) & (fwd[4] >= 0.05)
    up = (c["v_xy"], c["v_depth"], c["v_conic"], torch.zeros(c["n"]))
    auto, out = rc.proj_autograd(c, up, normalise_quats=True)
    r64 = gsplat_ref.project_gaussians_backward(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"],
                                                c["fx"], c["fy"], out[5], fwd[2], out[2], out[3], *up, dtype=f64)
    q = c["quats"].double()
    qn = q.norm(dim=-1, keepdim=True)
    qh = q / qn
    radial = (r64[2] * qh).sum(-1, keepdim=True)
    proj = (r64[2] - qh * radial) / qn
    for nm in ("ordinary", "qnorm_1e-3", "qnorm_1e3"):
        m = live & (c["feat"] == rc.PROJ_FEATURES.index(nm))
        assert int(m.sum()) >= 20
        assert rel(proj[m], auto[2][m]) < 1e-9, nm
        assert float((radial[m].abs() / r64[2][m].abs().amax(1, keepdim=True)).median()) > 1e-2, nm
        assert float((auto[2][m] * qh[m]).sum(-1).abs().max() / auto[2][m].abs().max()) < 1e-12  # autograd: none


def test_deviation_compensation_vjp_adds_1e_6():
    c = rc.proj_case("n255_17x33_bw8")
    fwd = rc.proj_forward(c)
    rows = _smooth_rows(c, fwd)
    z2, z, z3 = torch.zeros(c["n"], 2), torch.zeros(c["n"]), torch.zeros(c["n"], 3)
    up = (z2, z, z3, c["v_compensation"])
    auto, out = rc.proj_autograd(c, up)
    r64 = gsplat_ref.project_gaussians_backward(c["means"], c["scales"], c["glob_scale"], c["quats"], c["viewmat"],
                                                c["fx"], c["fy"], out[5], fwd[2], out[2], out[3], *up, dtype=f64,
                                                return_cov=True)
    comp = out[3][rows][:, None]
    for onm, a, x in zip(PROJ_OUT, auto, r64):
        assert rel(x[rows] * (comp + 1e-6) / comp, a[rows]) < 1e-9, onm
        assert rel(x[rows], a[rows]) > 1e-7, onm  # 1e-6 / compensation, compensation < 1


# ---- 3. sensitivity: wrong variants miss the GPU tests' bars --------------------------------------------------------
def _raster_bars(name, bw=16):
    r32, r64 = rc.raster_backward_ref(name, bw, f32), rc.raster_backward_ref(name, bw, f64)
    return r64, [BAR_FACTOR * rel(a, b) for a, b in zip(r32, r64)]


def _fails(variant, ref, bars):
    """Outputs on which the variant misses its bar."""
    return [i for i, (v, r, b) in enumerate(zip(variant, ref, bars)) if rel(v, r) > b]


RASTER_VARIANTS = {
    "backward_clamp_0999": ("saturated", None),
    "final_idx_excluded": ("partial_40x24", dict(include_final=False)),
    "background_dropped": ("partial_40x24", dict(with_background=False)),
    "v_out_alpha_dropped": ("partial_40x24", "no_alpha"),
    "batch_last_record_dropped": ("batch_257", "drop"),
}


@pytest.mark.parametrize("variant", list(RASTER_VARIANTS))
def test_wrong_rasterizer_variant_misses_the_bar(variant):
    name, how = RASTER_VARIANTS[variant]
    c = rc.raster_case(name)
    ref, bars = _raster_bars(name)
    assert max(bars) <= RASTER_CAP
    if how is None:
        wrong = rc.raster_backward_ref(name, 16, f64, alpha_clamp=0.999)
    elif how == "no_alpha":
        wrong = rc.raster_autograd(name, 16, v_out_alpha=torch.zeros_like(c["v_out_alpha"]))[:5]
    elif how == "drop":
        wrong = rc.raster_autograd(name, 16, drop_batch_last=True)[:5]
    else:
        wrong = rc.raster_autograd(name, 16, **how)[:5]
    if how is not None:  # the unmodified autograd passes the same bars (the variant is what fails, not the method)
        assert _fails(rc.raster_autograd(name, 16)[:5], ref, bars) == []
    bad = _fails(wrong, ref, bars)
    print(f"\n[{variant}] on {name}: misses on {[RASTER_OUT[i] for i in bad]}; "
          + ", ".join(f"{RASTER_OUT[i]} {rel(w, r):.1e} (bar {b:.1e})"
                      for i, (w, r, b) in enumerate(zip(wrong, ref, bars))))
    assert len(bad) >= 3, bad


def test_batch_drop_is_invisible_below_a_full_batch():
    """The same wrong variant on 255 records changes nothing: only the 256 / 257 / 512 / 513 cases can see it."""
    ref, bars = _raster_bars("batch_255")
    assert _fails(rc.raster_autograd("batch_255", 16, drop_batch_last=True)[:5], ref, bars) == []
    for name in ("batch_256", "batch_512", "batch_513"):
        ref, bars = _raster_bars(name)
        assert _fails(rc.raster_autograd(name, 16, drop_batch_last=True)[:5], ref, bars), name


PROJ_VARIANTS = ["compensation_dropped", "depth_dropped", "glob_scale_not_applied", "cov3d_offdiag_not_doubled",
                 "v_quat_divided_by_norm"]


@pytest.mark.parametrize("variant", PROJ_VARIANTS)
def test_wrong_projection_variant_misses_the_bar(variant):
    c = rc.proj_case("n2000_160x120_bw16")  # glob_scale 1.7
    fwd = rc.proj_forward(c)
    r32, r64 = rc.proj_backward_ref(c, fwd, f32), rc.proj_backward_ref(c, fwd, f64)
    up = [c["v_xy"], c["v_depth"], c["v_conic"], c["v_compensation"]]
    wrong = list(r64)
    if variant == "compensation_dropped":
        wrong = rc.proj_backward_ref(c, fwd, f64, (up[0], up[1], up[2], torch.zeros(c["n"])))
    elif variant == "depth_dropped":
        wrong = rc.proj_backward_ref(c, fwd, f64, (up[0], torch.zeros(c["n"]), up[2], up[3]))
    elif variant == "glob_scale_not_applied":
        wrong[1] = r64[1] / c["glob_scale"]
    elif variant == "cov3d_offdiag_not_doubled":
        wrong[4] = r64[4] * torch.tensor([1.0, 0.5, 0.5, 1.0, 0.5, 1.0], dtype=f64)
    else:
        wrong[2] = r64[2] / c["quats"].double().norm(dim=-1, keepdim=True)
    feature = "qnorm_1e3" if variant == "v_quat_divided_by_norm" else "ordinary"
    m = (fwd[2] > 0) & (c["feat"] == rc.PROJ_FEATURES.index(feature))
    bars = [BAR_FACTOR * rel(a[m], b[m]) for a, b in zip(r32, r64)]
    assert max(bars) <= 3e-5
    bad = _fails([w[m] for w in wrong], [r[m] for r in r64], bars)
    print(f"\n[{variant}] on {feature}: misses on {[PROJ_OUT[i] for i in bad]}")
    assert bad, variant
    if variant == "v_quat_divided_by_norm":  # invisible on unit quaternions, visible on both scaled groups
        m1 = (fwd[2] > 0) & (c["feat"] == rc.PROJ_FEATURES.index("ordinary"))
        assert rel(wrong[2][m1], r64[2][m1]) < 1e-6
        m3 = (fwd[2] > 0) & (c["feat"] == rc.PROJ_FEATURES.index("qnorm_1e-3"))
        assert rel(wrong[2][m3], r64[2][m3]) > 1.0


# ---- the cases themselves -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.RASTER_CASES)
def test_raster_case_is_clear_of_the_thresholds(name):
    assert rc.near_threshold_pairs(rc.raster_case(name)) == 0


def test_nonfinite_quaternions_are_culled_by_the_oracle():
    """Zero, denormal-norm and NaN quaternions: NaN radius -> the tile box's float -> int conversions give 0 (the
    GPU's conversion, gsplat_ref.cvt_i32) -> area 0 -> culled.  conics and cov3d are stored before the area test,
    as for every other culled Gaussian, and keep their NaNs."""
    c = rc.proj_case("n2000_160x120_bw16")
    xys, depths, radii, conics, comp, tiles, cov3d = rc.proj_forward(c)
    m = c["feat"] == rc.PROJ_FEATURES.index("bad_quat")
    assert int(m.sum()) >= 100
    for t in (xys, depths, radii, comp, tiles):
        assert float(t[m].double().abs().max()) == 0.0
    assert bool(torch.isnan(conics[m]).all()) and bool(torch.isnan(cov3d[m]).all())
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e9, -3e9, 2147483520.0, -7.9, 7.9])
    assert gsplat_ref.cvt_i32(x).tolist() == [0, 2147483647, -2147483648, 2147483647, -2147483648, 2147483520, -7, 7]
