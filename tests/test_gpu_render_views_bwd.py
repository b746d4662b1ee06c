"""Batched multi-view differentiable render (gs_render.rasterize_gaussians_to_multiimgs_batched) and its two HIP
backward entries, against the eval path (forward, bit for bit), the gsplat v0.1.11 CPU oracle (gradients) and the
existing per-view autograd path (the yardstick for the gradient error).

Common scene: make_scene(1500, deg, seed=31) with features_dc * 2.5 (pixels above 1 before the image clamp, SH
colours clamped at 0), 100 x 84 images (both sides ragged against the 16-pixel tile), background (0.3, 0.2, 0.1),
the two make_cameras views and an "away" camera that sees nothing (gsplat's empty-list branch).

Oracle gradient chain (per view, summed): gsplat_ref.rasterize_backward -> project_gaussians_backward and
spherical_harmonics_bwd -> torch autograd through the glue ops of render_ref.glue_args (exp, q / |q|, sigmoid,
clamp(rgb + 0.5, min=0), the degree-0 sigmoid colour) on float32 leaves; view directions carry no gradient.
"""
import functools

import pytest
import torch

from oracle import gsplat_ref, render_ref
from splatformer_amd import _lib, gs_render
from splatformer_amd import train as strain
from splatformer_amd.scenes import look_at_c2w, make_cameras, make_scene, to_device

pytestmark = pytest.mark.gpu

W, H, N = 100, 84, 1500
ATTRS = ["means", "scales", "quats", "opacities", "features_dc", "features_rest"]


def _away(cams):
    """A camera at view 0's position looking away from the scene centre: no Gaussian in front of it."""
    eye = cams["camera_to_worlds"][0][:3, 3].double()
    centre = torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64)
    return look_at_c2w(eye, 2 * eye - centre).float()


@functools.lru_cache(maxsize=None)
def _common(deg):
    s = make_scene(N, deg, seed=31)
    s["features_dc"] = s["features_dc"] * 2.5
    cams = make_cameras(W, H, n_views=2)
    cams["background_color"] = torch.tensor([0.3, 0.2, 0.1])
    return s, cams, _away(cams)


def _with_views(cams, c2ws):
    out = dict(cams)
    out["camera_to_worlds"] = torch.stack(list(c2ws))
    return out


def _leaves(s, device):
    return {k: v.to(device).clone().requires_grad_(True) for k, v in s.items()}


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


# ---- the oracle chain ------------------------------------------------------------------------------------------
def _view_oracle(s, c2w, cams):
    """Canonical glue + projection of one view on the CPU oracle."""
    a = render_ref.glue_args(s, c2w, canonical=True)
    proj = gsplat_ref.project_gaussians(a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"],
                                        cams["cx"], cams["cy"], H, W, 16)
    return a, proj


def _chain(s, views, cams, grads):
    """views: [(glue args, projection)] per view; grads: per view (v_xy [n,2], v_conic [n,3], v_rgb [n,3],
    v_opacity [n]) with respect to the projected Gaussians -> gradients of the raw attributes."""
    n = s["means"].shape[0]
    deg = views[0][0]["sh_degree"]
    nb = (deg + 1) ** 2
    Vm, Vs, Vq = torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n, 4)
    Vop, Vcol = torch.zeros(n, 1), torch.zeros(n, nb, 3)
    for (a, proj), (v_xy, v_conic, v_rgb, v_op) in zip(views, grads):
        xys, depths, radii, conics, comp, tiles, cov3d = proj
        live = (radii > 0)[:, None].float()  # a Gaussian dead in a view gets nothing from that view
        vm, vs, vq = gsplat_ref.project_gaussians_backward(
            a["means"], a["scales"], 1.0, a["quats"], a["viewmat"], cams["fx"], cams["fy"], cov3d, radii, conics,
            comp, v_xy, torch.zeros(n), v_conic, torch.zeros(n))
        Vm, Vs, Vq = Vm + vm, Vs + vs, Vq + vq
        Vop = Vop + v_op.reshape(n, 1) * live
        if deg == 0:
            Vcol[:, 0] += v_rgb * live
        else:  # clamp(rgb + 0.5, min=0) by torch autograd, then the oracle's SH backward
            pre = gsplat_ref.spherical_harmonics(deg, a["viewdirs"], a["colors"]).requires_grad_(True)
            torch.clamp(pre + 0.5, min=0.0).backward(v_rgb * live)
            Vcol += gsplat_ref.spherical_harmonics_bwd(deg, a["viewdirs"], pre.grad, nb)
    lv = {k: v.clone().requires_grad_(True) for k, v in s.items()}
    q = lv["quats"] / torch.norm(lv["quats"], dim=-1, keepdim=True)
    q = torch.where(torch.isnan(q).any(-1, keepdim=True), torch.tensor([0, 0, 0, 1.0]), q)
    total = (lv["means"] * Vm).sum() + (torch.exp(lv["scales"]) * Vs).sum() + (q * Vq).sum() \
        + (torch.sigmoid(lv["opacities"]) * Vop).sum()
    if deg == 0:
        total = total + (torch.sigmoid(lv["features_dc"]) * Vcol[:, 0]).sum()
    else:
        colors = torch.cat([lv["features_dc"].unsqueeze(1), lv["features_rest"]], 1)
        total = total + (colors * Vcol).sum()
    total.backward()
    return {k: v.grad for k, v in lv.items()}


@functools.lru_cache(maxsize=None)
def _whole_reference(deg):
    """Test 3's reference: oracle forward (canonical glue) of views 0, 1 and the away camera, the loss weights,
    rasterize_backward per view and the chain.  Computed once per degree."""
    s, cams, away = _common(deg)
    c2ws = [cams["camera_to_worlds"][0], cams["camera_to_worlds"][1], away]
    g = torch.Generator().manual_seed(7 + deg)
    ws = [torch.randn(H, W, 3, generator=g) for _ in c2ws]
    us = [torch.randn(H, W, 1, generator=g) for _ in c2ws]
    bg = cams["background_color"]
    tx, ty = (W + 15) // 16, (H + 15) // 16
    views, grads = [], []
    n = s["means"].shape[0]
    for c2w, w, u in zip(c2ws, ws, us):
        a, proj = _view_oracle(s, c2w, cams)
        xys, depths, radii, conics, comp, tiles, cov3d = proj
        views.append((a, proj))
        if int(tiles.sum()) < 1:  # gsplat's empty-list branch: a constant image, no gradient
            grads.append((torch.zeros(n, 2), torch.zeros(n, 3), torch.zeros(n, 3), torch.zeros(n)))
            continue
        _, gids, bins = gsplat_ref.bin_and_sort_gaussians(xys, depths, radii, tiles, tx, ty, 16)
        img, fT, fidx = gsplat_ref.rasterize_forward(tx, ty, 16, H, W, gids, bins, xys, conics, a["rgbs"],
                                                     a["opacities"], bg)
        v_out = w * (img <= 1.0).float()  # torch.clamp(max=1) passes gradient where the input is <= 1
        v_xy, v_conic, v_rgb, v_op = gsplat_ref.rasterize_backward(
            tx, ty, 16, H, W, gids, bins, xys, conics, a["rgbs"], a["opacities"], bg, fT, fidx, v_out, u[..., 0])
        grads.append((v_xy, v_conic, v_rgb, v_op.reshape(-1)))
    return c2ws, ws, us, _chain(s, views, cams, grads)


def _loss(rgbs, alphas, ws, us, device):
    return sum((r * w.to(device)).sum() + (a * u.to(device)).sum() for r, a, w, u in zip(rgbs, alphas, ws, us))


# ---- 1. forward identity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 1, 3])
def test_forward_equals_eval_path(device, deg):
    s, cams, away = _common(deg)
    cd = to_device(_with_views(cams, [cams["camera_to_worlds"][0], cams["camera_to_worlds"][1], away]), device)
    sd = to_device(s, device)
    with torch.no_grad():
        r_ref, a_ref = gs_render.rasterize_gaussians_to_multiimgs(sd, cd)
    rgbs, alphas = gs_render.rasterize_gaussians_to_multiimgs_batched(_leaves(s, device), cd)
    assert len(rgbs) == 3 and rgbs[0].requires_grad
    for v in range(3):
        assert rgbs[v].shape == (H, W, 3) and alphas[v].shape == (H, W, 1)
        assert torch.equal(rgbs[v], r_ref[v]), v
        assert torch.equal(alphas[v], a_ref[v]), v
    assert float(alphas[2].detach().min()) == 1.0  # the away view: gsplat's empty-list quirk


# ---- 2. the prep backward alone ----------------------------------------------------------------------------------
def _prep_bwd(sd, cams_dev, radii, conics, grads, nb):
    """sfx_render_prep_project_views_bwd on separate (contiguous) attribute tensors -> dict of gradients."""
    n, V = sd["means"].shape[0], radii.shape[0]
    out = {k: torch.full_like(sd[k].reshape(n, -1), float("nan")) for k in ATTRS if k in sd}  # no zero-fill needed
    io = []
    for d in (sd, out):
        for k in ATTRS:
            t = d.get(k)
            io.append([None, 0] if t is None else [t.data_ptr(), t.reshape(n, -1).shape[1]])
    c2ws = cams_dev["camera_to_worlds"].contiguous()
    _lib.call("sfx_render_prep_project_views_bwd", n, V, nb, *sum(io[:6], []), c2ws.data_ptr(), cams_dev["fx"],
              cams_dev["fy"], radii.data_ptr(), conics.data_ptr(), *[g.data_ptr() for g in grads], *sum(io[6:], []),
              _lib.stream())
    return {k: v.reshape(sd[k].shape) for k, v in out.items()}


@pytest.mark.parametrize("deg", [0, 1, 3])
def test_prep_backward_matches_oracle_and_is_deterministic(device, deg):
    """V = 3: two close-ups of the common scene (the two cameras' directions at radius 0.6: 1078 and 1082 of the 1500
    Gaussians project, 226 in exactly one of them, 307 in neither) and the away camera -- from the full-size views
    every Gaussian is live, which would leave the per-view and the dead-everywhere masks untested."""
    s, cams, away = _common(deg)
    near = make_cameras(W, H, n_views=2, radius=0.6)["camera_to_worlds"]
    c2ws = [near[0], near[1], away]
    n, V, nb = N, 3, (deg + 1) ** 2
    g = torch.Generator().manual_seed(11 + deg)
    v_xys, v_conics = torch.randn(V, n, 2, generator=g), torch.randn(V, n, 3, generator=g) * 1e-3
    v_rgbs, v_ops = torch.randn(V, n, 3, generator=g), torch.randn(V, n, generator=g)
    views = [_view_oracle(s, c2w, cams) for c2w in c2ws]
    ref = _chain(s, views, cams, [(v_xys[v], v_conics[v], v_rgbs[v], v_ops[v]) for v in range(V)])
    # the forward's per-view radii / conics from the batched eval pass itself
    sd = {k: v.to(device).contiguous() for k, v in s.items()}
    cd = to_device(_with_views(cams, c2ws), device)
    with torch.no_grad():
        _, _, meta = gs_render.render_views_meta(sd, cd)
    radii, conics = meta["radii"].contiguous(), meta["conics"].contiguous()
    for v in range(V):
        assert torch.equal(radii[v].cpu(), views[v][1][2]), v  # the projection is bit-exact to the oracle
    dev_grads = [t.to(device).contiguous() for t in (v_xys, v_conics, v_rgbs, v_ops)]
    got = _prep_bwd(sd, cd, radii, conics, dev_grads, nb)
    again = _prep_bwd(sd, cd, radii, conics, dev_grads, nb)
    live = (radii > 0).any(0).cpu()
    assert int(live.sum()) > 1000 and int((~live).sum()) > 100 and int(((radii > 0).sum(0) == 1).sum()) > 100
    for k, exp in ref.items():
        o = got[k].cpu()
        assert torch.equal(got[k], again[k]), f"{k}: two calls differ"
        assert not torch.isnan(o).any(), f"{k}: an element was not stored"
        scale = exp[live].abs().max().clamp_min(1e-6)
        err = float((o - exp)[live].abs().max() / scale)
        print(f"\n[prep bwd deg {deg}] {k}: max|d| / max|ref| = {err:.2e}")
        assert err < 1e-4, f"{k}: rel err {err}"
        assert float(o[~live].abs().max()) == 0.0, f"{k}: a Gaussian dead in every view has a gradient"


# ---- 3. the whole op ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [1, 3])
def test_whole_op_matches_oracle_like_per_view_path(device, deg):
    """e_new, e_old: rel-L2 error per attribute of the batched op / of the existing per-view autograd path against
    the oracle chain.  Measured on MI355X: see DESIGN.md (batched training render)."""
    s, cams, _ = _common(deg)
    c2ws, ws, us, ref = _whole_reference(deg)
    cd = to_device(_with_views(cams, c2ws), device)
    with torch.no_grad():
        _, _, meta = gs_render.render_views_meta(to_device(s, device), cd)
    bins = meta["tile_bins"]
    longest = (bins[..., 1] - bins[..., 0]).amax(1)
    assert int(longest[0]) > 256 and int(longest[1]) > 256  # the 256-record batch loop runs more than once
    res = {}
    for name, fn in (("new", gs_render.rasterize_gaussians_to_multiimgs_batched),
                     ("old", gs_render.rasterize_gaussians_to_multiimgs)):
        p = _leaves(s, device)
        rgbs, alphas = fn(p, cd)
        _loss(rgbs, alphas, ws, us, device).backward()
        res[name] = {k: v.grad.cpu() for k, v in p.items()}
    for k, exp in ref.items():
        assert float(exp.norm()) > 0, k
        e_new, e_old = rel_l2(res["new"][k], exp), rel_l2(res["old"][k], exp)
        print(f"\n[whole op deg {deg}] {k}: e_new {e_new:.2e}, e_old {e_old:.2e}")
        assert e_new <= 2.0 * e_old + 1e-5, f"{k}: batched {e_new:.2e} vs per-view {e_old:.2e} (to the oracle)"


# ---- 4. view sum -------------------------------------------------------------------------------------------------
def test_identical_views_sum(device):
    s, cams, _ = _common(1)
    c2w = cams["camera_to_worlds"][0]
    g = torch.Generator().manual_seed(3)
    w, u = torch.randn(H, W, 3, generator=g), torch.randn(H, W, 1, generator=g)
    grads = {}
    for V in (1, 3):
        cd = to_device(_with_views(cams, [c2w] * V), device)
        p = _leaves(s, device)
        rgbs, alphas = gs_render.rasterize_gaussians_to_multiimgs_batched(p, cd)
        for v in range(1, V):
            assert torch.equal(rgbs[v], rgbs[0]) and torch.equal(alphas[v], alphas[0]), v
        _loss(rgbs, alphas, [w] * V, [u] * V, device).backward()
        grads[V] = {k: t.grad for k, t in p.items()}
    for k, g1 in grads[1].items():
        assert float(g1.norm()) > 0, k
        err = rel_l2(grads[3][k], 3.0 * g1)
        assert err <= 1e-5, f"{k}: rel {err:.3e}"  # differences in atomic order only


# ---- 5. packed versus dict entry ----------------------------------------------------------------------------------
def test_packed_entry_equals_dict_entry(device):
    s, cams, away = _common(1)
    cd = to_device(_with_views(cams, [cams["camera_to_worlds"][0], cams["camera_to_worlds"][1], away]), device)
    g = torch.Generator().manual_seed(4)
    ws = [torch.randn(H, W, 3, generator=g) for _ in range(3)]
    us = [torch.randn(H, W, 1, generator=g) for _ in range(3)]
    p = _leaves(s, device)
    rgbs, alphas = gs_render.rasterize_gaussians_to_multiimgs_batched(p, cd)
    _loss(rgbs, alphas, ws, us, device).backward()
    # one record with the attributes in another order and unused columns in front, between and behind
    cols, parts, c = {}, [], 2
    parts.append(torch.full((N, 2), 7.0))
    for k in ["features_rest", "quats", "means", "PAD", "opacities", "features_dc", "scales"]:
        t = torch.full((N, 3), -3.0) if k == "PAD" else s[k].reshape(N, -1)
        if k != "PAD":
            cols[k] = (c, t.shape[1])
        parts.append(t)
        c += t.shape[1]
    parts.append(torch.full((N, 1), 9.0))
    leaf = torch.cat(parts, 1).to(device).requires_grad_(True)
    r2, a2 = gs_render.rasterize_packed_to_multiimgs_batched(leaf, cols, cd)
    for v in range(3):
        assert torch.equal(r2[v], rgbs[v]) and torch.equal(a2[v], alphas[v]), v
    _loss(r2, a2, ws, us, device).backward()
    used = torch.zeros(leaf.shape[1], dtype=torch.bool)
    for k, (c0, w) in cols.items():
        used[c0:c0 + w] = True
        err = rel_l2(leaf.grad[:, c0:c0 + w].cpu(), p[k].grad.reshape(N, -1).cpu())
        assert err <= 1e-5, f"{k}: rel {err:.3e}"
    assert int((~used).sum()) == 6
    assert float(leaf.grad[:, ~used.to(device)].abs().max()) == 0.0
    # attributes that are already columns of one record (FeaturePredictor.unpack's views) are used in place
    leaf2 = leaf.detach().clone().requires_grad_(True)
    views = {k: leaf2[:, c0:c0 + w] for k, (c0, w) in cols.items()}
    views["features_rest"] = views["features_rest"].unflatten(1, (-1, 3))
    r3, a3 = gs_render.rasterize_gaussians_to_multiimgs_batched(views, cd)
    _loss(r3, a3, ws, us, device).backward()
    assert rel_l2(leaf2.grad.cpu(), leaf.grad.cpu()) <= 1e-5


# ---- 6. empty input ----------------------------------------------------------------------------------------------
def test_all_views_empty(device):
    s, cams, away = _common(1)
    cd = to_device(_with_views(cams, [away, away]), device)
    p = _leaves(s, device)
    rgbs, alphas = gs_render.rasterize_gaussians_to_multiimgs_batched(p, cd)
    bg = cams["background_color"].to(device)
    for v in range(2):
        assert torch.equal(rgbs[v], bg.expand(H, W, 3)), v
        assert float(alphas[v].detach().min()) == 1.0 and float(alphas[v].detach().max()) == 1.0
    sum(r.sum() + a.sum() for r, a in zip(rgbs, alphas)).backward()
    torch.cuda.synchronize()
    for k, t in p.items():
        assert t.grad is not None and float(t.grad.abs().max()) == 0.0, k


# ---- 7. trainer plumbing -----------------------------------------------------------------------------------------
class _FixedMasks:
    """DropPath masks from a seeded CPU generator: the same sequence for every trainer built with the same seed."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, name, n, p, device=None):
        if p <= 0.0:
            return None
        keep = 1.0 - p
        return ((torch.rand(n, generator=self.g) < keep).float() / keep).to(device)


def test_trainer_batched_render(device, monkeypatch):
    from splatformer_amd.feature_predictor import FeaturePredictor
    torch.manual_seed(0)
    sd0 = FeaturePredictor(sh_degree=1, zeroinit=False).state_dict()
    s = to_device(make_scene(3000, 1, seed=2), device)
    cams = to_device(make_cameras(96, 80, n_views=2), device)
    gt = [torch.rand(80, 96, 3, generator=torch.Generator().manual_seed(v)).to(device) for v in range(2)]
    perms = [[0, 1, 2, 3]] * 5
    calls = {"batched": 0, "per_view": 0}

    def spy(key, fn):
        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(strain, "rasterize_packed_to_multiimgs_batched",
                        spy("batched", strain.rasterize_packed_to_multiimgs_batched))
    monkeypatch.setattr(strain, "rasterize_gaussians_to_multiimgs",
                        spy("per_view", strain.rasterize_gaussians_to_multiimgs))
    losses = {}
    for mode in ("batched", "per_view"):
        model = FeaturePredictor(sh_degree=1, zeroinit=False)
        model.load_state_dict(sd0)
        model = model.to(device)
        tr = strain.Trainer(model, lr=1e-3, render=mode)
        assert tr.render == mode
        before = [p.detach().clone() for p in tr.params]
        calls.update(batched=0, per_view=0)
        losses[mode] = tr.step([s], [cams], [gt], masks=_FixedMasks(5), perms=perms)
        assert calls == ({"batched": 1, "per_view": 0} if mode == "batched" else {"batched": 0, "per_view": 1})
        assert losses[mode] == losses[mode] and 0 < losses[mode] < float("inf")
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, tr.params))
        assert float(tr.flat_grad.abs().max()) == 0.0  # zeroed after the optimiser step
    # both forwards are within the project's 2e-4 image bar of the oracle and the loss is a mean of absolute image
    # differences: 4e-4
    assert abs(losses["batched"] - losses["per_view"]) <= 4e-4, losses
    with pytest.raises(ValueError, match="render"):
        strain.Trainer(model, render="tiled")
