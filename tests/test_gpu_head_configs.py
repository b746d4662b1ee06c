"""Every FeaturePredictor head wiring on the device (tests/heads_ref.py:CASES a-g): the fused heads kernel with its
per-column epilogue table against the fp64 restatement and against the unfused chain, the generalised batchify, the
training step's per-column epilogue and its derivative, the head gradients, and the public API end to end."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import heads_ref  # noqa: E402
from splatformer_amd import ptv3_ops as ops  # noqa: E402
from splatformer_amd import train as strain  # noqa: E402
from splatformer_amd import train_ops as tops  # noqa: E402
from splatformer_amd.feature_predictor import ALL_FEATURES, FeaturePredictor  # noqa: E402
from splatformer_amd.scenes import make_cameras, make_scene, to_device  # noqa: E402

pytestmark = pytest.mark.gpu
BK = dict(enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1))  # a shallow backbone: the heads are the subject
CB = 96


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _model(name, seed=0, **more):
    torch.manual_seed(seed)
    return FeaturePredictor(**heads_ref.product_kwargs(heads_ref.CASES[name], zeroinit=False, backbone_kwargs=BK,
                                                       **more))


def _head_sd(fp, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype) for k, v in fp.features_outputhead.state_dict().items()}


def _synthetic_rows(fp, n, seed):
    """A head input buffer H0 [n, ld] with rows of magnitude 2^-6 .. 2^6 in every column, and the input dict whose
    batchify gives it (attributes that are neither an input nor a residual base: zeros)."""
    ld, fcol, rcol = fp.row_layout()
    g = torch.Generator().manual_seed(seed)
    h0 = torch.randn(n, ld, generator=g) * torch.exp2(torch.randint(-6, 7, (n, 1), generator=g).float())
    used = CB + fp.gs_features_dim
    h0[:, used:(used + 3) // 4 * 4] = 0.0  # (the pad columns are zero in the product's buffer)
    gs = {}
    for f in ALL_FEATURES:
        c = fcol.get(f, rcol.get(f))
        w = fp.ch[f]
        v = h0[:, c:c + w].double() if c is not None else torch.zeros(n, w, dtype=torch.float64)
        gs[f] = v.reshape(n, -1, 3) if f == "features_rest" else v
    return h0, gs


def _predicted_ref(fp, case, h0, gs):
    """fp64: the heads' part of every output column, side by side in output order."""
    pred = heads_ref.predicted(_head_sd(fp), h0[:, :CB].double(), gs, input_features=fp.input_features,
                               output_features=fp.output_features,
                               output_features_type=case["output_features_type"],
                               input_feat_to_mlp=case["input_feat_to_mlp"], activations=case["activations"],
                               max_scale_normalized=case["max_scale_normalized"])
    return torch.cat([pred[f] for f in fp.output_features], 1)


def _predicted_part(fp, h0, y):
    """y minus what the epilogue adds behind the activation (residual base, clamp constant), in fp64."""
    act, res, add = fp.epilogue_table()
    out = y.double().clone()
    for c in range(len(act)):
        if res[c] >= 0:
            out[:, c] -= h0[:, res[c]].double()
        out[:, c] -= float(torch.tensor(add[c], dtype=torch.float32))
    return out


def _unfused(fp, h0d):
    w1, b1, mids, wl, bl, _ = fp._packed_heads()
    hh = ops.linear(h0d[:, :w1.shape[1]], w1, b1, act=ops.ACT_RELU)
    for wm, bm in mids:
        hh = ops.grouped_linear(hh, wm, bm, len(fp.output_features), act=ops.ACT_RELU)
    return ops.col_epilogue(ops.linear(hh, wl, bl), fp.col_table(h0d.device), h0d)


def run_case(name, n, device=None, unfused=True):
    """The fused kernel on synthetic rows against the fp64 restatement (2e-6) and the unfused chain (4e-6)."""
    device = device or torch.device("cuda:0")
    case = heads_ref.CASES[name]
    fp = _model(name, seed=ord(name))
    h0, gs = _synthetic_rows(fp, n, seed=ord(name) + n)
    ref = _predicted_ref(fp, case, h0, gs)
    fp = fp.to(device)
    out_dim = sum(fp.ch[f] for f in fp.output_features)
    assert ops.heads_fused_ok(len(fp.output_features), fp.nlayer, fp.width, fp.head_in, out_dim)
    st, pr, ocols, od = fp._fused_heads()
    h0d = h0.to(device)
    y = ops.heads_cols(h0d, fp.head_in, od, ocols, fp.epilogue_table(), st, pr).cpu()
    got = _predicted_part(fp, h0, y)
    err = rel_l2(got, ref)
    print(f"\n[heads {name} n={n}] kin {fp.head_in} out_dim {od}: fused vs fp64 {err:.3e}")
    assert err < 2e-6, err
    if case["output_features_type"] == "dc" and "scales" in fp.output_features and case["max_scale_normalized"] > 0:
        c0 = fp.columns()["scales"][0]
        k = torch.log(torch.tensor(case["max_scale_normalized"], dtype=torch.float32))
        sc = y[:, c0:c0 + 3]
        assert bool((sc <= k).all())
        z = heads_ref.mlp(_head_sd(fp), "scales", torch.cat([h0[:, :CB].double(), h0[:, CB:fp.head_in].double()], 1))
        below = z < -1e-3
        assert bool(below.any()) and bool((sc[below].view(torch.int32) == k.view(torch.int32)).all())
    if unfused:
        yu = _unfused(fp, h0d).cpu()
        e2 = rel_l2(got, _predicted_part(fp, h0, yu))
        print(f"[heads {name} n={n}] fused vs unfused {e2:.3e}")
        assert e2 < 4e-6, e2
    return err


@pytest.mark.parametrize("name,n", [(c, 300) for c in "abcdefg"] + [("a", 1), ("c", 1)])
def test_fused_heads_every_wiring(device, name, n):
    run_case(name, n, device)


def test_base_wiring_old_and_new_entry_give_the_same_bits(device):
    torch.manual_seed(3)
    fp = FeaturePredictor(zeroinit=False, backbone_kwargs=BK)
    h0, _ = _synthetic_rows(fp, 300, seed=77)
    fp = fp.to(device)
    st, pr, ocols, od = fp._fused_heads()
    h0d = h0.to(device)
    y_old = ops.heads(h0d, fp.head_in, CB, od, 3, ocols, st, pr)
    y_new = ops.heads_cols(h0d, fp.head_in, od, ocols, ops.heads_base_table(CB, 3, od), st, pr)
    assert fp.epilogue_table() == ops.heads_base_table(CB, 3, od)
    assert torch.equal(y_old.view(torch.int32), y_new.view(torch.int32))


def test_default_model_keeps_its_entry_points(device, monkeypatch):
    """refine_packed of the default model: sfx_gs_pack and sfx_heads, none of the column-table entries."""
    torch.manual_seed(4)
    fp = FeaturePredictor(backbone_kwargs=BK).to(device).eval()
    names = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    s = to_device(make_scene(1500, 1, seed=3), device)
    out = fp.refine_packed(s)
    fp.check_refine()
    assert out.shape == (1500, 23)
    assert "sfx_gs_pack" in names and "sfx_heads" in names
    assert not {"sfx_gs_pack_cols", "sfx_heads_cols", "sfx_col_epilogue_fwd"} & set(names)


def test_unsplit_head_groups_in_a_child_process(device):
    """All heads in one workgroup (what large scenes take) is reachable only through SFX_HEADS_SPLIT=0, read once
    per process: cases a and d once more in a fresh interpreter, against the same fp64 bar."""
    code = ("import sys; sys.path.insert(0, %r); import test_gpu_head_configs as t\n"
            "for c in 'ad':\n    t.run_case(c, 300, unfused=False)\nprint('UNSPLIT-OK')\n" % HERE)
    env = dict(os.environ, SFX_HEADS_SPLIT="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), env=env, capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-600:])
    assert r.returncode == 0 and "UNSPLIT-OK" in r.stdout, r.stderr[-2000:]


# ---- generalised batchify ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [300, 1])
@pytest.mark.parametrize("name", ["c", "g", "strided"])
def test_gs_pack_cols(device, name, n):
    case = heads_ref.CASES["c" if name == "strided" else name]
    fp = _model("c" if name == "strided" else name)
    deg = case["sh_degree"]
    s = make_scene(max(n, 2), max(deg, 1), seed=50 + n)  # (a one-point scene has no extent to normalise by)
    s = {k: v[:n].contiguous() for k, v in s.items()}
    sd = to_device(s, device)
    if name == "strided":  # an input (means) and a residual-only attribute (scales) as column slices of wider rows
        sd["means"] = torch.cat([torch.zeros(n, 2), s["means"], torch.ones(n, 3)], 1).to(device)[:, 2:5]
        sd["scales"] = torch.cat([torch.ones(n, 1), s["scales"], torch.zeros(n, 1)], 1).to(device)[:, 1:4]
        assert sd["means"].stride(0) == 8 and sd["scales"].stride(0) == 5
    h0, feat, grid, gmax = fp.to(device).pack_input(sd)
    ld, fcol, rcol = fp.row_layout()
    want = torch.cat([s[f].reshape(n, -1) for f in fp.input_features], 1)
    assert torch.equal(feat.cpu().view(torch.int32), want.contiguous().view(torch.int32))
    for f, c in rcol.items():
        src = s[f].reshape(n, -1).contiguous()
        assert torch.equal(h0[:, c:c + fp.ch[f]].cpu().contiguous().view(torch.int32), src.view(torch.int32))
    # every column that is neither stays zero
    mask = torch.ones(ld, dtype=torch.bool)
    mask[CB:CB + fp.gs_features_dim] = False
    for f, c in rcol.items():
        mask[c:c + fp.ch[f]] = False
    assert bool((h0.cpu()[:, mask] == 0).all())
    # grid_coord and its maximum: what sfx_gs_pack gives for the same means
    full = to_device(make_scene(n, 1, seed=9), device)
    full["means"] = sd["means"].contiguous()
    f2 = torch.zeros(n, 24, device=device)
    g2 = torch.empty(n, 3, device=device, dtype=torch.int32)
    m2 = torch.zeros(1, device=device, dtype=torch.int32)
    ops.gs_pack(full, f2[:, :23], 384.0, g2, m2)
    assert torch.equal(grid, g2) and torch.equal(gmax, m2)
    assert torch.equal(grid.cpu(), torch.floor(s["means"] * 384).int())


# ---- the training path's per-column epilogue ---------------------------------------------------------------------
def _col_ref(z, x, act, res, add, dy):
    z = z.clone().requires_grad_()
    cols = []
    for c in range(z.shape[1]):
        v = z[:, c]
        v = [v, torch.tanh(v), torch.sigmoid(v), -torch.relu(v)][act[c]]
        v = v + torch.tensor(add[c], dtype=torch.float32).to(z.dtype)
        if res[c] >= 0:
            v = x[:, res[c]] + v
        cols.append(v)
    y = torch.stack(cols, 1)
    (y * dy).sum().backward()
    return y.detach(), z.grad


@pytest.mark.parametrize("M", [1, 257])
@pytest.mark.parametrize("N", [1, 23, 59])
def test_col_epilogue_forward_backward(device, M, N):
    g = torch.Generator().manual_seed(M * 100 + N)
    z = torch.randn(M, N + 3, generator=g)[:, :N] * 3.0
    x = torch.randn(M, N + 5, generator=g) * 4.0
    dy = torch.randn(M, N, generator=g)
    act = [(c + 1 + M) % 4 for c in range(N)]
    res = [(c * 7) % (N + 5) if c % 3 != 1 else -1 for c in range(N)]
    add = [-4.6051702 if a == 3 else (0.25 if c % 5 == 4 else 0.0) for c, a in enumerate(act)]
    y64, dz64 = _col_ref(z.double(), x.double(), act, res, add, dy.double())
    y32, dz32 = _col_ref(z.clone(), x, act, res, add, dy)
    tab = ops.ColTable((act, res, add), device)
    zd = torch.zeros(M, N + 3, device=device)
    zd[:, :N] = z.to(device)
    zv = zd[:, :N]
    y = ops.col_epilogue(zv, tab, x.to(device))
    dz = tops.col_epilogue_bwd(dy.to(device), zv, tab)
    assert bool((zd[:, N:] == 0).all())
    for tag, got, r64, r32 in (("fwd", y, y64, y32), ("bwd", dz, dz64, dz32)):
        rn = r64.norm(dim=1).clamp_min(1e-30)
        e_hip = (got.cpu().double() - r64).norm(dim=1) / rn
        e_f32 = (r32.double() - r64).norm(dim=1) / rn
        print(f"\n[col epilogue {tag} M={M} N={N}] hip {float(e_hip.max()):.2e} fp32 {float(e_f32.max()):.2e}")
        assert bool((e_hip <= 2 * e_f32 + 1e-7).all()), (tag, float((e_hip - 2 * e_f32).max()))
    # in place: dz may be dy
    dy2 = dy.to(device).clone()
    assert torch.equal(tops.col_epilogue_bwd(dy2, zv, tab, out=dy2), dz)


# ---- head gradients ------------------------------------------------------------------------------------------------
def _train_once(fp, gs, d_packed, device, perms=None):
    for p in fp.parameters():
        p.grad = torch.zeros_like(p) if p.requires_grad else None
    # (no DropPath, and `perms` replays a run's shuffled serialization orders: two runs then agree)
    packed, tape = strain.refine_train(fp, gs, lambda name, n, p, device=None: None, perms=perms)
    x = tape["x"].detach().cpu().clone()
    saved = tape["o"].detach().cpu().clone()
    strain.refine_backward(fp, tape, d_packed.to(device))
    return packed.cpu(), x, saved


@pytest.mark.parametrize("name", ["a", "c", "d"])
def test_head_gradients_match_fp64_autograd(device, name):
    case = heads_ref.CASES[name]
    fp = _model(name, seed=11).to(device)
    strain.select_trainable(fp, ("features_outputhead",))
    s = make_scene(1500, case["sh_degree"], seed=60)
    n = s["means"].shape[0]
    gs = to_device(s, device)
    od = sum(fp.ch[f] for f in fp.output_features)
    d_packed = torch.randn(n, od, generator=torch.Generator().manual_seed(5))
    packed, x, saved = _train_once(fp, gs, d_packed, device)
    assert all(t.grad is None for t in gs.values())  # nothing flows to the inputs
    # fp64 autograd of the restatement, the backbone feature the tape holds taken as given
    sd = {k: v.requires_grad_() for k, v in _head_sd(fp).items()}
    gs64 = {k: v.double() for k, v in s.items()}
    pred = heads_ref.predicted(sd, x[:, :CB].double(), gs64, input_features=fp.input_features,
                               output_features=fp.output_features, output_features_type=case["output_features_type"],
                               input_feat_to_mlp=case["input_feat_to_mlp"], activations=case["activations"],
                               max_scale_normalized=case["max_scale_normalized"])
    if case["output_features_type"] == "dc" and case["max_scale_normalized"] > 0 and "scales" in pred:
        # -relu has no derivative at 0: where the fp64 pre-activation is within fp32 rounding of 0 the kernel's branch
        # (the sign of its stored pre-activation) is as right as the other and is taken as given; elsewhere the two
        # must agree
        c0, w = fp.columns()["scales"]
        y64 = torch.cat([x[:, :CB].double(), heads_ref.batchify(gs64, fp.input_features)[0]], 1)
        zs = heads_ref.mlp(sd, "scales", y64 if case["input_feat_to_mlp"] else y64[:, :CB])
        on_hip = saved[:, c0:c0 + w] > 0
        differ = (zs.detach() > 0) != on_hip
        worst_z = float(zs.detach()[differ].abs().max()) if bool(differ.any()) else 0.0
        print(f"\n[head grads {name}] clamp branches unlike fp64's: {int(differ.sum())} of {differ.numel()}, "
              f"largest |z| among them {worst_z:.2e}")
        assert worst_z < 1e-5
        pred["scales"] = -(zs * on_hip)
    ref = torch.cat([pred[f] for f in fp.output_features], 1)
    (ref * d_packed.double()).sum().backward()
    h0 = torch.zeros(n, fp.row_layout()[0])
    h0[:, :x.shape[1]] = x
    for f, c in fp.row_layout()[2].items():
        h0[:, c:c + fp.ch[f]] = s[f].reshape(n, -1)
    assert rel_l2(_predicted_part(fp, h0, packed), ref) < 1e-5  # (the forward the gradients belong to)
    errs = {k: rel_l2(p.grad.cpu(), sd[k].grad) for k, p in fp.features_outputhead.named_parameters()}
    print(f"\n[head grads {name}] " + " ".join(f"{k}={e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) < 1e-5, max(errs.items(), key=lambda t: t[1])
    assert all(p.grad is None for k, p in fp.named_parameters() if not k.startswith("features_outputhead."))
    if name == "c":  # the rows of d_packed reach only their own output columns' head
        c0, w = fp.columns()["scales"]
        d2 = d_packed.clone()
        d2[:, c0:c0 + w] = 0.0
        before = {k: p.grad.clone() for k, p in fp.features_outputhead.named_parameters()}
        _train_once(fp, gs, d2, device, perms=fp.backbone.backbone.last_perms)
        for k, p in fp.features_outputhead.named_parameters():
            if k.startswith("scales."):
                assert not bool(p.grad.any()), k
            else:
                assert rel_l2(p.grad, before[k]) < 1e-6, k


# ---- the public API, end to end ------------------------------------------------------------------------------------
def test_case_c_refines_renders_and_trains(device):
    from splatformer_amd.evaluate import evaluate_scenes
    case = heads_ref.CASES["c"]
    fp = _model("c", seed=21).to(device).eval()
    s = to_device(make_scene(1500, 1, seed=61), device)
    out = fp([s], [0])[0]
    fp.check_refine()
    assert list(out) == ["scales", "means", "features_dc", "features_rest", "opacities", "quats"]
    for k in ("features_dc", "features_rest", "opacities", "quats"):
        assert out[k] is s[k]
    assert out["scales"].shape == (1500, 3) and out["means"].shape == (1500, 3)
    # residual + sigmoid / tanh: the refined values stay within the activation's range of the input
    d_sc, d_mu = out["scales"] - s["scales"], out["means"] - s["means"]
    assert bool((d_sc >= -1e-5).all()) and bool((d_sc <= 1 + 1e-5).all()) and float(d_sc.max()) > 0
    assert bool((d_mu.abs() <= 1 + 1e-6).all()) and float(d_mu.abs().max()) > 0
    cams = to_device(make_cameras(64, 48, n_views=2), device)
    gt = torch.rand(2, 48, 64, 3, device=device)
    m = evaluate_scenes(fp, [out], [cams], lambda i: gt, device, evaluate_input=True)
    assert m["psnr"] == m["psnr"] and m["ssim"] == m["ssim"]
    for mode in strain.RENDER_MODES:
        tr = strain.Trainer(fp, finetune_list=("features_outputhead",), render=mode,
                            generator=torch.Generator(device=device).manual_seed(0))
        assert tr.params and len(tr.params) == 2 * 2 * fp.nlayer
        before = [p.detach().clone() for p in tr.params]
        loss = tr.step([s], [cams], [list(gt.unbind(0))])
        assert loss == loss and 0 < loss < float("inf"), (mode, loss)
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, tr.params)), mode
    assert case["output_features"] == ["scales", "means"]
