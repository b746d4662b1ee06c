"""Training every refiner parameter: the new kernels against fp64, the whole refiner's parameter gradients against
torch autograd of the CPU oracle, a parameter subset, and the Trainer end to end.

Bars: the kernels `rel_l2 < 1e-5` to fp64 (the bar of test_linear_wgrad); the refiner's gradients, per module
(weight and bias concatenated -- several biases have an exactly zero true gradient: a Linear bias in front of a
train-mode BatchNorm, the key bias under the softmax; both sides hold rounding noise there), no further from the fp64
oracle than 2x the fp32 oracle in aggregate and 4x per module (+1e-5), the bar test_gpu_train applies to qkv.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ptv3_ref
from splatformer_amd import ptv3_ops as ops
from splatformer_amd import ptv3_train as pt
from splatformer_amd import train as strain
from splatformer_amd import train_ops as tops
from splatformer_amd.scenes import make_cameras, make_scene, to_device
from test_gpu_ptv3 import _model, rel_l2
from test_gpu_train import FEATS, RecordingMasks

pytestmark = pytest.mark.gpu

NEW_ENTRIES = {"sfx_subm_conv_wgrad", "sfx_layernorm_wgrad", "sfx_linear_wgrad_rs"}


# ---- 1. sfx_subm_conv_wgrad ---------------------------------------------------------------------------------
def _conv_case(n, cin, cout, dup, res):
    g = torch.Generator().manual_seed(1000 * n + cin + cout)
    grid = torch.randint(0, res, (n, 3), generator=g).int()
    if dup:  # duplicate voxels: the centre offset of a later copy maps to the lowest point index
        grid[n // 2:n // 2 + 200] = grid[:200]
    nbr = ptv3_ref.subm_neighbors(grid, torch.zeros(n, dtype=torch.int32))
    dy = torch.randn(n, cout, generator=g)
    x = torch.randn(n, cin, generator=g)
    return grid, nbr, dy, x


def _conv_wgrad_ref(nbr, dy, x, rnd=lambda t: t):
    """fp64, per offset: dY[out]^T X[in] over the (in, out) pairs that nbr lists."""
    n, cout = dy.shape
    dw = torch.zeros(cout, 27, x.shape[1], dtype=torch.float64)
    dyd, xd = rnd(dy).double(), rnd(x).double()
    for k in range(27):
        out = torch.nonzero(nbr[:, k] >= 0)[:, 0]
        dw[:, k] = dyd[out].T @ xd[nbr[out, k].long()]
    return dw.reshape(cout, -1), dy.double().sum(0)


@pytest.mark.parametrize("n,cin,cout,dup,res,nonzero", [
    (1, 64, 64, False, 4, False),
    (1, 512, 512, False, 4, False),
    (300, 64, 64, False, 7, False),
    (300, 96, 96, False, 7, True),      # accumulates into a non-zero dW / db
    (300, 512, 512, False, 7, False),   # 4 x 4 output tiles
    (300, 64, 96, False, 7, False),     # Cin != Cout: tile edges in both directions
    (5000, 64, 64, True, 20, False),    # duplicate voxels, several reduction splits per offset
    (5000, 96, 96, True, 20, False),
])
def test_subm_conv_wgrad(device, n, cin, cout, dup, res, nonzero):
    grid, nbr, dy, x = _conv_case(n, cin, cout, dup, res)
    if dup:
        assert int((nbr[:, 13] != torch.arange(n)).sum()) >= 200  # the centre pairs in != out there
    dw_ref, db_ref = _conv_wgrad_ref(nbr, dy, x)
    g = torch.Generator().manual_seed(7)
    dw0 = torch.randn(cout, 27 * cin, generator=g) if nonzero else torch.zeros(cout, 27 * cin)
    db0 = torch.randn(cout, generator=g) if nonzero else torch.zeros(cout)
    smap = ops.subm_neighbors(grid.to(device), None)
    dw, db = dw0.to(device), db0.to(device)
    tops.subm_conv_wgrad(dy.to(device), x.to(device), smap, dw, db)
    e_w, e_b = rel_l2(dw.cpu(), dw0 + dw_ref), rel_l2(db.cpu(), db0 + db_ref)
    print(f"\n[subm_conv_wgrad n={n} {cin}->{cout}] dW {e_w:.2e} db {e_b:.2e}")
    assert e_w < 1e-5
    assert e_b < 1e-5


@pytest.mark.parametrize("n,cin,cout,res", [(5000, 64, 64, 20), (300, 96, 96, 7)])
def test_subm_conv_wgrad_reference_precision(device, n, cin, cout, res):
    """Under ops.precision("amp") (three bf16 term products) the error sits strictly between the fp32-accurate
    mode's and that of fp16-rounded operands, as for the dense kernel."""
    grid, nbr, dy, x = _conv_case(n, cin, cout, True if n >= 1000 else False, res)
    exact, _ = _conv_wgrad_ref(nbr, dy, x)
    e16 = rel_l2(_conv_wgrad_ref(nbr, dy, x, rnd=lambda t: t.half())[0], exact)
    smap = ops.subm_neighbors(grid.to(device), None)
    dw = torch.zeros(cout, 27 * cin, device=device)
    with ops.precision("amp"):
        tops.subm_conv_wgrad(dy.to(device), x.to(device), smap, dw, None)
    e_amp = rel_l2(dw.cpu(), exact)
    dw.zero_()
    tops.subm_conv_wgrad(dy.to(device), x.to(device), smap, dw, None)
    e_32 = rel_l2(dw.cpu(), exact)
    print(f"\n[subm_conv_wgrad precision n={n} C={cin}] fp32-accurate {e_32:.2e} amp {e_amp:.2e} fp16 {e16:.2e}")
    assert e_32 < e_amp < e16, (e_32, e_amp, e16)


# ---- 2. sfx_layernorm_wgrad and the row-scaled weight gradient ---------------------------------------------------
@pytest.mark.parametrize("C", [64, 96, 512])
@pytest.mark.parametrize("M", [1, 77, 4000])
def test_layernorm_wgrad(device, M, C):
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g) * 2.0 + 0.5
    dy = torch.randn(M, C, generator=g)
    gamma = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x.double(), (C,), gamma, beta, 1e-5).backward(dy.double())
    xd, dyd = x.to(device), dy.to(device)
    runs = []
    for _ in range(2):
        dg = torch.full((C,), 7.0, device=device)
        db = torch.full((C,), 7.0, device=device)
        tops.layernorm_wgrad(xd, dyd, 1e-5, dg, db, accumulate=False)
        runs.append((dg.cpu(), db.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])  # fixed reduction order
    e_g, e_b = rel_l2(runs[0][0], gamma.grad), rel_l2(runs[0][1], beta.grad)
    print(f"\n[layernorm_wgrad M={M} C={C}] dgamma {e_g:.2e} dbeta {e_b:.2e}")
    assert e_g < 1e-5
    assert e_b < 1e-5
    g0 = torch.randn(C, generator=g)
    dg, db = g0.to(device), g0.to(device).clone()
    tops.layernorm_wgrad(xd, dyd, 1e-5, dg, db)  # accumulating, as the backward uses it
    assert rel_l2(dg.cpu(), g0.double() + gamma.grad) < 1e-5
    assert rel_l2(db.cpu(), g0.double() + beta.grad) < 1e-5


@pytest.mark.parametrize("C", [64, 96, 512])
@pytest.mark.parametrize("M", [1, 77, 4000])
def test_linear_wgrad_rowscale(device, M, C):
    """dW += (rowscale o dY)^T X, db += sum rowscale * dY against autograd of rowscale * Linear(x) in fp64."""
    g = torch.Generator().manual_seed(3 * M + C)
    N, K = C, C
    x = torch.randn(M, K, generator=g)
    dy = torch.randn(M, N, generator=g)
    keep = 0.7
    rs = (torch.rand(M, generator=g) < keep).float() / keep  # DropPath mask: zeros in it
    if M == 1:
        rs[:] = 1.0 / keep  # (a single dropped row has a zero gradient: nothing to compare)
    else:
        rs[0] = 0.0
    w = torch.randn(N, K, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(N, generator=g, dtype=torch.float64, requires_grad=True)
    (rs.double()[:, None] * F.linear(x.double(), w, b)).backward(dy.double())
    dw0, db0 = torch.randn(N, K, generator=g), torch.randn(N, generator=g)
    dw, db = dw0.to(device), db0.to(device)
    tops.linear_wgrad_rs(dy.to(device), x.to(device), rs.to(device), dw, db)
    e_w, e_b = rel_l2(dw.cpu(), dw0.double() + w.grad), rel_l2(db.cpu(), db0.double() + b.grad)
    print(f"\n[linear_wgrad_rs M={M} C={C}] dW {e_w:.2e} db {e_b:.2e}")
    assert e_w < 1e-5
    assert e_b < 1e-5
    # a null rowscale is sfx_linear_wgrad
    dw1, dw2 = torch.zeros(N, K, device=device), torch.zeros(N, K, device=device)
    tops.linear_wgrad_rs(dy.to(device), x.to(device), None, dw1, None)
    tops.linear_wgrad(dy.to(device), x.to(device), dw2, None)
    assert rel_l2(dw1, dw2) < 1e-6


# ---- 3 / 4. whole refiner -----------------------------------------------------------------------------------
BK = dict(enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1))


class ReplayMasks:
    def __init__(self, rec):
        self.masks = rec.masks

    def __call__(self, name, n, p, device=None):
        return None if p <= 0.0 else self.masks[name].to(device)


class LaunchLog:
    """Records the libsfx entry points the training ops call."""

    def __init__(self, monkeypatch):
        self.names = []
        for mod in (ops, tops):
            real = mod.call
            monkeypatch.setattr(mod, "call", lambda name, *a, _r=real: (self.names.append(name), _r(name, *a))[1])


def _fresh(r, device):
    """The fixture's model as it was before its forward (same weights and running statistics)."""
    model = _model(21, **BK)
    model.load_state_dict(r["sd"])
    return model.to(device)


def _run_hip(model, gs, masks, perms, d_packed, device):
    for p in model.parameters():
        p.grad = torch.zeros_like(p) if p.requires_grad else None
    packed, tape = strain.refine_train(model, gs, masks, perms=perms)
    strain.refine_backward(model, tape, d_packed.to(device))
    return packed, tape


@pytest.fixture(scope="module")
def all_run(device):
    """One all-parameter HIP forward + backward of the reduced-depth refiner, shared by the tests below."""
    model = _model(21, **BK)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model = model.to(device)
    strain.select_trainable(model, None)
    s = make_scene(2000, 1, seed=2001, unique_voxels=True)
    n = s["means"].shape[0]
    gs = to_device(s, device)
    masks = RecordingMasks(n + 17)
    torch.manual_seed(5)
    d_packed = torch.randn(n, sum(s[f].reshape(n, -1).shape[1] for f in FEATS),
                           generator=torch.Generator().manual_seed(9))
    packed, tape = _run_hip(model, gs, masks, None, d_packed, device)
    perms = model.backbone.backbone.last_perms
    W = model.width
    relu = {f: [(h[:, g * W:(g + 1) * W] > 0).cpu() for h in tape["hs"]]
            for g, f in enumerate(model.output_features)}
    fused = [r["mlp_fused"] for st in tape["bb"]["enc"] + tape["bb"]["dec"] for r in st if r["kind"] == "block"]
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    return dict(model=model, sd=sd, s=s, n=n, gs=gs, masks=masks, perms=perms, d_packed=d_packed,
                packed=packed.cpu(), relu=relu, grads=grads, fused=fused)


def test_refiner_all_param_grads_match_oracle(all_run):
    """Every parameter's gradient against autograd of the CPU oracle (fp32 and fp64, HIP's DropPath masks and ReLU
    active sets replayed), per module.  Measured on an MI355X: aggregate HIP 1.41e-6 against the fp32 oracle's
    1.82e-6; largest error enc0.block0.attn.proj 3.81e-6 against 3.53e-6, largest ratio dec0.block0.norm1 1.34e-6
    against 3.76e-7."""
    r = all_run
    model, sd, s, n, masks, perms, d_packed = (r[k] for k in ("model", "sd", "s", "n", "masks", "perms", "d_packed"))
    cfg = ptv3_ref.PTv3Config(**BK)
    pnames = [k for k, _ in model.named_parameters()]
    assert not any(r["fused"])  # mlp.fc1 / fc2 train: every block took the unfused MLP branch

    def oracle(dtype):
        sdd = {k: (v.to(dtype) if v.is_floating_point() else v).clone() for k, v in sd.items()}
        for k in pnames:  # every parameter (the other floating-point entries are the BatchNorm running statistics,
            sdd[k].requires_grad_()  # which the train-mode forward updates in place)
        sc = {k: v.to(dtype) for k, v in s.items()}
        mk = {k: m.to(dtype) for k, m in masks.masks.items()}
        ref, _ = ptv3_ref.feature_predictor_forward(sdd, cfg, sc, perms, train=True, masks=mk, relu_masks=r["relu"])
        rp = torch.cat([ref[f].reshape(n, -1) for f in FEATS], 1)
        (rp * d_packed.to(dtype)).sum().backward()
        return sdd, rp.detach()

    sd32, ref_packed = oracle(torch.float32)
    in_packed = torch.cat([s[f].reshape(n, -1) for f in FEATS], 1)
    assert rel_l2(r["packed"] - in_packed, ref_packed - in_packed) < 1e-5
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        sd64, _ = oracle(torch.float64)
    finally:
        torch.set_default_dtype(prev)
    modules = {}
    for k in pnames:
        modules.setdefault(k.rsplit(".", 1)[0], []).append(k)
    compared = 0
    cat = lambda src, ks, f=(lambda t: t): torch.cat([f(src[k]).double().reshape(-1) for k in ks])
    rows = []
    for mod, ks in modules.items():
        assert all(sd64[k].grad is not None for k in ks), mod
        hip, r32, r64 = cat(r["grads"], ks), cat(sd32, ks, lambda t: t.grad), cat(sd64, ks, lambda t: t.grad)
        rows.append((mod, rel_l2(hip, r64), rel_l2(r32, r64)))
        compared += len(ks)
    print(f"\n[refiner all-parameter grads, n={n}] per module, error to the fp64 oracle: HIP / fp32 oracle")
    for mod, eh, er in rows:
        print(f"  {mod:55s} {eh:.2e} {er:.2e}{'   <-- over 4x' if eh > 4.0 * er + 1e-5 else ''}")
    hip, r32, r64 = (cat(r["grads"], pnames), cat(sd32, pnames, lambda t: t.grad),
                     cat(sd64, pnames, lambda t: t.grad))
    e_hip, e_ref = rel_l2(hip, r64), rel_l2(r32, r64)
    worst = max(rows, key=lambda t: t[1] / (4.0 * t[2] + 1e-5))
    print(f"  aggregate HIP {e_hip:.2e}, fp32 oracle {e_ref:.2e}; worst module {worst[0]} {worst[1]:.2e} vs "
          f"{worst[2]:.2e}")
    assert compared == sum(1 for p in model.parameters() if p.is_floating_point()) == len(pnames)
    assert e_hip <= 2.0 * e_ref + 1e-5, f"HIP {e_hip:.2e} vs fp32-oracle {e_ref:.2e} (to fp64)"
    for mod, eh, er in rows:
        assert eh <= 4.0 * er + 1e-5, f"{mod}: HIP {eh:.2e} vs fp32-oracle {er:.2e} (to fp64)"


def test_default_list_takes_none_of_the_new_code(all_run, device, monkeypatch):
    """finetune_list = ('attn.qkv',): the backward launches what it launched before this feature -- none of the new
    entry points, the fused MLP backward, no state kept for other layers -- and its qkv gradients are those of a
    run in which the new entry points are not callable at all: the same launch sequence, entry by entry.
    Two runs of those very launches are not bitwise equal on this path, before this feature either: the training
    forward's conv, the conv input gradient and the weight gradient's reduction splits add with float atomics in
    whatever order they finish.  Measured on an MI355X, run against run of the unchanged qkv-only path: 0 of 9 qkv
    modules bitwise equal, 1.2e-6 .. 1.5e-6 on the worst module (enc0.block0, the end of the backward), 6.6e-7 ..
    7.2e-7 over all qkv gradients together.  So the sequence of launches is what is compared exactly, and the
    gradients together to the 1e-6 allowed where float atomics reorder."""
    r = all_run
    model = _fresh(r, device)
    strain.select_trainable(model, ("attn.qkv",))
    _run_hip(model, r["gs"], ReplayMasks(r["masks"]), r["perms"], r["d_packed"], device)  # (builds the W^T caches)
    log = LaunchLog(monkeypatch)
    _, tape = _run_hip(model, r["gs"], ReplayMasks(r["masks"]), r["perms"], r["d_packed"], device)
    assert not NEW_ENTRIES & set(log.names)
    assert "sfx_affine_act" in log.names and "sfx_block_mlp_bwd" in log.names
    blocks = [x for st in tape["bb"]["enc"] + tape["bb"]["dec"] for x in st if x["kind"] == "block"]
    # the fused MLP launch wherever the fine-tuning recipe takes it (its channel counts), no conv input kept
    assert all(b["mlp_fused"] == pt.mlp_train_fused_ok(b["x2"], b["blk"].channels) for b in blocks)
    assert any(b["mlp_fused"] for b in blocks) and all(b["cpe_in"] is None for b in blocks)
    assert tape["x"] is None and tape["bb"]["emb"] is None
    first = {k: p.grad.clone() for k, p in model.named_parameters() if p.requires_grad}
    assert first and all("attn.qkv" in k for k in first)
    assert all(p.grad is None for k, p in model.named_parameters() if "attn.qkv" not in k)

    def forbidden(*a, **k):
        raise AssertionError("new code taken on the default path")

    for name in ("linear_wgrad_rs", "linear_wgrad_padk", "subm_conv_wgrad", "layernorm_wgrad", "gelu"):
        monkeypatch.setattr(tops, name, forbidden)
    n_first = len(log.names)
    names_first = list(log.names)
    _run_hip(model, r["gs"], ReplayMasks(r["masks"]), r["perms"], r["d_packed"], device)
    assert log.names[n_first:] == names_first
    second = {k: p.grad for k, p in model.named_parameters() if p.requires_grad}
    assert list(second) == list(first)
    exact = sum(int(torch.equal(g, second[k])) for k, g in first.items())
    e = rel_l2(torch.cat([second[k].reshape(-1) for k in first]), torch.cat([g.reshape(-1) for g in first.values()]))
    print(f"\n[default path] {exact} of {len(first)} qkv gradient tensors bitwise equal between the two runs; "
          f"all together {e:.2e}")
    assert exact == len(first) or e <= 1e-6


def test_subset_finetune_list(all_run, device):
    """A subset, the MLP Linears and the heads: only those get .grad, equal to the all-parameter run's.  The list
    holds substrings of parameter names (filter_grads): the MLP's Linears are named `...mlp.0.fc1` / `...mlp.0.fc2`
    (PointSequential(MLP)), so the substring that selects them is 'mlp.0.fc' ('mlp.fc' occurs in no name)."""
    r = all_run
    model = _fresh(r, device)
    sel = ("mlp.0.fc", "features_outputhead")
    assert not any("mlp.fc" in k for k, _ in model.named_parameters())
    strain.select_trainable(model, sel)
    _, tape = _run_hip(model, r["gs"], ReplayMasks(r["masks"]), r["perms"], r["d_packed"], device)
    blocks = [x for st in tape["bb"]["enc"] + tape["bb"]["dec"] for x in st if x["kind"] == "block"]
    assert blocks and not any(b["mlp_fused"] for b in blocks)  # the unfused MLP branch
    n_sel = 0
    worst = 0.0
    modules = {}
    for k, p in model.named_parameters():
        if any(t in k for t in sel):
            modules.setdefault(k.rsplit(".", 1)[0], []).append(k)
            n_sel += 1
        else:
            assert p.grad is None, k
    mp = dict(model.named_parameters())
    # float atomics reorder between any two runs (see test_default_list_takes_none_of_the_new_code; measured here:
    # 3.2e-7 .. 3.4e-7 over the selected gradients together, up to 9.8e-7 on single modules), so the selected
    # gradients are compared together, to 1e-6.  (Not per tensor: fc2's bias in the first block -- no DropPath, a
    # train-mode BatchNorm behind every path out of the block -- has an exactly zero true gradient.)
    for mod, ks in modules.items():
        worst = max(worst, rel_l2(torch.cat([mp[k].grad.cpu().reshape(-1) for k in ks]),
                                  torch.cat([r["grads"][k].reshape(-1) for k in ks])))
    sel_names = [k for ks in modules.values() for k in ks]
    e_all = rel_l2(torch.cat([mp[k].grad.cpu().reshape(-1) for k in sel_names]),
                   torch.cat([r["grads"][k].reshape(-1) for k in sel_names]))
    print(f"\n[subset] selected gradients vs the all-parameter run: together {e_all:.2e}, worst module {worst:.2e}")
    assert e_all <= 1e-6
    assert n_sel == 2 * 2 * len(blocks) + 2 * model.nlayer * len(model.output_features)
    # the optimiser: moments for exactly those, and the step runs
    model2 = _fresh(r, device)
    tr = strain.Trainer(model2, finetune_list=sel, generator=torch.Generator(device=device).manual_seed(0))
    names = [k for k, p in model2.named_parameters() if p.requires_grad]
    assert names and all(any(t in k for t in sel) for k in names)
    assert len(tr.params) == len(tr.exp_avg) == len(tr.exp_avg_sq) == n_sel
    cams = to_device(make_cameras(64, 64, n_views=2), device)
    gt = [torch.rand(64, 64, 3, device=device) for _ in range(2)]
    before = [p.detach().clone() for p in tr.params]
    loss = tr.step([r["gs"]], [cams], [gt])
    assert loss == loss and loss > 0
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, tr.params))


# ---- 5. Trainer end to end ------------------------------------------------------------------------------------
def test_trainer_all_parameters_lr_dict(device):
    torch.manual_seed(0)
    model = _model(33, **BK).to(device)
    lr = {"backbone": 3e-5, "means": 1e-5, "base": 0.0}
    tr = strain.Trainer(model, finetune_list=None, lr=lr, generator=torch.Generator(device=device).manual_seed(0))
    assert len(tr.params) == len(list(model.parameters()))
    s = to_device(make_scene(2000, 1, seed=6), device)
    cams = to_device(make_cameras(64, 64, n_views=2), device)
    gt = [torch.rand(64, 64, 3, device=device) for _ in range(2)]
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    stats = {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k}
    loss = tr.step([s], [cams], [gt])
    assert loss == loss and loss > 0
    for k, p in model.named_parameters():
        moves = k.startswith("backbone.") or k.startswith("features_outputhead.means.")
        assert torch.equal(before[k], p.detach()) != moves, k  # lr 0 keeps the bits, any other lr moves it
    after = model.state_dict()
    assert stats and all(not torch.equal(v, after[k]) for k, v in stats.items())  # running statistics updated
    sd = tr.state_dict()
    assert any(float(m.abs().max()) > 0 for m in sd["exp_avg"])
    tr2 = strain.Trainer(model, finetune_list=None, lr=lr, generator=torch.Generator(device=device).manual_seed(1))
    tr2.load_state_dict(sd)
    assert tr2.step_count == tr.step_count == 1
    for a, b in zip(tr.exp_avg + tr.exp_avg_sq, tr2.exp_avg + tr2.exp_avg_sq):
        assert torch.equal(a, b)
    tr3 = strain.Trainer(model, generator=torch.Generator(device=device).manual_seed(2))  # the qkv default
    with pytest.raises(ValueError):
        tr3.load_state_dict(sd)
