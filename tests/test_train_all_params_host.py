"""Host-side algebra of the all-parameter training backward (no GPU): the unfolding of the folded CPE conv's
gradients into cpe.0 / cpe.1, the scatter of the packed head gradients back to the per-feature heads, and the
parameter selection / learning-rate tables of the Trainer -- each against fp64 torch autograd."""
import copy

import pytest
import torch

from splatformer_amd import ptv3_train as pt
from splatformer_amd import train as strain
from splatformer_amd.feature_predictor import FeaturePredictor


def test_cpe_unfold_matches_autograd_of_linear_of_conv():
    """Linear(Conv(x)) on a dense stand-in: 27 random row gathers play the indice pairs of the 27 offsets."""
    g = torch.Generator().manual_seed(3)
    n, C = 40, 8
    x = torch.randn(n, C, generator=g, dtype=torch.float64)
    gathers = [torch.randint(0, n, (n,), generator=g) for _ in range(27)]
    keep = [(torch.rand(n, generator=g) < 0.6).double()[:, None] for _ in range(27)]  # absent neighbours
    w_conv = torch.randn(C, 3, 3, 3, C, generator=g, dtype=torch.float64, requires_grad=True)
    b_conv = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    w_lin = torch.randn(C, C, generator=g, dtype=torch.float64, requires_grad=True)
    b_lin = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dv = torch.randn(n, C, generator=g, dtype=torch.float64)
    xs = [x[gathers[k]] * keep[k] for k in range(27)]
    wk = w_conv.reshape(C, 27, C)
    u = sum(xs[k] @ wk[:, k].t() for k in range(27)) + b_conv
    v = u @ w_lin.t() + b_lin
    (v * dv).sum().backward()
    # what the training step has: the gradient of the folded conv W'_k = W_lin W_k, b' = W_lin b_conv + b_lin
    dwf = torch.stack([dv.t() @ xs[k] for k in range(27)], 1).reshape(C, 27 * C)
    dbf = dv.sum(0)
    dwc, dbc, dwl, dbl = pt.cpe_unfold_grads(dwf, dbf, w_conv.detach(), b_conv.detach(), w_lin.detach())
    for got, ref in ((dwc.reshape(w_conv.shape), w_conv.grad), (dbc, b_conv.grad), (dwl, w_lin.grad),
                     (dbl, b_lin.grad)):
        assert torch.allclose(got, ref, rtol=1e-12, atol=1e-12)


@pytest.fixture(scope="module")
def fp64_model():
    torch.manual_seed(11)
    return FeaturePredictor(sh_degree=1, zeroinit=False, backbone_kwargs=dict(
        enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1))).double()


def test_scatter_of_packed_head_grads_matches_unpacked_heads(fp64_model):
    fp = fp64_model
    g = torch.Generator().manual_seed(5)
    m = 17
    x = torch.randn(m, fp.head_in, generator=g, dtype=torch.float64)
    out_dim = sum(fp.ch[f] for f in fp.output_features)
    r = torch.randn(m, out_dim, generator=g, dtype=torch.float64)
    # reference: autograd of the unpacked per-feature heads
    ref = copy.deepcopy(fp.features_outputhead)
    o = torch.cat([ref[f](x) for f in fp.output_features], 1)
    (o * r).sum().backward()
    # packed forward / autograd of the packed matrices, then the scatter under test
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (the packed last layer is assembled in the default dtype)
    try:
        w1, b1, mids, wl, bl, od = fp._packed_heads()
    finally:
        torch.set_default_dtype(prev)
    assert od == out_dim and wl.dtype == torch.float64
    G, W = len(fp.output_features), fp.width
    leaves = [t.detach().clone().requires_grad_() for t in (w1, b1, wl, bl)]
    mleaves = [(wm.detach().clone().requires_grad_(), bm.detach().clone().requires_grad_()) for wm, bm in mids]
    xp = torch.nn.functional.pad(x, (0, w1.shape[1] - fp.head_in))
    h = torch.relu(xp @ leaves[0].t() + leaves[1])
    for wm, bm in mleaves:
        h = torch.relu(torch.cat([h[:, i * W:(i + 1) * W] @ wm[i].t() + bm[i] for i in range(G)], 1))
    op = h @ leaves[2].t() + leaves[3]
    assert torch.allclose(op, o.detach(), rtol=1e-12, atol=1e-12)
    (op * r).sum().backward()
    for p in fp.features_outputhead.parameters():
        p.requires_grad_(True)
        p.grad = None
    frozen = fp.features_outputhead["scales"][2].weight  # a frozen tensor gets no .grad
    frozen.requires_grad_(False)
    strain.scatter_head_grads(fp, leaves[0].grad, leaves[1].grad, [(a.grad, b.grad) for a, b in mleaves],
                              leaves[2].grad, leaves[3].grad)
    got = dict(fp.features_outputhead.named_parameters())
    n = 0
    for name, p in ref.named_parameters():
        if got[name] is frozen:
            assert got[name].grad is None
            continue
        assert torch.allclose(got[name].grad, p.grad, rtol=1e-12, atol=1e-12), name
        n += 1
    assert n == len(got) - 1
    frozen.requires_grad_(True)


def test_check_trainable_accepts_every_backbone_parameter(fp64_model):
    bb = fp64_model.backbone.backbone
    strain.select_trainable(fp64_model, None)
    assert all(p.requires_grad for p in fp64_model.parameters())
    pt.check_trainable(bb)  # nothing unsupported in the backbone as it is
    bb.register_parameter("extra_scale", torch.nn.Parameter(torch.ones(1)))
    try:
        with pytest.raises(NotImplementedError, match="extra_scale"):
            pt.check_trainable(bb)
    finally:
        del bb._parameters["extra_scale"]


def test_select_trainable_and_lr_dict(fp64_model):
    fp = fp64_model
    strain.select_trainable(fp, ("mlp.0.fc", "features_outputhead"))
    on = {n for n, p in fp.named_parameters() if p.requires_grad}
    assert any("mlp.0.fc1" in n for n in on) and any("features_outputhead" in n for n in on)
    assert {n for n, _ in fp.named_parameters() if "mlp.0.fc" in n or "features_outputhead" in n} == on
    strain.select_trainable(fp, ("attn.qkv",))
    assert all(("attn.qkv" in n) == p.requires_grad for n, p in fp.named_parameters())
    lrs = strain.param_lrs(fp, {"backbone": 3e-5, "means": 1e-5, "base": 0.0})
    for n, p in fp.named_parameters():
        want = 3e-5 if n.startswith("backbone.") else (1e-5 if n.startswith("features_outputhead.means.") else 0.0)
        assert lrs[id(p)] == want, n
    assert set(strain.param_lrs(fp, 2e-4).values()) == {2e-4}
    with pytest.raises(ValueError):
        strain.param_lrs(fp, {"backbone": 1e-4})
    strain.select_trainable(fp, None)
