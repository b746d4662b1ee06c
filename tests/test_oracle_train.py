"""oracle/train_ref.py pinned to torch in fp64, the proof that the inputs of tests/test_gpu_train_kernels.py are
discriminating (a deliberately wrong formula misses the correct one by more than the bar the GPU test applies, on the
same inputs), and the host-side argument checks of the training entries.  No GPU."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import train_cases as tc
from oracle import train_ref as tr

D = torch.float64


def d(t):
    return t.double()


def close(a, b, tol=1e-12):
    return tc.rel_l2(a, b) < tol


# ---- pins to torch (fp64) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C", [(1, 64), (33, 48), (261, 96), (31, 500)])
def test_layernorm_restatements_match_autograd(M, C):
    c = {k: d(v) for k, v in tc.ln_case(M, C).items()}
    g = tc.gen(11, M, C)
    beta = torch.randn(C, generator=g, dtype=D)
    x = c["x"].clone().requires_grad_()
    gamma = c["gamma"].clone().requires_grad_()
    b = beta.clone().requires_grad_()
    F.layer_norm(x, (C,), gamma, b, tc.LN_EPS).backward(c["dy"])
    assert close(tr.layernorm_bwd(c["x"], c["gamma"], c["dy"], tc.LN_EPS), x.grad)
    assert close(tr.layernorm_bwd(c["x"], c["gamma"], c["dy"], tc.LN_EPS, c["dres"]), x.grad + c["dres"])
    dgamma, dbeta = tr.layernorm_wgrad(c["x"], c["dy"], tc.LN_EPS)
    assert close(dgamma, gamma.grad) and close(dbeta, b.grad)
    # block tail: x1 = xx + LN_cpe(u), h = LN1(x1); gradients dh into h and dx2 into x1 directly
    u = c["u"].clone().requires_grad_()
    x1 = c["x"].clone().requires_grad_()
    (F.layer_norm(x1, (C,), c["gamma"], beta, tc.LN_EPS) * c["dy"]).sum().backward()
    dx1_ref = x1.grad + c["dx2"]
    F.layer_norm(u, (C,), c["g_cpe"], beta, tc.LN_EPS).backward(dx1_ref)
    dx1, du = tr.cpe_ln_bwd(c["u"], c["x"], c["g_cpe"], c["gamma"], c["dx2"], c["dy"], tc.LN_EPS)
    assert close(dx1, dx1_ref) and close(du, u.grad)


def _bn_module(c, C):
    bn = torch.nn.BatchNorm1d(C, eps=tc.BN_EPS, momentum=tc.BN_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["running_mean"])
        bn.running_var.copy_(c["running_var"])
    return bn.train()


BN_SHAPES = [(127, 64), (128, 63), (129, 65), (385, 300)]


def _bn64(M, C):
    return {k: (d(v) if v.is_floating_point() else v) for k, v in tc.bn_case(M, C).items()}


@pytest.mark.parametrize("M,C", BN_SHAPES)
@pytest.mark.parametrize("act", [0, 1])
def test_batchnorm_restatement_matches_module(M, C, act):
    c = _bn64(M, C)
    bn = _bn_module(c, C)
    x = c["x"].clone().requires_grad_()
    z = bn(x)
    y = (F.gelu(z) if act else z) + c["res"][c["ridx"].long()]
    y.backward(c["dy"])
    r = tc.bn_chain_ref(c, act, "idx", D)
    assert close(r["y"], y) and close(r["dx"], x.grad, 1e-10)
    assert close(r["running_mean"], bn.running_mean) and close(r["running_var"], bn.running_var)
    assert close(r["bwd_sums"][0], bn.bias.grad, 1e-10) and close(r["bwd_sums"][1], bn.weight.grad, 1e-10)
    # two-pass moments are the summed-statistics ones, and two ranks' sums add up to the batch's
    mean, var = tr.bn_moments(c["x"])
    assert close(mean, r["mean"]) and close(1.0 / torch.sqrt(var + tc.BN_EPS), r["rstd"], 1e-9)
    h = M // 2
    assert close(tr.bn_sums(c["x"][:h]) + tr.bn_sums(c["x"][h:]), tr.bn_sums(c["x"]))
    halves = [tr.bn_bwd_sums(c["x"][s], r["mean"], r["rstd"], c["gamma"], c["beta"], act, c["dy"][s])
              for s in (slice(0, h), slice(h, M))]
    assert close(halves[0] + halves[1], r["bwd_sums"], 1e-10)


SEG_CS = (1, 30, 64, 96, 128, 200, 256, 300, 512)


@pytest.mark.parametrize("layout", tc.SEGMENT_LAYOUTS)
@pytest.mark.parametrize("C", [1, 30, 200])
def test_segment_restatements_match_plain_loop(C, layout):
    c = tc.segment_case(C, layout)
    x, ptr_, sidx = c["x"], c["idx_ptr"], c["sidx"]
    y, arg = tr.segment_max_arg(x, ptr_, sidx)
    s = tr.segment_sum(d(c["xs"]), ptr_, sidx)
    dx = tr.segment_max_bwd(c["dy"], arg, c["n"])
    xl, xsl = x.tolist(), d(c["xs"]).tolist()
    seen = 0
    for seg in range(c["m"]):
        for col in range(C):
            best, where, tot = None, -1, 0.0
            for p in range(ptr_[seg], ptr_[seg + 1]):
                v = xl[sidx[p]][col]
                tot += xsl[sidx[p]][col]
                if where < 0 or v > best:
                    best, where = v, sidx[p]
            assert int(arg[seg, col]) == where
            assert torch.tensor(best).view(torch.int32) == y[seg, col].view(torch.int32)  # sign of zero included
            assert float(s[seg, col]) == tot
            assert float(dx[where, col]) == float(c["dy"][seg, col])
            seen += 1
    assert int((dx != 0).sum()) == seen  # nothing but the arg rows, no gradient split over a tie


@pytest.mark.parametrize("act", [1, 2, 3])
def test_activation_derivatives_match_autograd(act):
    c = tc.act_case(act)
    p = d(c["pre"])
    if act == 3:
        z = torch.atanh(p).requires_grad_()
        torch.tanh(z).sum().backward()
    else:
        z = p.clone().requires_grad_()
        (F.gelu(z) if act == 1 else torch.relu(z)).sum().backward()
    assert close(tr.act_grad(p, act), z.grad, 1e-9)
    assert torch.equal(tr.act_bwd(d(c["dy"]), p, act, 3)[:, 3:], d(c["dy"])[:, 3:])


@pytest.mark.parametrize("scale", [3.0, 1e-3, 0.0])
def test_clip_coef_matches_clip_grad_norm(scale):
    grads = [d(g) * scale for g in tc.grads_case(257)]
    ps = [torch.zeros_like(g).requires_grad_() for g in grads]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, 2.0)
    norm = tr.grad_norm(grads)
    coef = tr.clip_coef(norm, 2.0)
    assert close(norm, total) or (scale == 0.0 and float(norm) == 0.0 == float(total))
    for p, g in zip(ps, grads):
        assert torch.allclose(p.grad, g * coef, rtol=1e-13, atol=0)
    assert (float(coef) == 1.0) == (scale != 3.0)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_adam_restatement_matches_torch_optim(wd, eps):
    c = tc.adam_case(257)
    p_ref = d(c["p"]).clone().requires_grad_()
    opt = torch.optim.Adam([p_ref], lr=0.1, eps=eps, weight_decay=wd)
    p, m1, m2 = d(c["p"]), torch.zeros(257, dtype=D), torch.zeros(257, dtype=D)
    for step in (1, 2, 3):
        g = d(c["grads"][step - 1])
        p_ref.grad = g * 0.37
        opt.step()
        p, m1, m2 = tr.adam_step(p, g, m1, m2, step, 0.1, 0.9, 0.999, eps, wd, grad_scale=0.37)
        st = opt.state[p_ref]
        assert close(p, p_ref) and close(m1, st["exp_avg"]) and close(m2, st["exp_avg_sq"])
        assert bool(torch.isfinite(p).all())


# ---- the GPU tests' inputs are discriminating: a wrong variant misses by more than the bar ------------------------
@pytest.mark.parametrize("layout", ["one", "mix", "reversed"])
@pytest.mark.parametrize("C", SEG_CS)
def test_wrong_last_maximum_is_caught(C, layout):
    """Last instead of first maximum in run order (the first maximum of the reversed runs): arg and the scattered
    gradient are compared exactly on the GPU, and both differ."""
    c = tc.segment_case(C, layout)
    p = c["idx_ptr"]
    rev = [r for s in range(c["m"]) for r in reversed(c["sidx"][p[s]:p[s + 1]])]
    y, arg = tr.segment_max_arg(c["x"], p, c["sidx"])
    y2, arg2 = tr.segment_max_arg(c["x"], p, rev)
    assert torch.equal(y, y2) and not torch.equal(arg, arg2)
    assert tc.rel_l2(tr.segment_max_bwd(c["dy"], arg2, c["n"]), tr.segment_max_bwd(c["dy"], arg, c["n"])) > tc.BAR_TIGHT
    # and the signed zero of the first maximum differs from the last one's
    if C >= 3:
        assert not torch.equal(y.view(torch.int32), y2.view(torch.int32))


@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_wrong_batchnorm_statistics_are_caught(M, C):
    c = _bn64(M, C)
    r = tc.bn_chain_ref(c, 1, "none", D)
    # biased instead of unbiased running variance (the GPU test: rel_l2 < 1e-6)
    biased = (1 - tc.BN_MOMENTUM) * c["running_var"] + tc.BN_MOMENTUM * (1.0 / r["rstd"] ** 2 - tc.BN_EPS)
    assert tc.rel_l2(biased, r["running_var"]) > tc.BAR_TIGHT
    # count = rows of one rank instead of the global count, on the sums of the two halves
    r32 = tc.bn_chain_ref(c, 1, "none", torch.float32)
    h = M // 2
    mean, var = tr.bn_stats_from_sums(tr.bn_sums(c["x"]), float(h))
    rstd, scale, shift, _, _ = tr.bn_finalize(mean, var, float(h), c["gamma"], c["beta"], tc.BN_EPS, tc.BN_MOMENTUM)
    y = tr.affine_act(c["x"], scale, shift, 1)
    assert bool((tc.slice_err(y, r["y"], 0) > tc.slice_bar(r32["y"], r["y"], 0)).all())
    dx = tr.bn_bwd_apply(c["x"], r["mean"], r["rstd"], c["gamma"], c["beta"], 1, c["dy"], r["bwd_sums"], float(h))
    assert bool((tc.slice_err(dx, r["dx"], 0) > tc.slice_bar(r32["dx"], r["dx"], 0)).all())
    # GELU' without the density term x * phi(x)
    xh = (c["x"] - r["mean"]) * r["rstd"]
    z = xh * c["gamma"] + c["beta"]
    g = c["dy"] * 0.5 * (1.0 + torch.erf(z * 0.7071067811865475244))
    dx = c["gamma"] * r["rstd"] * (g - g.mean(0) - xh * (g * xh).mean(0))
    assert bool((tc.slice_err(dx, r["dx"], 0) > tc.slice_bar(r32["dx"], r["dx"], 0)).all())


@pytest.mark.parametrize("act", [1, 2, 3])
def test_wrong_activation_backward_is_caught(act):
    c = tc.act_case(act)
    dy, pre = d(c["dy"]), d(c["pre"])
    N = dy.shape[1]
    for ncols in (0, 3):  # ncols ignored
        assert tc.rel_l2(tr.act_bwd(dy, pre, act, N), tr.act_bwd(dy, pre, act, ncols)) > tc.BAR_TIGHT
    if act == 1:  # GELU' without the density term
        wrong = dy * 0.5 * (1.0 + torch.erf(pre * 0.7071067811865475244))
        assert tc.rel_l2(wrong, tr.act_bwd(dy, pre, 1, N)) > tc.BAR_TIGHT


@pytest.mark.parametrize("n", tc.SUMSQ_SIZES)
def test_unclamped_clip_coef_is_caught(n):
    """The GPU test wants coef bit-exactly 1.0f when the norm is below max_norm (= twice the norm, as there)."""
    norm = tr.grad_norm([d(g) for g in tc.grads_case(n)])
    max_norm = 2.0 * float(norm)
    assert float(tr.clip_coef(norm, max_norm)) == 1.0
    assert float(torch.tensor(max_norm / (float(norm) + 1e-6), dtype=torch.float32)) != 1.0


ADAM_SIZES = (1, 255, 256, 257, 70001)


@pytest.mark.parametrize("n", ADAM_SIZES)
@pytest.mark.parametrize("eps", [1e-15, 1e-8])
def test_wrong_adam_variants_are_caught(n, eps):
    c = tc.adam_case(n)
    p, m1, m2 = d(c["p"]), torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    for step in (1, 2, 3):
        g = d(c["grads"][step - 1])
        for wd in (0.0, 1e-2):
            ok = tr.adam_step(p, g, m1, m2, step, 0.1, 0.9, 0.999, eps, wd)
            if step == 3:  # no bias correction (1 - beta^step -> 1)
                assert tc.rel_l2(tr.adam_step(p, g, m1, m2, 10 ** 9, 0.1, 0.9, 0.999, eps, wd)[0], ok[0]) > tc.BAR_TIGHT
            if wd:  # AdamW: the decay applied to the parameter, not folded into the gradient
                w = tr.adam_step(p * (1 - 0.1 * wd), g, m1, m2, step, 0.1, 0.9, 0.999, eps, 0.0)
                assert all(tc.rel_l2(a, b) > tc.BAR_TIGHT for a, b in zip(w, ok))
        p, m1, m2 = tr.adam_step(p, g, m1, m2, step, 0.1, 0.9, 0.999, eps, 0.0)


# ---- host-side argument checks -----------------------------------------------------------------------------------
def test_training_entries_check_arguments_without_gpu():
    """A too-small leading dimension, a NULL required buffer and C = 513 fail host-side with -1 and a message (no
    kernel launched: the buffers are host memory that is never read)."""
    from splatformer_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    b = ctypes.addressof(buf)

    def fails(name, msg, *args):
        assert getattr(lib, name)(*args) == -1, name
        assert msg in lib.sfx_last_error(), (name, lib.sfx_last_error())

    M, C = 8, 64
    ln = lambda **k: (k.get("M", M), k.get("C", C), k.get("X", b), k.get("ldx", C), b, b, k.get("ldgy", C),
                      k.get("dR", None), k.get("ldr", 0), 1e-5, k.get("dX", b), k.get("lddx", C), None)
    fails("sfx_layernorm_bwd", b"C must be in [1, 512]", *ln(C=513, ldx=513, ldgy=513, lddx=513))
    fails("sfx_layernorm_bwd", b"null buffer", *ln(X=None))
    fails("sfx_layernorm_bwd", b"null buffer", *ln(dX=None))
    for k in ("ldx", "ldgy", "lddx"):
        fails("sfx_layernorm_bwd", b"sfx_layernorm_bwd: leading dim", *ln(**{k: C - 1}))
    fails("sfx_layernorm_bwd", b"sfx_layernorm_bwd: leading dim", *ln(dR=b, ldr=C - 1))
    assert lib.sfx_layernorm_bwd(*ln(M=0, X=None)) == 0
    fails("sfx_cpe_ln_bwd", b"C must be in [1, 512]", M, 513, b, b, b, b, b, b, 1e-5, b, b, None)
    fails("sfx_cpe_ln_bwd", b"null buffer", M, C, b, None, b, b, b, b, 1e-5, b, b, None)
    fails("sfx_layernorm_wgrad", b"C must be in [1, 512]", M, 513, b, 513, b, 513, 1e-5, b, 1 << 20, b, b, 0, None)
    fails("sfx_layernorm_wgrad", b"null buffer", M, C, None, C, b, C, 1e-5, b, 1 << 20, b, b, 0, None)
    fails("sfx_layernorm_wgrad", b"leading dim", M, C, b, C - 1, b, C, 1e-5, b, 1 << 20, b, b, 0, None)
    ws = 1 << 20
    fails("sfx_bn_stats", b"sfx_bn_stats: leading dim", M, C, b, C - 1, b, ws, b, None)
    fails("sfx_affine_act", b"sfx_affine_act: leading dim", M, C, b, C - 1, b, b, 1, None, 0, None, b, C, None)
    fails("sfx_affine_act", b"sfx_affine_act: leading dim", M, C, b, C, b, b, 1, None, 0, None, b, C - 1, None)
    fails("sfx_affine_act", b"sfx_affine_act: leading dim", M, C, b, C, b, b, 1, b, C - 1, None, b, C, None)
    fails("sfx_bn_act_bwd_reduce", b"sfx_bn_act_bwd_reduce: leading dim", M, C, b, C, b, b, b, b, 1, b, C - 1, b, ws, b,
          None)
    fails("sfx_bn_act_bwd_reduce", b"sfx_bn_act_bwd_reduce: leading dim", M, C, b, C - 1, b, b, b, b, 1, b, C, b, ws, b,
          None)
    for lds in ((C - 1, C, C), (C, C - 1, C), (C, C, C - 1)):
        fails("sfx_bn_act_bwd_apply", b"sfx_bn_act_bwd_apply: leading dim", M, C, b, lds[0], b, b, b, b, 1, b, lds[1], b,
              float(M), b, lds[2], 0, None)
        fails("sfx_act_bwd", b"sfx_act_bwd: leading dim", M, C, b, lds[0], b, lds[1], 1, C, b, lds[2], None)
    fails("sfx_segment_sum", b"sfx_segment_sum: leading dim", M, C, b, b, b, C - 1, b, None)
