"""The training step's norm, pooling, activation and optimiser kernels (csrc/train.hip) at their edges, against the
fp64 restatements of oracle/train_ref.py on the inputs of oracle/train_cases.py (tests/test_oracle_train.py shows on
the CPU that a wrong formula misses these bars on the same inputs).

Bars (tests/test_gpu_train_ops.py's and tests/test_gpu_train_all_params.py's rules):
- whole tensor: rel_l2 < 1e-5 to fp64; 1e-6 for the segment ops, the activation backward and the optimiser;
- per row (LayerNorm family) / per column (BatchNorm family): error to fp64 <= 4 x the error of the same formula
  evaluated in fp32 on the CPU + 1e-5;
- arg-max, scatter, transpose, untouched columns and every padding element: exact.
Every strided output is a view of a sentinel-filled parent; its padding columns and the rows past M must keep the
sentinel.  Each test prints its worst figures (`EDGE <op> <family> <error>`; profiles/train_kernels_edges.txt)."""
import numpy as np
import pytest
import torch

from oracle import train_cases as tc
from oracle import train_ref as tr
from splatformer_amd import ptv3_ops as ops
from splatformer_amd import train_ops as tops
from splatformer_amd._lib import call, stream

pytestmark = pytest.mark.gpu

SENT = -7777.25  # sentinel of the parent buffers
D = torch.float64
_worst = {}


def note(op, family, err):
    key = (op, family)
    _worst[key] = max(_worst.get(key, 0.0), float(err))
    print(f"EDGE {op} {family} {_worst[key]:.3e}")


def f32(v):
    """A Python float as the C ABI's `float` parameter carries it."""
    return float(np.float32(v))


class View:
    """A [M, C] float32 device matrix with leading dimension `ld`, `off` floats into a sentinel-filled parent that
    also holds two rows past M."""

    def __init__(self, src, dev, ld=None, off=0, M=None, C=None):
        M, C = (src.shape if src is not None else (M, C))
        ld = C if ld is None else ld
        self.parent = torch.full((off + (M + 2) * ld + 4,), SENT, device=dev, dtype=torch.float32)
        self.t = torch.as_strided(self.parent, (M, C), (ld, 1), off)
        if src is not None:
            self.t.copy_(src.to(dev))

    def padding_intact(self):
        chk = self.parent.clone()
        torch.as_strided(chk, self.t.shape, self.t.stride(), self.t.storage_offset()).fill_(SENT)
        return bool((chk == SENT).all())


# layouts of the LayerNorm operands: (leading-dimension excess, offset in floats)
LAYOUTS = {"contig": (0, 0), "ld+4": (4, 0), "offset1": (4, 1), "ld+1": (1, 0)}
LN_MS = (1, 31, 32, 33, 261)


def _check_rows(op, family, got, ref, ref32):
    err, bar = tc.slice_err(got, ref, 1), tc.slice_bar(ref32, ref, 1)
    note(op, family, err.max())
    note(op + "(fp32 cpu)", family, tc.slice_err(ref32, ref, 1).max())
    assert tc.rel_l2(got, ref) < tc.BAR_TENSOR
    bad = torch.nonzero(err > bar).flatten().tolist()
    assert not bad, (family, bad[:8], err[bad[:8]].tolist(), bar[bad[:8]].tolist())


def _ln_run(c, dev, C, layout, with_res):
    pad, off = LAYOUTS[layout]
    ld = C + pad
    x, dy = View(c["x"], dev, ld, off), View(c["dy"], dev, ld, off)
    dr = View(c["dres"], dev, ld, off) if with_res else None
    out = View(None, dev, ld, off, *c["x"].shape)
    # gamma stays 16-byte aligned except in the offset layout
    gbuf = torch.empty(C + 1, device=dev)
    gamma = gbuf[off:off + C]
    gamma.copy_(c["gamma"].to(dev))
    tops.layernorm_bwd(x.t, gamma, dy.t, tc.LN_EPS, dres=dr.t if dr else None, out=out.t)
    assert out.padding_intact()
    return out.t.clone()


def _ln_refs(c, with_res):
    c64 = {k: v.double() for k, v in c.items()}
    ref = tr.layernorm_bwd(c64["x"], c64["gamma"], c64["dy"], tc.LN_EPS, c64["dres"] if with_res else None)
    ref32 = tr.layernorm_bwd(c["x"], c["gamma"], c["dy"], tc.LN_EPS, c["dres"] if with_res else None)
    return ref, ref32


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("C", [64, 96, 128, 256, 512])
def test_layernorm_bwd_vector_widths(device, C, layout):
    """Row counts ragged against the 4 / 8 / 16 / 32 rows a workgroup holds; contiguous, ld = C + 4 (vector kernel),
    a base one float into the buffer and ld = C + 1 (both: the scalar fallback); with and without dres."""
    for M in LN_MS:
        c = tc.ln_case(M, C)
        for with_res in (False, True):
            got = _ln_run(c, device, C, layout, with_res)
            _check_rows("layernorm_bwd", f"C={C},{layout}", got, *_ln_refs(c, with_res))


@pytest.mark.parametrize("C", [48, 65, 192, 500])
def test_layernorm_bwd_scalar_widths(device, C):
    for M in LN_MS:
        c = tc.ln_case(M, C)
        for layout in ("contig", "ld+4"):
            for with_res in (False, True):
                got = _ln_run(c, device, C, layout, with_res)
                _check_rows("layernorm_bwd", f"C={C},scalar", got, *_ln_refs(c, with_res))


def test_layernorm_bwd_fallback_agrees_with_vector_kernel(device):
    """C = 64: the scalar fallback against the vector kernel, under the bar each meets against fp64 (two summation
    orders: not bitwise)."""
    for M in LN_MS:
        c = tc.ln_case(M, 64)
        ref, ref32 = _ln_refs(c, True)
        vec = _ln_run(c, device, 64, "ld+4", True)
        for layout in ("offset1", "ld+1"):
            fb = _ln_run(c, device, 64, layout, True)
            err = tc.slice_err(fb, vec, 1)
            note("layernorm_bwd", "C=64,fallback-vs-vector", err.max())
            assert bool((err <= tc.slice_bar(ref32, ref, 1)).all())


def _cpe_run(c, dev, off):
    M, C = c["x"].shape
    ins = {k: View(c[k], dev, C, off) for k in ("u", "x", "dx2", "dy")}
    gb = torch.empty(2, C + 4, device=dev)  # both rows 16-byte aligned when off = 0
    gc, g1 = gb[0, off:off + C], gb[1, off:off + C]
    gc.copy_(c["g_cpe"].to(dev))
    g1.copy_(c["gamma"].to(dev))
    dx1, du = View(None, dev, C, off, M, C), View(None, dev, C, off, M, C)
    call("sfx_cpe_ln_bwd", M, C, ins["u"].t.data_ptr(), ins["x"].t.data_ptr(), gc.data_ptr(), g1.data_ptr(),
         ins["dx2"].t.data_ptr(), ins["dy"].t.data_ptr(), tc.LN_EPS, dx1.t.data_ptr(), du.t.data_ptr(), stream())
    assert dx1.padding_intact() and du.padding_intact()
    return dx1.t.clone(), du.t.clone()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("C", [64, 96, 128, 256, 512, 48, 65, 192, 500])
def test_cpe_ln_bwd_widths_and_bases(device, C, off):
    """The fused block tail (contiguous rows, per its ABI) from an aligned base and from one float further."""
    for M in LN_MS:
        c = tc.ln_case(M, C)
        c64 = {k: v.double() for k, v in c.items()}
        ref = tr.cpe_ln_bwd(c64["u"], c64["x"], c64["g_cpe"], c64["gamma"], c64["dx2"], c64["dy"], tc.LN_EPS)
        ref32 = tr.cpe_ln_bwd(c["u"], c["x"], c["g_cpe"], c["gamma"], c["dx2"], c["dy"], tc.LN_EPS)
        got = _cpe_run(c, device, off)
        fam = f"C={C},{'offset1' if off else 'aligned'}"
        _check_rows("cpe_ln_bwd.dx1", fam, got[0], ref[0], ref32[0])
        _check_rows("cpe_ln_bwd.du", fam, got[1], ref[1], ref32[1])


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("C", [48, 500])
def test_layernorm_wgrad_scalar_widths_and_views(device, C, pad):
    for M in (33, 261):
        c = tc.ln_case(M, C)
        x, dy = View(c["x"], device, C + pad), View(c["dy"], device, C + pad)
        base = torch.randn(2, C, generator=tc.gen(7, M, C))
        ref = tr.layernorm_wgrad(c["x"].double(), c["dy"].double(), tc.LN_EPS)
        for acc in (False, True):
            dg, db = base[0].to(device), base[1].to(device)
            tops.layernorm_wgrad(x.t, dy.t, tc.LN_EPS, dg, db, accumulate=acc)
            e = max(tc.rel_l2(dg, ref[0] + (base[0].double() if acc else 0)),
                    tc.rel_l2(db, ref[1] + (base[1].double() if acc else 0)))
            note("layernorm_wgrad", f"C={C},ld=C+{pad}", e)
            assert e < tc.BAR_TENSOR


# ---- BatchNorm chain ------------------------------------------------------------------------------------------
BN_SHAPES = [(127, 64), (128, 63), (129, 65), (385, 300)]


def _check_cols(op, family, got, ref, ref32):
    err, bar = tc.slice_err(got, ref, 0), tc.slice_bar(ref32, ref, 0)
    note(op, family, err.max())
    note(op + "(fp32 cpu)", family, tc.slice_err(ref32, ref, 0).max())
    assert tc.rel_l2(got, ref) < tc.BAR_TENSOR
    bad = torch.nonzero(err > bar).flatten().tolist()
    assert not bad, (family, bad[:8], err[bad[:8]].tolist(), bar[bad[:8]].tolist())


def _bn_refs(c, act, residual):
    return tc.bn_chain_ref(c, act, residual, D), tc.bn_chain_ref(c, act, residual, torch.float32)


def _bn_module(c, C, dev):
    bn = torch.nn.BatchNorm1d(C, eps=tc.BN_EPS, momentum=tc.BN_MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(c["gamma"])
        bn.bias.copy_(c["beta"])
        bn.running_mean.copy_(c["running_mean"])
        bn.running_var.copy_(c["running_var"])
    return bn.to(dev)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_chain_strided_flags(device, M, C, act):
    """Strided X, dY, dX and Y; residual gathered through ridx, row for row (ldr > C) and absent; accumulate 0 / 1 onto
    a random base; running statistics updated once, and left alone when NULL."""
    c = tc.bn_case(M, C)
    fam = f"M={M},C={C},act={act}"
    x, dy = View(c["x"], device, C + 3), View(c["dy"], device, C + 5)
    for residual in ("idx", "rows", "none"):
        r64, r32 = _bn_refs(c, act, residual)
        bn = _bn_module(c, C, device)
        res = {"idx": c["res"].to(device), "rows": View(c["res_rows"], device, C + 2).t, "none": None}[residual]
        ridx = c["ridx"].to(device) if residual == "idx" else None
        y = View(None, device, C + 1, 0, M, C)
        _, st = tops.bn_train_forward(x.t, bn, act, residual=res, residual_idx=ridx, out=y.t)
        assert y.padding_intact()
        _check_cols("bn_forward.y", fam, y.t, r64["y"], r32["y"])
        for k in ("mean", "rstd", "scale", "shift"):
            note("bn_finalize." + k, fam, tc.rel_l2(getattr(st, k), r64[k]))
            assert tc.rel_l2(getattr(st, k), r64[k]) < tc.BAR_TIGHT
        for k in ("running_mean", "running_var"):
            note("bn_finalize." + k, fam, tc.rel_l2(getattr(bn, k), r64[k]))
            assert tc.rel_l2(getattr(bn, k), r64[k]) < tc.BAR_TIGHT
        # NULL running statistics: same output, the module's statistics keep their bits
        before = (bn.running_mean.clone(), bn.running_var.clone())
        y2, st2 = tops.bn_train_forward(x.t, bn, act, residual=res, residual_idx=ridx, update_running=False)
        assert torch.equal(y2, y.t) and torch.equal(st2.mean, st.mean) and torch.equal(st2.rstd, st.rstd)
        assert torch.equal(bn.running_mean, before[0]) and torch.equal(bn.running_var, before[1])
        if residual != "idx":
            continue
        for acc in (False, True):
            dx = View(c["base"], device, C + 4)
            tops.bn_act_bwd(st, bn, act, dy.t, out=dx.t, accumulate=acc)
            assert dx.padding_intact()
            add64, add32 = (c["base"].double(), c["base"]) if acc else (0.0, 0.0)
            _check_cols("bn_act_bwd.dx", fam + f",acc={int(acc)}", dx.t, r64["dx"] + add64, r32["dx"] + add32)


def _bn_stats(xv, dev):
    M, C = xv.shape
    ws, nbytes = tops._colsum_ws(M, C, dev)
    sums = torch.empty(2 * C, device=dev, dtype=D)
    call("sfx_bn_stats", M, C, xv.data_ptr(), xv.stride(0), ws.data_ptr(), nbytes, sums.data_ptr(), stream())
    return sums


def _bn_bwd_sums(xv, dyv, mean, rstd, gamma, beta, act, dev):
    M, C = xv.shape
    ws, nbytes = tops._colsum_ws(M, C, dev)
    sums = torch.empty(2 * C, device=dev, dtype=D)
    call("sfx_bn_act_bwd_reduce", M, C, xv.data_ptr(), xv.stride(0), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
         beta.data_ptr(), act, dyv.data_ptr(), dyv.stride(0), ws.data_ptr(), nbytes, sums.data_ptr(), stream())
    return sums


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_two_rank_sums_and_determinism(device, M, C, act):
    """SyncBatchNorm arithmetic without a process group: statistics and backward sums of the two halves of the batch
    added, finalised / applied with count = M and NULL running statistics -- against the restatement with the global
    count and against the single-call result; the two reductions run twice give the same bits."""
    c = tc.bn_case(M, C)
    fam = f"M={M},C={C},act={act},two-rank"
    r64, r32 = _bn_refs(c, act, "none")
    x, dy = View(c["x"], device, C + 3), View(c["dy"], device, C + 5)
    gamma, beta = c["gamma"].to(device), c["beta"].to(device)
    h = M // 2
    halves = (slice(0, h), slice(h, M))
    whole = _bn_stats(x.t, device)
    assert torch.equal(whole, _bn_stats(x.t, device))
    sums = _bn_stats(x.t[halves[0]], device) + _bn_stats(x.t[halves[1]], device)
    assert tc.rel_l2(sums, whole) < 1e-14
    mean, rstd, scale, shift = (torch.empty(C, device=device) for _ in range(4))
    call("sfx_bn_finalize", C, float(M), sums.data_ptr(), gamma.data_ptr(), beta.data_ptr(), tc.BN_EPS, tc.BN_MOMENTUM,
         None, None, mean.data_ptr(), rstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), stream())
    for k, v in (("mean", mean), ("rstd", rstd), ("scale", scale), ("shift", shift)):
        note("bn_finalize." + k, fam, tc.rel_l2(v, r64[k]))
        assert tc.rel_l2(v, r64[k]) < tc.BAR_TIGHT
    bn = _bn_module(c, C, device)
    y1, st = tops.bn_train_forward(x.t, bn, act)
    y = View(None, device, C + 1, 0, M, C)
    call("sfx_affine_act", M, C, x.t.data_ptr(), C + 3, scale.data_ptr(), shift.data_ptr(), act, None, 0, None,
         y.t.data_ptr(), C + 1, stream())
    assert y.padding_intact()
    _check_cols("bn_forward.y", fam, y.t, r64["y"], r32["y"])
    assert bool((tc.slice_err(y.t, y1, 0) <= tc.slice_bar(r32["y"], r64["y"], 0)).all())
    # backward: each half reduces its rows, the sums are added, each half applies them with the global count
    whole_b = _bn_bwd_sums(x.t, dy.t, mean, rstd, gamma, beta, act, device)
    assert torch.equal(whole_b, _bn_bwd_sums(x.t, dy.t, mean, rstd, gamma, beta, act, device))
    bsums = sum(_bn_bwd_sums(x.t[s], dy.t[s], mean, rstd, gamma, beta, act, device) for s in halves)
    note("bn_act_bwd.sums", fam, tc.rel_l2(bsums, r64["bwd_sums"].flatten()))
    assert tc.rel_l2(bsums, r64["bwd_sums"].flatten()) < tc.BAR_TENSOR
    dx = View(None, device, C + 4, 0, M, C)
    for s in halves:
        xs, ds, os_ = x.t[s], dy.t[s], dx.t[s]
        call("sfx_bn_act_bwd_apply", xs.shape[0], C, xs.data_ptr(), C + 3, mean.data_ptr(), rstd.data_ptr(),
             gamma.data_ptr(), beta.data_ptr(), act, ds.data_ptr(), C + 5, bsums.data_ptr(), float(M), os_.data_ptr(),
             C + 4, 0, stream())
    assert dx.padding_intact()
    _check_cols("bn_act_bwd.dx", fam, dx.t, r64["dx"], r32["dx"])
    dx1 = tops.bn_act_bwd(st, bn, act, dy.t)
    assert bool((tc.slice_err(dx.t, dx1, 0) <= tc.slice_bar(r32["dx"], r64["dx"], 0)).all())


# ---- segments ----------------------------------------------------------------------------------------------------
def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("layout", tc.SEGMENT_LAYOUTS)
@pytest.mark.parametrize("C", [1, 30, 64, 96, 128, 200, 256, 300, 512])
def test_segment_ops_ties_and_layouts(device, C, layout):
    """First maximum in run order (torch_scatter segment_csr) on exact duplicates whose first member in run order has
    the higher index, a constant column, -inf and signed zeros: y (bits) and arg exact, the gradient scattered whole
    to the arg row and nowhere else; segment_sum on a strided view; the eval pooling kernel gives the same maxima."""
    c = tc.segment_case(C, layout)
    n, m = c["n"], c["m"]
    ip = torch.tensor(c["idx_ptr"], dtype=torch.int32, device=device)
    si = torch.tensor(c["sidx"], dtype=torch.int32, device=device)
    y_ref, arg_ref = tr.segment_max_arg(c["x"], c["idx_ptr"], c["sidx"])
    x = c["x"].to(device)
    y, arg = tops.segment_max_arg(x, ip, si, m)
    assert torch.equal(arg.cpu().long(), arg_ref)
    assert torch.equal(bits(y), bits(y_ref))
    dx = tops.segment_max_bwd(c["dy"].to(device), arg, n)
    assert torch.equal(dx.cpu(), tr.segment_max_bwd(c["dy"], arg_ref, n))
    assert int((dx != 0).sum()) == int((c["dy"] != 0).sum())
    # eval consistency, bitwise: the eval kernel's unit affine (v * 1 + 0) turns a -0.0 maximum into +0.0 (IEEE), so
    # the training maxima go through the same fp32 affine before the bits are compared; the values are equal as is
    one, zero = torch.ones(C, device=device), torch.zeros(C, device=device)
    y_eval = ops.segment_max_affine_act(x, ip, si, m, one, zero, 0)
    assert torch.equal(y_eval, y)
    assert torch.equal(bits(y_eval), bits(y * one + zero))
    xs = View(c["xs"], device, C + 4)
    s = tops.segment_sum(xs.t, ip, si, m)
    e = tc.rel_l2(s, tr.segment_sum(c["xs"].double(), c["idx_ptr"], c["sidx"]))
    note("segment_sum", f"C={C},{layout}", e)
    assert e < tc.BAR_TIGHT


# ---- activation backward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [0, 3, 23])
@pytest.mark.parametrize("act", [1, 2, 3])
def test_act_bwd_acts_ncols_strides(device, act, ncols):
    c = tc.act_case(act)
    M, N = c["dy"].shape
    dy, pre = View(c["dy"], device, N + 1), View(c["pre"], device, N + 2, 1)
    out = View(None, device, N + 3, 0, M, N)
    tops.act_bwd(dy.t, pre.t, act, ncols=ncols, out=out.t)
    assert out.padding_intact()
    e = tc.rel_l2(out.t, tr.act_bwd(c["dy"].double(), c["pre"].double(), act, ncols))
    note("act_bwd", f"act={act},ncols={ncols}", e)
    assert e < tc.BAR_TIGHT
    assert torch.equal(bits(out.t[:, ncols:]), bits(c["dy"][:, ncols:]))
    if act == 2:  # ReLU' is 0 or 1: exact, +-0.0 arguments give 0
        assert torch.equal(out.t.cpu(), tr.act_bwd(c["dy"], c["pre"], 2, ncols))


# ---- gradient norm, clip coefficient -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", tc.SUMSQ_SIZES)
def test_sumsq_clip_coef_branches(device, n):
    """Three tensors accumulated (the last size runs the grid-stride loop past the 1024-block cap); the clipping
    branch, the coef = 1 branch (bit-exact) and the all-zero gradient."""
    grads = tc.grads_case(n)
    norm64 = float(tr.grad_norm([g.double() for g in grads]))
    dg = [g.to(device) for g in grads]
    for max_norm, clipped in ((f32(0.5 * norm64), True), (f32(2.0 * norm64), False)):
        coef, norm = tops.grad_clip_coef(dg, max_norm)
        e = abs(float(norm) - norm64) / norm64
        note("sumsq.norm", f"n={n}", e)
        assert e < tc.BAR_TIGHT
        if clipped:
            ref = float(tr.clip_coef(torch.tensor(norm64, dtype=D), max_norm))
            note("clip_coef", f"n={n}", abs(float(coef) - ref) / ref)
            assert abs(float(coef) - ref) / ref < tc.BAR_TIGHT and float(coef) < 1.0
        else:
            assert bits(coef).item() == bits(torch.ones(1)).item()
    coef, norm = tops.grad_clip_coef([torch.zeros_like(g) for g in dg], 2.0)
    assert float(coef) == 1.0 and float(norm) == 0.0


# ---- Adam ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_adam_step_options(device, n, wd):
    """p, exp_avg and exp_avg_sq after steps 1-3 and a step numbered 100 000, each against the fp64 restatement fed
    the fp32 state the kernel started from and the hyper-parameters as the float ABI carries them; lr = 0.1 so the
    update is of the parameter's size.  Exact-zero gradient elements stay finite with eps 1e-15; lr = 0 keeps the
    parameter's bits and still moves the moments."""
    c = tc.adam_case(n)
    lr, b1, b2, wdf = f32(0.1), f32(0.9), f32(0.999), f32(wd)
    for eps in (1e-15, 1e-8):
        for gscale in (None, 0.37):
            gs = None if gscale is None else torch.tensor([gscale], device=device)
            p = View(c["p"][None], device)
            m1, m2 = View(torch.zeros(1, n), device), View(torch.zeros(1, n), device)
            fam = f"n={n},wd={wd},eps={eps},scale={gscale}"
            for step, lr_now in ((1, lr), (2, lr), (3, lr), (100000, lr), (4, 0.0)):
                g = c["grads"][min(step, 4) - 1]
                before = [v.t[0].clone().cpu() for v in (p, m1, m2)]
                tops.adam_step(p.t[0], g.to(device), m1.t[0], m2.t[0], step, lr_now, betas=(b1, b2), eps=eps,
                               weight_decay=wdf, grad_scale=gs)
                ref = tr.adam_step(before[0].double(), g.double(), before[1].double(), before[2].double(), step,
                                   lr_now, b1, b2, f32(eps), wdf, None if gscale is None else f32(gscale))
                # the same step with the hyper-parameters in double (torch.optim's): reported, not asserted
                ref_t = tr.adam_step(before[0].double(), g.double(), before[1].double(), before[2].double(), step,
                                     0.1 if lr_now else 0.0, 0.9, 0.999, eps, wd, gscale)
                for name, v, r, rt in zip(("p", "exp_avg", "exp_avg_sq"), (p, m1, m2), ref, ref_t):
                    assert v.padding_intact()
                    assert bool(torch.isfinite(v.t).all())
                    e = tc.rel_l2(v.t[0], r)
                    note("adam." + name, f"wd={wd}", e)
                    note("adam." + name + "(vs double hyper-parameters)", f"wd={wd}", tc.rel_l2(v.t[0], rt))
                    assert e < tc.BAR_TIGHT, (fam, step, name, e)
                if lr_now == 0.0:
                    assert torch.equal(bits(p.t[0]), bits(before[0]))
                    assert not torch.equal(m1.t[0].cpu(), before[1])


# ---- drop mask, transpose ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257])
def test_drop_mask_small_sizes(device, n):
    out = View(None, device, None, 0, 1, n)
    call("sfx_drop_mask", n, 1.0, 99, out.t.data_ptr(), stream())
    assert out.padding_intact() and bool((out.t == 1.0).all())
    call("sfx_drop_mask", n, f32(0.7), 99, out.t.data_ptr(), stream())
    assert out.padding_intact()
    assert torch.equal(out.t[0], tops.drop_mask(n, 0.7, 99, device))
    assert set(torch.unique(out.t).tolist()) <= {0.0, float(torch.tensor(1.0) / torch.tensor(0.7))}


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 77), (77, 1), (31, 33), (32, 32), (33, 65), (1728, 64)])
def test_transpose_shapes_and_leading_dims(device, rows, cols):
    src = torch.randn(rows, cols, generator=tc.gen(8, rows, cols))
    assert torch.equal(bits(tops.transpose(src.to(device))), bits(src.T))
    s = View(src, device, cols + 3, 1)
    dst = View(None, device, rows + 5, 1, cols, rows)
    call("sfx_transpose", rows, cols, s.t.data_ptr(), cols + 3, dst.t.data_ptr(), rows + 5, stream())
    assert dst.padding_intact()
    assert torch.equal(bits(dst.t), bits(src.T))
