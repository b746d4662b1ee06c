"""Every epilogue option of sfx_linear / sfx_linear_bwd_data (include/sfx.h) on both store paths of
csrc/gemm_kernel.h -- the direct epilogue and the output-row-remapped one, their Stream-K partial forms, every
tile configuration and every operand form -- against oracle/linear_ref.py in fp64.

The bar is the project's single-GEMM bar (test_linear_narrow_cases): for every output row,
    |y_hip - y64| / |y64|  <=  2 |y_f32 - y64| / |y64| + 1e-7,
y_f32 being the same reference function evaluated by torch on the CPU in fp32; it applies to Y, Ypre and dX.
On top of it, exactly: nothing outside the result is written (buffers are wider and taller than the result and
pre-filled with a sentinel), a DropPath-dropped row equals its residual row bit for bit, and a y_amax slot
bounds max |Y| from above.

Shapes are the smallest at which each mechanism can break: M in {1, 33, 261} (one row; one 32-row MFMA block
+ 1; two 128-row tiles + 5), N in {23, 100, 200} (odd and under one block; ragged; two N tiles of every width
but 256), K in {23, 24, 96, 544} (scalar loads; vector exact fp32; fp16x2; 17 slabs, where Stream-K is legal).
Operand rows carry mixed magnitudes (x1e4, x1e-5) so the per-row operand scales are live.  Every case prints its
worst ratio e_hip / (2 e_f32 + 1e-7) before asserting it <= 1.
"""
import functools

import pytest
import torch

from oracle import linear_ref as lr
from splatformer_amd import _lib
from splatformer_amd import ptv3_ops as ops
from splatformer_amd import train_ops as tops

pytestmark = pytest.mark.gpu

SENT = -12345.625  # sentinel of every output buffer (exact in fp32, far from every result)


def _slot_value(slot):
    """Largest value among the sub-slots of an amax slot (ops.new_amax ring) that carry its tag."""
    buf = next(st[0] for st in ops._amax_state.values()
               if st[0].data_ptr() <= slot[0] < st[0].data_ptr() + 8 * st[0].numel())
    off = (slot[0] - buf.data_ptr()) // 8
    w = buf[off:off + ops.AMAX_SUB].cpu()
    vals = [int(v) & 0xFFFFFFFF for v in w.tolist() if (int(v) >> 32) & 0xFFFFFFFF == slot[1]]
    return max(torch.tensor(vals, dtype=torch.int64).to(torch.int32).view(torch.float32).tolist()) if vals else 0.0


def _bar(name, got, ref64, ref32):
    """The per-row bar; prints the worst ratio, then asserts."""
    got, ref32 = got.double(), ref32.double()
    rn = ref64.norm(dim=1).clamp_min(1e-30)
    e_hip, e_f32 = (got - ref64).norm(dim=1) / rn, (ref32 - ref64).norm(dim=1) / rn
    ratio = e_hip / (2 * e_f32 + 1e-7)
    worst = int(ratio.argmax())
    print(f"[epilogue] {name}: worst e_hip/(2 e_f32+1e-7) = {float(ratio[worst]):.3f} (row {worst}: "
          f"{float(e_hip[worst]):.2e} vs fp32 {float(e_f32[worst]):.2e})")
    assert bool(torch.isfinite(got).all()), name
    assert bool((e_hip <= 2 * e_f32 + 1e-7).all()), (name, worst, float(e_hip[worst]), float(e_f32[worst]))


def _mixed(g, rows, cols, big=1e4):
    t = torch.randn(rows, cols, generator=g)
    t[::3] *= big
    t[1::7] *= 1e-5
    return t


def _mask(g, n, keep=0.7):
    """DropPath keep mask / keep with at least one dropped and (n > 1) one kept row."""
    m = (torch.rand(n, generator=g) < keep).float() / keep
    m[n // 2] = 0.0
    if n > 1:
        m[0] = 1.0 / keep
    return m


@functools.lru_cache(maxsize=None)
def _case(M, N, K, act=0, act_ncols=-1, bias=True, affine=False, rowscale=False, residual=False, short_r=False,
          pre=None, remap=False, gather=False, lda_extra=0, big_bias=False, big=1e4):
    """CPU tensors of one sfx_linear case and its fp64 / fp32 references (computed once, never modified).
    pre: None | "before" | "after";  remap: shuffled injection of the GEMM rows into T = M + 9 output rows with
    some -1 entries;  gather: one-segment gather_idx (some -1 = empty rows);  short_r: residual rows picked through
    residual_idx from a shorter R;  big_bias: |bias| above every |Y| (ragged-M amax question);  big: the factor of
    the large operand rows."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + 7 * K + 31 * act + (act_ncols + 1) + 2 * affine +
                                      4 * rowscale + 8 * remap + 16 * gather)
    c = dict(M=M, N=N, K=K, act=act, act_ncols=act_ncols, pre=pre, lda=K + 8 + lda_extra)
    src_rows = M + 5 if gather else M
    xb = 0.1 * torch.randn(src_rows, c["lda"], generator=g) if big_bias else _mixed(g, src_rows, c["lda"], big)
    c["xb"] = xb
    x = xb[:, 4:4 + K]
    c["gidx"] = None
    A = x
    if gather:
        gi = torch.randint(0, src_rows, (M, 1), generator=g, dtype=torch.int32)
        gi[M // 3] = -1
        c["gidx"] = gi
        A = torch.where(gi >= 0, x[gi.flatten().clamp_min(0).long()], torch.zeros(()))
    c["w"] = torch.randn(N, K, generator=g) / K ** 0.5
    c["bias"] = (torch.randn(N, generator=g) if not big_bias else 50.0 + torch.rand(N, generator=g)) if bias else None
    c["scale"] = torch.rand(N, generator=g) + 0.5 if affine else None
    c["shift"] = torch.randn(N, generator=g) if affine else None
    T = M + 9 if remap else M
    c["T"] = T
    c["rows"] = None
    if remap:
        rows = torch.randperm(T, generator=g)[:M].int()
        rows[::5] = -1
        c["rows"] = rows
    c["rowscale"] = _mask(g, T) if rowscale else None
    if rowscale and remap:  # a written row that is dropped, and its neighbour kept
        named = rows[rows >= 0]
        c["rowscale"][named[0]] = 0.0
        c["rowscale"][named[1]] = 1.0 / 0.7
    c["Rb"], c["ridx"] = None, None
    R = None
    if residual:
        rr = max(2, T // 3) if short_r else T
        if big_bias:  # cancels the padding rows' value bias * scale + shift
            pad = c["bias"] * c["scale"] + c["shift"] if affine else c["bias"]
            c["Rb"] = -pad.repeat(rr, 1) + 0.1 * torch.randn(rr, N, generator=g)
            c["Rb"] = torch.cat([torch.zeros(rr, 1), c["Rb"], torch.zeros(rr, 2)], 1)
        else:
            c["Rb"] = torch.randn(rr, N + 3, generator=g)
        R = c["Rb"][:, 1:1 + N]
        if short_r:
            c["ridx"] = torch.randint(0, rr, (T,), generator=g, dtype=torch.int32)
    kw = dict(act=act, act_ncols=act_ncols, rowscale=c["rowscale"], R=R, residual_idx=c["ridx"], out_rows=c["rows"],
              n_out_rows=T, pre_before_act=pre == "before")
    c["ref64"] = lr.linear_epilogue(A.double(), c["w"], c["bias"], c["scale"], c["shift"], **kw)
    c["ref32"] = lr.linear_epilogue(A, c["w"], c["bias"], c["scale"], c["shift"], **kw)
    return c


def _run(device, name, M, N, K, y_amax=False, raw_bf16x3=False, **spec):
    """Launch one case on the GPU (ops.linear, or the C ABI directly without a pre-split weight -> bf16x3) and
    check Y / Ypre against the references, the sentinels, the dropped rows and the amax slot.  Returns
    (published amax or None, max |Y| of the written rows)."""
    c = _case(M, N, K, **spec)
    T = c["T"]
    d = lambda t: None if t is None else t.to(device)
    xb = d(c["xb"])
    x = xb[:, 4:4 + K]
    w, b, sc, sh = d(c["w"]), d(c["bias"]), d(c["scale"]), d(c["shift"])
    Rb, ridx, rows, rs, gi = d(c["Rb"]), d(c["ridx"]), d(c["rows"]), d(c["rowscale"]), d(c["gidx"])
    R = None if Rb is None else Rb[:, 1:1 + N]
    ybuf = torch.full((T + 3, N + 5), SENT, device=device)
    pbuf = torch.full((T + 2, N + 7), SENT, device=device) if c["pre"] else None
    y = ybuf[:T, :N]
    p = None if pbuf is None else pbuf[:T, :N]
    slot = None
    if raw_bf16x3:
        assert gi is None and K % 4 == 0 and K >= ops.SPLIT_MIN_K and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
        slot = ops.new_amax(device) if y_amax else None
        _lib.call("sfx_linear", M, N, K, x.data_ptr(), x.stride(0), None, 1, w.data_ptr(), w.stride(0),
                  _lib.ptr(b), _lib.ptr(sc), _lib.ptr(sh), c["act"], c["act_ncols"],
                  None if R is None else R.data_ptr(), 0 if R is None else R.stride(0), _lib.ptr(ridx),
                  y.data_ptr(), y.stride(0), None if p is None else p.data_ptr(), 0 if p is None else p.stride(0),
                  1, 0, 0, 0, 0, _lib.ptr(rows), _lib.ptr(rs), 1 if c["pre"] == "before" else 0, None, 0, None, 0,
                  *(slot or (None, 0)), None, None, _lib.stream())
    else:
        r = ops.linear(x, w, b, act=c["act"], act_ncols=c["act_ncols"], scale=sc, shift=sh, residual=R,
                       residual_idx=ridx, out=y, pre_out=p, gather_idx=gi, out_rows=rows, rowscale=rs,
                       pre_before_act=c["pre"] == "before", y_amax=y_amax)
        if y_amax:
            slot = r[1]
    yh = ybuf.cpu()
    ref64, ref32 = c["ref64"], c["ref32"]
    written = ~torch.isnan(ref64[0][:, 0])
    assert int(written.sum()) == (M if c["rows"] is None else int((c["rows"] >= 0).sum()))
    for nm, buf, r64, r32 in (("Y", yh, ref64[0], ref32[0]),) + \
            ((("Ypre", pbuf.cpu(), ref64[1], ref32[1]),) if pbuf is not None else ()):
        assert bool((buf[T:] == SENT).all()), f"{name} {nm}: rows >= the result were written"
        assert bool((buf[:, N:] == SENT).all()), f"{name} {nm}: columns >= N were written"
        assert bool((buf[:T, :N][~written] == SENT).all()), f"{name} {nm}: unnamed / dropped (-1) rows were written"
        _bar(f"{name} {nm}", buf[:T, :N][written], r64[written], r32[written])
    got = yh[:T, :N]
    if c["rowscale"] is not None:  # DropPath: a dropped row is its residual row, bit for bit
        drop = written & (c["rowscale"] == 0)
        assert int(drop.sum()) > 0
        o = torch.nonzero(drop).flatten()
        if c["Rb"] is None:
            want = torch.zeros(o.numel(), N)
        else:
            want = c["Rb"][:, 1:1 + N][c["ridx"][o].long() if c["ridx"] is not None else o]
        assert torch.equal(got[o], want), f"{name}: dropped rows differ from their residual rows"
    ymax = float(got[written].abs().max())
    if slot is None:
        return None, ymax
    amax = _slot_value(slot)
    print(f"[epilogue] {name}: y_amax slot {amax:.6g}, max|Y| {ymax:.6g}, equal to 1e-6: "
          f"{abs(amax - ymax) <= 1e-6 * ymax}")
    assert amax >= ymax, f"{name}: y_amax slot {amax} below max |Y| {ymax}"
    return amax, ymax


# ---- a. option semantics under the cost model's configuration ------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 23, 23), (33, 100, 96), (261, 200, 24), (261, 23, 544)])
def test_droppath_rowscale_residual(device, M, N, K):
    """ptv3_train.py's proj / fc2 call: Y = rowscale * (A W^T + b) + R, Bernoulli / keep rows with zeros."""
    _run(device, f"droppath {M}x{N}x{K}", M, N, K, rowscale=True, residual=True)
    # with an activation in front: rowscale multiplies act(z), not z
    _run(device, f"droppath tanh {M}x{N}x{K}", M, N, K, act=ops.ACT_TANH, act_ncols=N // 2, rowscale=True,
         residual=True, pre="after")


@pytest.mark.parametrize("M,N,K", [(33, 200, 24), (261, 100, 96), (1, 100, 544), (33, 23, 23)])
def test_gelu_pre_before_act(device, M, N, K):
    """fc1 of the training MLP: Y = GELU(z), Ypre = z saved for the backward (pre_before_act = 1)."""
    _run(device, f"gelu+pre {M}x{N}x{K}", M, N, K, act=ops.ACT_GELU, pre="before")


@pytest.mark.parametrize("M,N,K", [(261, 200, 96), (33, 23, 23), (261, 100, 544), (1, 200, 24)])
def test_unpooling_pre_after_act_residual_idx(device, M, N, K):
    """SerializedUnpooling's call: Y = GELU((A W^T + b) * scale + shift) + coarse[inverse] with a shorter coarse,
    Ypre = the skip value after the activation and before the residual (pre_before_act = 0)."""
    _run(device, f"unpool {M}x{N}x{K}", M, N, K, act=ops.ACT_GELU, affine=True, residual=True, short_r=True,
         pre="after")


@pytest.mark.parametrize("act", [ops.ACT_TANH, ops.ACT_RELU])
@pytest.mark.parametrize("M,N,K", [(33, 23, 96), (261, 100, 24)])
def test_head_partial_activation(device, act, M, N, K):
    """The heads' call: tanh / ReLU on the first act_ncols columns only, act_ncols in {0, 3, N // 2, N}, with
    pre_out and a residual.  Ypre is the activation's output for tanh (what its backward takes) and the
    pre-activation for ReLU.

    Full-width tanh is the one call whose output does not scale with its input row: at x1e4 every |Y| is <= 1 + |R|
    while |dz| ~ 1e4 eps, so a row's error is that of its one or two elements with z near 0 -- a single draw on
    each side (measured: e_hip 3.1e-5 against e_f32 1.5e-6 on one row of (261, 100, 24), z itself within the bar),
    which the per-row bar cannot compare.  That call keeps the mixed magnitudes with large rows of x4 (row scales
    2^2 against 2^-17), where the rounding of z stays spread over the row."""
    for nc in (0, 3, N // 2, N):
        big = 4.0 if (act == ops.ACT_TANH and nc == N) else 1e4
        _run(device, f"head act{act} ncols{nc} {M}x{N}x{K}", M, N, K, act=act, act_ncols=nc, residual=True,
             pre="after" if act == ops.ACT_TANH else "before", big=big)


@pytest.mark.parametrize("gather", [False, True], ids=["dense", "gather"])
@pytest.mark.parametrize("M,N,K", [(261, 100, 96), (33, 23, 24), (261, 200, 544)])
def test_out_rows_remapped_epilogue(device, gather, M, N, K):
    """out_row_idx: a shuffled injection of the GEMM rows into a taller buffer, some rows dropped (-1), with
    rowscale and residual_idx read at the OUTPUT row, Ypre and a y_amax slot -- the remapped epilogue, which no
    caller of the package reaches in dense mode; also through a one-segment gather_idx."""
    _run(device, f"out_rows {'gather' if gather else 'dense'} {M}x{N}x{K}", M, N, K, y_amax=True, act=ops.ACT_GELU,
         affine=True, rowscale=True, residual=True, short_r=True, pre="after", remap=True, gather=gather)


# ---- b. operand forms ------------------------------------------------------------------------------------------
_FORMS = {  # form -> (M, N, K, lda_extra, raw_bf16x3)
    "scalar_k23": (33, 23, 23, 0, False),
    "scalar_k96_odd_lda": (261, 100, 96, 1, False),
    "vector_fp32_k24": (261, 200, 24, 0, False),
    "fp16x2_k96": (33, 100, 96, 0, False),
    "bf16x3_k96": (261, 23, 96, 0, True),
    "bf16x3_k544": (33, 200, 544, 0, True),
}


@pytest.mark.parametrize("form", list(_FORMS))
def test_operand_forms(device, form):
    """The unpooling-shaped and the DropPath-shaped call in every operand form: scalar fp32 loads (K = 23; K = 96
    with an odd lda), vector exact fp32 (K = 24), fp16x2 (K = 96, pre-split weight) and bf16x3 (the C ABI called
    without w_split / w_inv, which ops.linear never does)."""
    M, N, K, extra, raw = _FORMS[form]
    _run(device, f"{form} unpool", M, N, K, raw_bf16x3=raw, lda_extra=extra, act=ops.ACT_GELU, affine=True,
         residual=True, short_r=True, pre="after")
    _run(device, f"{form} droppath", M, N, K, raw_bf16x3=raw, lda_extra=extra, rowscale=True, residual=True)
    _run(device, f"{form} gelu+pre", M, N, K, raw_bf16x3=raw, lda_extra=extra, act=ops.ACT_GELU, pre="before")


# ---- e. sfx_linear_bwd_data -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bwd_case(M, N, K, dact, ncols):
    """dX [M, K] = (base +) rowscale * (dY [M, N] W [N, K]) * act'(pre) on columns < ncols: CPU tensors and the
    fp64 / fp32 references with and without the accumulated-into base."""
    g = torch.Generator().manual_seed(7919 * M + 131 * N + 17 * K + 5 * dact + ncols + 1)
    c = dict(dyb=_mixed(g, M, N + 8), W=torch.randn(N, K, generator=g) / N ** 0.5, rs=_mask(g, M),
             preb=torch.randn(M, K + 5, generator=g), base=torch.randn(M, K, generator=g))
    if dact == tops.DACT_TANH_OUT:
        c["preb"] = torch.tanh(c["preb"])
    dy, pre = c["dyb"][:, 4:4 + N], c["preb"][:, 2:2 + K]
    for acc in (0, 1):
        base = c["base"] if acc else None
        c["ref64", acc] = lr.linear_bwd_data(dy.double(), c["W"], c["rs"], dact, ncols, pre if dact else None, base)
        c["ref32", acc] = lr.linear_bwd_data(dy, c["W"], c["rs"], dact, ncols, pre if dact else None, base)
    return c


def _run_bwd(device, name, M, N, K, dact, ncols, acc):
    c = _bwd_case(M, N, K, dact, ncols)
    dyb, preb = c["dyb"].to(device), c["preb"].to(device)
    wt = c["W"].T.contiguous().to(device)
    xbuf = torch.full((M + 2, K + 6), SENT, device=device)
    dx = xbuf[:M, 3:3 + K]
    if acc:
        dx.copy_(c["base"].to(device))
    tops.linear_bwd_data(dyb[:, 4:4 + N], wt, rowscale=c["rs"].to(device), dact=dact, dact_ncols=ncols,
                         dact_pre=preb[:, 2:2 + K] if dact else None, out=dx, accumulate=bool(acc))
    xh = xbuf.cpu()
    assert bool((xh[M:] == SENT).all()) and bool((xh[:, :3] == SENT).all()) and bool((xh[:, 3 + K:] == SENT).all()), \
        f"{name}: dX written outside its [M, K] window"
    got = xh[:M, 3:3 + K]
    _bar(name, got, c["ref64", acc], c["ref32", acc])
    drop = c["rs"] == 0
    assert torch.equal(got[drop], c["base"][drop] if acc else torch.zeros(int(drop.sum()), K)), \
        f"{name}: dropped rows must keep the accumulated-into value (or be zero)"


@pytest.mark.parametrize("dact", [tops.DACT_GELU, tops.DACT_RELU, tops.DACT_TANH_OUT])
@pytest.mark.parametrize("M,N,K", [(33, 23, 100), (261, 96, 200)])
def test_linear_bwd_data_options(device, dact, M, N, K):
    """dact in {GELU on the pre-activation, ReLU, tanh given its output} x dact_ncols in {-1, 0, 3, K} x
    accumulate in {0, 1}, with rowscale; dY of N = 23 columns (scalar path) and N = 96 (fp16x2); dX and dact_pre
    are column slices of wider buffers."""
    for ncols in (-1, 0, 3, K):
        for acc in (0, 1):
            _run_bwd(device, f"bwd_data dact{dact} ncols{ncols} acc{acc} {M}x{N}x{K}", M, N, K, dact, ncols, acc)


# ---- c. every tile configuration x Stream-K ---------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(range(ops.GEMM_NUM_CONFIGS)))
def test_every_tile_config_epilogue_options(device, cfg):
    """Every tile configuration (the eight-wave ones included: K >= 64 and vector-aligned, so the forced
    configuration is really used) x Stream-K forced off / on: the three shaped calls at (261, 200, 96); at
    (261, 200, 544), where Stream-K is legal, bias + scale / shift + rowscale + residual through residual_idx into
    a strided Y (dropped rows still equal their residual rows bit for bit when the tile is summed from atomic
    pieces) and sfx_linear_bwd_data with accumulate = 0, rowscale, GELU dact on 150 of 200 columns into a strided
    dX."""
    try:
        for sk in (0, 1):
            ops.gemm_force_config(cfg, sk)
            tag = f"cfg{cfg} sk{sk}"
            _run(device, f"{tag} droppath", 261, 200, 96, rowscale=True, residual=True)
            _run(device, f"{tag} gelu+pre", 261, 200, 96, act=ops.ACT_GELU, pre="before")
            _run(device, f"{tag} unpool", 261, 200, 96, act=ops.ACT_GELU, affine=True, residual=True, short_r=True,
                 pre="after")
            _run(device, f"{tag} streamk affine+rowscale+ridx", 261, 200, 544, affine=True, rowscale=True,
                 residual=True, short_r=True)
            _run_bwd(device, f"{tag} streamk bwd_data", 261, 544, 200, tops.DACT_GELU, 150, 0)
    finally:
        ops.gemm_force_config(-1, -1)


# ---- d. grouped -----------------------------------------------------------------------------------------------
def test_grouped_linear_relu_amax(device):
    """ops.grouped_linear (the block-diagonal head layers): G = 3 groups of N = 40 outputs over K = 128 inputs,
    ReLU, M = 261, a y_amax slot, against the fp64 block-diagonal product; the output is a column slice of a
    wider, taller buffer."""
    g = torch.Generator().manual_seed(40)
    M, G, N, K = 261, 3, 40, 128
    x = _mixed(g, M, G * K)
    w = torch.randn(G, N, K, generator=g) / K ** 0.5
    b = torch.randn(G, N, generator=g)
    ref64 = lr.linear_epilogue(x.double(), w, b, act=lr.ACT_RELU, groups=G)[0]
    ref32 = lr.linear_epilogue(x, w, b, act=lr.ACT_RELU, groups=G)[0]
    ybuf = torch.full((M + 3, G * N + 4), SENT, device=device)
    _, slot = ops.grouped_linear(x.to(device), w.to(device), b.to(device), G, act=ops.ACT_RELU, out=ybuf[:M, :G * N],
                                 y_amax=True)
    yh = ybuf.cpu()
    assert bool((yh[M:] == SENT).all()) and bool((yh[:, G * N:] == SENT).all())
    _bar("grouped relu", yh[:M, :G * N], ref64, ref32)
    amax, ymax = _slot_value(slot), float(yh[:M, :G * N].abs().max())
    print(f"[epilogue] grouped relu: y_amax slot {amax:.6g}, max|Y| {ymax:.6g}")
    assert amax >= ymax


# ---- the amax slot with ragged M ---------------------------------------------------------------------------------
@pytest.mark.parametrize("remap", [False, True], ids=["direct", "remapped"])
def test_amax_slot_ragged_rows_big_bias(device, remap):
    """include/sfx.h: y_amax receives an upper bound of max |Y|; a tile's padding rows (rows >= M of the last
    tile) may contribute act(bias * scale + shift).  With M = 33 (31 padding rows in every tile shape), a bias of
    ~50 and a residual that cancels it (|Y| < 1), the slot must bound max |Y| from above and stay within the
    documented contribution max |bias * scale + shift|.  Measured on the MI355X: the direct epilogue publishes
    the padding rows' value (slot 75.6 against max |Y| 0.56 -- not equal); the remapped epilogue masks them
    (equal to 1e-6)."""
    M, N, K = 33, 100, 96
    spec = dict(affine=True, residual=True, big_bias=True, remap=remap)
    amax, ymax = _run(device, f"amax big bias {'remapped' if remap else 'direct'}", M, N, K, y_amax=True, **spec)
    c = _case(M, N, K, **spec)
    pad = float((c["bias"].double() * c["scale"].double() + c["shift"].double()).abs().max())
    assert ymax < 2.0 < pad
    assert ymax <= amax <= max(ymax, pad) * (1 + 1e-6), (amax, ymax, pad)
