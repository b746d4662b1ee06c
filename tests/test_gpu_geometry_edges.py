"""The refiner's integer geometry at its range and batch edges (GPU): the SubM neighbour map and its pair lists
against a brute-force dict reference that shares no key packing with the kernel (oracle/geometry_cases.py), the
fused conv's row order, serialization at depth 1 and 16 with batch indices up to 16383, pooling through a chain, and
the small index helpers of misc.hip / serialize.hip against numpy.  Every comparison is exact except segment_mean,
whose bound is derived from its fp32 operation count.

The cases are a few thousand points at most; each builder asserts that its points reach the edge it is named for."""
import numpy as np
import pytest
import torch

from oracle import geometry_cases as gc
from oracle import ptv3_ref, serialize_ref
from splatformer_amd import _lib
from splatformer_amd import ptv3_ops as ops
from splatformer_amd.ptv3_ops import call, ptr, stream

pytestmark = pytest.mark.gpu

_CASES = {c.name: c for c in gc.all_cases()}
ALL = list(_CASES)
TINY = [n for n in ALL if n.startswith("tiny")]
DENSE = ["dense_cube", "dense_cube[twice]"]
TWINS = "batched_twins[B=3]"
ORDER_BITS = (2, 6, 8, 18, 20, 24, 26, 1, 7, 9, 11, 15, 17, 23, 10, 12)  # csrc/subm_fused.hip kOrderBits, high -> low


def _dev(a, device, dtype=None):
    t = torch.from_numpy(np.array(a))  # (a copy: the cases' arrays are shared and read-only)
    return (t if dtype is None else t.to(dtype)).to(device)


def _gpu_map(c, device, batch="case"):
    b = c.batch if isinstance(batch, str) else batch
    return ops.subm_neighbors(_dev(c.grid, device), None if b is None else _dev(b, device), with_pairs=False)


# ---- SubM neighbour map -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_subm_map_equals_bruteforce(device, name):
    c = _CASES[name]
    nbr = _gpu_map(c, device).nbr.cpu().numpy()
    bad = np.argwhere(nbr != c.nbr)
    assert bad.shape[0] == 0, (f"{bad.shape[0]} entries differ; first (row, k) = {bad[0].tolist()}: kernel "
                               f"{nbr[tuple(bad[0])]} vs brute force {c.nbr[tuple(bad[0])]}, point "
                               f"{c.grid[bad[0][0]].tolist()} batch {int(c.batch0[bad[0][0]])}")
    if c.batch is None:  # batch = NULL is batch 0 everywhere
        zero = _gpu_map(c, device, np.zeros(c.n, np.int32)).nbr.cpu().numpy()
        assert np.array_equal(zero, nbr)


@pytest.mark.parametrize("name", ["range_corners", TWINS])
def test_subm_map_stays_inside_its_batch(device, name):
    c = _CASES[name]
    nbr = _gpu_map(c, device).nbr.cpu().numpy()
    rows, ks = np.nonzero(nbr >= 0)
    assert rows.size > c.n  # more than the centres: the case has real neighbours
    assert np.array_equal(c.batch[nbr[rows, ks]], c.batch[rows])
    g = c.grid.astype(np.int64)
    off = np.stack([ks // 9 - 1, (ks // 3) % 3 - 1, ks % 3 - 1], 1)
    assert np.array_equal(g[nbr[rows, ks]], g[rows] + off)  # and sits exactly one offset away


def test_subm_map_issue_example(device):
    """The four points that showed the carry of x + 1 = 65536 into the next key field."""
    grid = np.array([[5, 7, 65535], [5, 8, 0], [65535, 3, 3], [0, 3, 3]], np.int32)
    batch = np.array([0, 0, 0, 1], np.int32)
    nbr = ops.subm_neighbors(_dev(grid, device), _dev(batch, device), with_pairs=False).nbr.cpu().numpy()
    want = np.full((4, 27), -1, np.int64)
    want[np.arange(4), 13] = np.arange(4)
    assert np.array_equal(nbr, want)


# ---- pair lists -------------------------------------------------------------------------------------------------
SENT, TAIL = -7, 64


def _pair_buffers(n, centre, device):
    cap = (27 if centre else 26) * n  # the documented capacity, plus a sentinel tail nothing may touch
    pin = torch.full((cap + TAIL,), SENT, device=device, dtype=torch.int32)
    pout = torch.full((cap + TAIL,), SENT, device=device, dtype=torch.int32)
    off = torch.full((28,), SENT, device=device, dtype=torch.int32)
    pos = torch.full((n, 27), SENT, device=device, dtype=torch.int32)
    return cap, pin, pout, off, pos


def _check_lists(ref, cap, pin, pout, off, pos):
    torch.cuda.synchronize()
    npairs = int(ref["pair_off"][27])
    assert npairs <= cap
    assert np.array_equal(off.cpu().numpy(), ref["pair_off"])
    pin, pout = pin.cpu().numpy(), pout.cpu().numpy()
    assert np.array_equal(pin[:npairs], ref["pair_in"]) and np.array_equal(pout[:npairs], ref["pair_out"])
    assert (pin[npairs:] == SENT).all() and (pout[npairs:] == SENT).all()  # unused capacity and the tail
    assert np.array_equal(pos.cpu().numpy(), ref["pair_pos"])


@pytest.mark.parametrize("name", DENSE + [TWINS] + TINY)
@pytest.mark.parametrize("centre", [False, True])
def test_pair_lists_equal_reference(device, name, centre):
    c = _CASES[name]
    n = c.n
    ref = gc.pair_lists_ref(c.nbr, centre)
    nbr = _dev(c.nbr, device, torch.int32)  # the brute-force map: the lists are tested apart from the map kernel
    cap, pin, pout, off, pos = _pair_buffers(n, centre, device)
    cpos = torch.full((n, 32), SENT, device=device, dtype=torch.int32)
    ws = _lib.workspace(_lib.fn("sfx_subm_pair_lists_workspace_bytes")(n), device)
    call("sfx_subm_pair_lists", n, ptr(nbr), ptr(ws), ws.numel(), ptr(pin), ptr(pout), ptr(off), ptr(pos), ptr(cpos),
         1 if centre else 0, stream())
    _check_lists(ref, cap, pin, pout, off, pos)
    assert np.array_equal(cpos.cpu().numpy(), ref["cpos"])  # every row
    if name in DENSE:  # the rows that fill their capacity
        assert (ref["cpos"][c.info["interior"], 31] == (27 if centre else 26)).all()


@pytest.mark.parametrize("name", DENSE)
@pytest.mark.parametrize("centre", [False, True])
def test_flag_scan_pair_builder_equals_reference(device, name, centre):
    c = _CASES[name]
    n = c.n
    ref = gc.pair_lists_ref(c.nbr, centre)
    nbr = _dev(c.nbr, device, torch.int32)
    cap, pin, pout, off, pos = _pair_buffers(n, centre, device)
    ws = _lib.workspace(_lib.fn("sfx_subm_pairs_workspace_bytes")(n), device)
    call("sfx_subm_pairs", n, ptr(nbr), ptr(ws), ws.numel(), ptr(pin), ptr(pout), ptr(off), 1 if centre else 0,
         stream())
    call("sfx_subm_pair_pos", n, int(off[27].item()), ptr(pout), ptr(off), ptr(pos), stream())
    _check_lists(ref, cap, pin, pout, off, pos)


# ---- the fused conv's row order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", DENSE + TINY)
def test_subm_row_order(device, name):
    c = _CASES[name]
    order = _gpu_map(c, device).order.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(c.n))
    key = np.zeros(c.n, np.int64)
    for k in ORDER_BITS:
        key = (key << 1) | (c.nbr[:, k] >= 0)
    assert np.array_equal(order, np.argsort(key, kind="stable"))
    if name in DENSE:
        assert (key[c.info["interior"]] == 0xFFFF).all()


# ---- serialization ----------------------------------------------------------------------------------------------
def _check_serialize(device, grid, batch, depth, code_bits, orders):
    n = grid.shape[0]
    bt = None if batch is None else _dev(batch, device, torch.int32)
    codes, order, inverse = ops.serialize(_dev(grid, device, torch.int32), bt, depth, code_bits, orders)
    rb = np.zeros(n, np.int64) if batch is None else batch.astype(np.int64)
    c_ref, o_ref, i_ref, _ = serialize_ref.serialization(grid, rb, orders, None, depth=depth)
    assert codes.shape == (len(orders), n)
    assert np.array_equal(codes.cpu().numpy(), c_ref)
    assert np.array_equal(order.cpu().numpy(), o_ref)
    assert np.array_equal(inverse.cpu().numpy(), i_ref)
    return c_ref, o_ref, i_ref


def test_serialize_depth_one(device):
    c = _CASES["depth_one"]
    _check_serialize(device, c.grid, None, 1, 3, ptv3_ref.ORDERS)


def test_serialize_depth_sixteen_batch_16383(device):
    """code_bits = 48 + 14 = 62, the largest sfx_serialize_keys accepts: the order index takes the top two bits."""
    c = _CASES["range_corners"]
    assert int(c.batch.max()) == 16383 and int(c.grid.max()) == 65535
    c_ref, _, _ = _check_serialize(device, c.grid, c.batch, 16, 62, ptv3_ref.ORDERS)
    assert int(c_ref.max()).bit_length() == 62


@pytest.mark.parametrize("B", [3, 5])
def test_serialize_batched_twins(device, B):
    c = _CASES[TWINS] if B == 3 else gc.batched_twins(B=5)
    _check_serialize(device, c.grid, c.batch, c.depth, 3 * c.depth + (B - 1).bit_length(), ptv3_ref.ORDERS)


def test_serialize_one_point(device):
    grid = np.array([[65535, 0, 12345]], np.int32)
    _check_serialize(device, grid, None, 16, 48, ptv3_ref.ORDERS)


@pytest.mark.parametrize("orders", [("hilbert-trans",), ("hilbert", "z-trans"), ("z", "z-trans", "hilbert",
                                                                                  "hilbert-trans")])
def test_serialize_order_list_lengths(device, orders):
    c = _CASES[TWINS]
    _check_serialize(device, c.grid, c.batch, c.depth, 3 * c.depth + 2, list(orders))


# ---- pooling ----------------------------------------------------------------------------------------------------
def _point(device, c, perm):
    from splatformer_amd.ptv3 import Point
    B = int(c.batch.max()) + 1
    cb = 3 * c.depth + max(0, (B - 1).bit_length())
    grid, batch = _dev(c.grid, device), _dev(c.batch, device)
    codes, order, inverse = ops.serialize(grid, batch, c.depth, cb, ptv3_ref.ORDERS)
    c_ref, _, _, _ = serialize_ref.serialization(c.grid, c.batch.astype(np.int64), ptv3_ref.ORDERS, None,
                                                 depth=c.depth)
    pt = Point(coord=grid.float() * 0.25, grid_coord=grid, offset=np.cumsum(np.bincount(c.batch)).tolist(),
               codes_phys=codes, order_phys=order, inverse_phys=inverse, order_type=list(perm),
               serialized_depth=c.depth, code_bits=cb, batch=batch)
    return pt, torch.from_numpy(c_ref)[list(perm)]


def _pool_and_check(pt, code, grid, batch, perm, stride=2):
    """One SerializedPooling.geometry step against pooling_ref; `code` [4][n]: the reference codes in the parent's
    logical row order.  -> (pooled Point, its reference codes / grid / batch, m)."""
    from splatformer_amd.ptv3 import SerializedPooling
    pool = SerializedPooling(8, 8, stride=stride, norm_layer=torch.nn.BatchNorm1d, act_layer=torch.nn.GELU)
    new, sidx, idx_ptr, m = pool.geometry(pt, list(perm))
    r = gc.pooling_ref(code, stride, pt.serialized_depth)
    n = code.shape[1]
    assert m == len(r["counts"])
    assert torch.equal(new.pooling_inverse.cpu().long(), r["cluster"])
    assert torch.equal(idx_ptr.cpu().long(), r["ptr"])
    rows = new.order_type  # the pooled point's logical row q is the parent's logical row perm[q]
    assert torch.equal(new.codes_phys.cpu()[rows], r["code_h"][list(perm)])
    assert torch.equal(new.order_phys.cpu().long()[rows], r["order"][list(perm)])
    assert torch.equal(new.inverse_phys.cpu().long()[rows], r["inverse"][list(perm)])
    assert torch.equal(new.grid_coord.cpu(), grid[r["head"]] >> r["pd"])
    assert torch.equal(new.batch.cpu().long(), batch[r["head"]])
    assert new.offset == torch.cumsum(torch.bincount(batch[r["head"]], minlength=len(pt.offset)), 0).tolist()
    assert new.serialized_depth == pt.serialized_depth - r["pd"] and new.code_bits == pt.code_bits - 3 * r["pd"]
    seg = torch.repeat_interleave(torch.arange(m), r["counts"])
    assert torch.equal(torch.sort(seg * n + sidx.cpu().long()).values, seg * n + r["indices"])  # same members
    return new, r["code_h"][list(perm)], grid[r["head"]] >> r["pd"], batch[r["head"]], m


def test_pooling_range_corners(device):
    c = _CASES["range_corners"].sorted_by_batch()  # B = 3: batches 0, 1, 2
    assert int(c.batch.max()) == 2 and c.depth == 16
    perm = [2, 0, 3, 1]
    pt, code = _point(device, c, perm)
    new, _, _, _, m = _pool_and_check(pt, code, torch.from_numpy(c.grid), torch.from_numpy(c.batch).long(),
                                      [0, 1, 2, 3])
    assert int(new.grid_coord.max()) == 32767 and 0 < m < c.n


def test_pooling_chain_of_four(device):
    c = _CASES[TWINS].sorted_by_batch()
    assert c.depth == 5
    pt, code = _point(device, c, [1, 3, 0, 2])
    counts = ops.pool_counts_begin(pt.codes_phys, pt.order_phys, [3, 6, 9, 12])
    grid, batch = torch.from_numpy(c.grid), torch.from_numpy(c.batch).long()
    ms = []
    for perm in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 0, 3, 2], [2, 3, 0, 1]):
        pt, code, grid, batch, m = _pool_and_check(pt, code, grid, batch, perm)
        ms.append(m)
    assert pt.serialized_depth == 1 and ms == sorted(ms, reverse=True) and ms[-1] >= 3
    assert counts.get()[:4] == ms


# ---- index helpers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [[1], [255], [257], [0, 0, 1, 1, 1], [0, 100, 100, 255, 255],
                                     [0, 0, 3, 3, 3, 200, 257, 257], [128, 256, 257]])
def test_offsets_to_batch(device, offsets):
    n, B = offsets[-1], len(offsets)
    offs = torch.tensor(offsets, dtype=torch.int64, device=device)
    batch = torch.full((n + 8,), -7, device=device, dtype=torch.int32)
    call("sfx_offsets_to_batch", n, B, ptr(offs), ptr(batch), stream())
    ref = np.repeat(np.arange(B), np.diff(offsets, prepend=0))
    got = batch.cpu().numpy()
    assert np.array_equal(got[:n], ref) and (got[n:] == -7).all()


@pytest.mark.parametrize("dtype,cols", [(torch.int32, 1), (torch.float32, 3), (torch.int32, 27), (torch.float32, 32),
                                        (torch.int64, 1), (torch.int64, 16)])
@pytest.mark.parametrize("scatter", [False, True])
def test_move_rows(device, dtype, cols, scatter):
    """words = 1, 3, 27, 32 (4-byte elements) and 2, 32 (8-byte); source and destination are column slices of wider
    buffers whose other columns must keep their sentinel."""
    g = torch.Generator().manual_seed(cols + (100 if scatter else 0))
    ns = 257 if scatter else 100
    idx = torch.randperm(ns, generator=g) if scatter else torch.randint(0, ns, (300,), generator=g)
    nd = ns if scatter else idx.shape[0]
    hi = (1 << 62) if dtype == torch.int64 else (1 << 30)
    wide_src = torch.randint(-hi, hi, (ns, cols + 3), generator=g, dtype=torch.int64).to(dtype)
    wide_dst = torch.full((nd, cols + 5), -7, dtype=dtype)
    ref = wide_dst.clone()
    if scatter:
        ref[idx, 2:2 + cols] = wide_src[:, 1:1 + cols]
    else:
        ref[:, 2:2 + cols] = wide_src[idx, 1:1 + cols]
    ws, wd = wide_src.to(device), wide_dst.to(device)
    out = ops.move_rows(ws[:, 1:1 + cols], idx.int().to(device), wd[:, 2:2 + cols], scatter=scatter)
    assert out.data_ptr() == wd[:, 2:2 + cols].data_ptr()
    assert torch.equal(wd.cpu(), ref)
    if not scatter:  # a fresh contiguous destination, and a 1-D source
        assert torch.equal(ops.move_rows(ws[:, 1:1 + cols], idx.int().to(device)).cpu(), wide_src[idx, 1:1 + cols])
        col = ws[:, 0].contiguous()
        assert torch.equal(ops.move_rows(col, idx.int().to(device)).cpu(), wide_src[idx, 0])


@pytest.mark.parametrize("n", [1, 256, 70001])
def test_invert_permutation(device, n):
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).int()
    inv = torch.full((n + 8,), -7, device=device, dtype=torch.int32)
    call("sfx_invert_permutation", n, ptr(perm.to(device)), ptr(inv), stream())
    ref = np.empty(n, np.int32)
    ref[perm.numpy()] = np.arange(n, dtype=np.int32)
    got = inv.cpu().numpy()
    assert np.array_equal(got[:n], ref) and (got[n:] == -7).all()


def test_serialize_permute(device):
    """All five outputs of the renumbering by order row 0, from the reference serialization of batched_twins."""
    c = _CASES[TWINS]
    codes, order, inverse, _ = serialize_ref.serialization(c.grid, c.batch.astype(np.int64), ptv3_ref.ORDERS, None,
                                                           depth=c.depth)
    coord = (c.grid.astype(np.float32) + np.float32(0.5)) * np.float32(0.1)
    cp, op, ip, gp, xp = ops.serialize_permute(_dev(codes, device), _dev(order, device, torch.int32),
                                               _dev(inverse, device, torch.int32), _dev(c.grid, device),
                                               _dev(coord, device))
    j = order[0]
    assert np.array_equal(cp.cpu().numpy(), codes[:, j])
    assert np.array_equal(ip.cpu().numpy(), inverse[:, j])
    assert np.array_equal(op.cpu().numpy(), inverse[0][order])  # the new index of each row's i-th point
    assert np.array_equal(op[0].cpu().numpy(), np.arange(c.n))
    assert np.array_equal(gp.cpu().numpy(), c.grid[j])
    assert np.array_equal(xp.cpu().numpy().view(np.int32), coord[j].view(np.int32))


def test_segment_mean_derived_bound(device):
    """Runs of L = 1 .. 8 rows listed through a permuted sorted_idx, D = 3, against the fp64 mean.  The kernel adds L
    fp32 terms in list order (the first add, to 0, is exact) and divides once: at most L roundings of relative
    size 2^-24 on partial sums bounded by sum |x_j|, so |got - ref| <= (L + 1) 2^-24 (sum_j |x_j|) / L per element
    (one rounding of slack for the second-order terms)."""
    g = torch.Generator().manual_seed(5)
    lens = torch.arange(1, 9).repeat(63)[torch.randperm(504, generator=g)]
    n, m = int(lens.sum()), lens.shape[0]
    sidx = torch.randperm(n, generator=g)
    idx_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    x = torch.randn(n, 3, generator=g) * torch.exp2(torch.randint(-12, 13, (n, 1), generator=g).float())
    got = ops.segment_mean(x.to(device), idx_ptr.int().to(device), sidx.int().to(device), m).cpu().double()
    seg = torch.repeat_interleave(torch.arange(m), lens)
    xs = x[sidx].double()
    L = lens.double()[:, None]
    ref = torch.zeros(m, 3, dtype=torch.float64).index_add_(0, seg, xs) / L
    bound = (L + 1) * 2.0 ** -24 * torch.zeros(m, 3, dtype=torch.float64).index_add_(0, seg, xs.abs()) / L
    err = (got - ref).abs()
    print(f"segment_mean: max err / bound = {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(got[lens == 1].float(), x[sidx][idx_ptr[:-1][lens == 1]])  # a run of one row is a copy


@pytest.mark.parametrize("rest_dim,res,negative", [(0, 256.0, False), (9, 384.0, False), (45, 384.0, False),
                                                    (9, 256.0, True)])
def test_gs_pack(device, rest_dim, res, negative):
    """n = 3000: at 59 columns 177 000 elements, more than the 512 x 256 threads of one grid-stride pass.  Inputs
    are column slices of wider buffers; the means hold negative values and exact cell boundaries (k / 256)."""
    n = 3000
    g = torch.Generator().manual_seed(rest_dim + int(res))
    wide = torch.randn(n, 20, generator=g)
    means = wide[:, 1:4]
    means[::7] = torch.randint(-300, 600, (means[::7].shape[0], 3), generator=g).float() / 256.0  # cell boundaries
    if negative:
        means.copy_(-means.abs() - 0.001)
    gs = {"means": means, "scales": wide[:, 5:8], "opacities": wide[:, 9:10], "quats": wide[:, 10:14],
          "features_dc": wide[:, 15:18].reshape(n, 1, 3)}
    rest_wide = torch.randn(n, rest_dim // 3, 6, generator=g)
    if rest_dim:
        gs["features_rest"] = rest_wide[:, :, ::2]  # non-contiguous view
    assert not gs["means"].is_contiguous()
    W = 14 + rest_dim
    cpu_cols = [gs[k].reshape(n, -1) for k in ("means", "scales", "opacities", "quats", "features_dc")]
    if rest_dim:
        cpu_cols.append(gs["features_rest"].reshape(n, -1))
    want = torch.cat(cpu_cols, 1)
    assert want.shape == (n, W)
    wdev = wide.to(device)
    dgs = {"means": wdev[:, 1:4], "scales": wdev[:, 5:8], "opacities": wdev[:, 9:10], "quats": wdev[:, 10:14],
           "features_dc": wdev[:, 15:18].reshape(n, 1, 3)}
    if rest_dim:
        dgs["features_rest"] = rest_wide.to(device)[:, :, ::2]
        assert not dgs["features_rest"].is_contiguous()
    buf = torch.full((n, W + 5), -7.0, device=device)
    grid = torch.full((n, 3), -7, device=device, dtype=torch.int32)
    init = -5 if negative else 0
    gmax = torch.full((1,), init, device=device, dtype=torch.int32)
    ops.gs_pack(dgs, buf[:, 2:2 + W], res, grid, gmax)
    out = buf.cpu()
    assert torch.equal(out[:, 2:2 + W].view(torch.int32), want.contiguous().view(torch.int32))  # bit-equal columns
    assert bool((out[:, :2] == -7).all()) and bool((out[:, 2 + W:] == -7).all())
    gref = np.floor(means.numpy().astype(np.float32) * np.float32(res)).astype(np.int32)  # one exact fp32 multiply
    assert np.array_equal(grid.cpu().numpy(), gref)
    if res == 256.0 and not negative:  # k / 256 is exact: a point on a cell boundary belongs to the upper cell
        on = means.numpy()[::7].astype(np.float64) * 256.0
        assert (on == np.round(on)).all() and np.array_equal(gref[::7], on.astype(np.int32)) and (on < 0).any()
    if negative:
        assert gref.max() < 0 and int(gmax.item()) == init  # nothing to report: the initial value stays
    else:
        assert (gref < 0).any() and int(gmax.item()) == int(gref.max())
    # without grid outputs the features are packed alone
    buf2 = torch.full((n, W), -7.0, device=device)
    ops.gs_pack(dgs, buf2, res, None, None)
    assert torch.equal(buf2.cpu().view(torch.int32), want.contiguous().view(torch.int32))
