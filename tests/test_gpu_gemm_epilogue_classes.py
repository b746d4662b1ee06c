"""The specialised epilogue classes of csrc/gemm_kernel.h (EPI_LIN, EPI_LIN_GELU, EPI_PAIR_STORE) against the general
epilogue on the same launch: bitwise equality, via ops.gemm_force_epilogue(0).  (The accuracy of either against fp64
is test_gpu_gemm_epilogue.py's business, which runs the specialised classes wherever dispatch picks them.)

Every comparison runs the launch twice -- general forced, then automatic -- into sentinel-filled buffers wider and
taller than the result, checks with ops.gemm_last_epilogue() that the two launches ran the classes meant, and
compares the whole buffers bit for bit (so a store outside the result shows too).  Stream-K is forced off: its pieces
run the general epilogue by design.
"""
import pytest
import torch

from splatformer_amd import ptv3_ops as ops
from splatformer_amd.scenes import make_scene

pytestmark = pytest.mark.gpu

SENT = -12345.625
# gemm.hip kCfgs: (BM, BN, waves)
CFGS = [(128, 128, 4), (128, 96, 4), (128, 64, 4), (64, 128, 4), (64, 64, 4), (256, 128, 8), (128, 256, 8)]
CLASSES = {"lin": (ops.ACT_NONE, ops.EPI_LIN), "lin_gelu": (ops.ACT_GELU, ops.EPI_LIN_GELU)}
OPTIONS = ["bias", "affine", "residual", "amax", "all"]


def _slot_value(slot):
    """Largest value among the sub-slots of an amax slot (ops.new_amax ring) that carry its tag."""
    buf = next(st[0] for st in ops._amax_state.values()
               if st[0].data_ptr() <= slot[0] < st[0].data_ptr() + 8 * st[0].numel())
    off = (slot[0] - buf.data_ptr()) // 8
    w = buf[off:off + ops.AMAX_SUB].cpu()
    vals = [int(v) & 0xFFFFFFFF for v in w.tolist() if (int(v) >> 32) & 0xFFFFFFFF == slot[1]]
    return max(torch.tensor(vals, dtype=torch.int64).to(torch.int32).view(torch.float32).tolist()) if vals else 0.0


def _inputs(M, N, K, dev, seed):
    """Device operands with mixed row magnitudes (the per-row operand scales are live) and signed zeros in reach
    (a zero bias column: v + 0 residual handling must keep -0)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(M, K + 4, generator=g, device=dev)
    x[::3] *= 1e4
    x[1::7] *= 1e-5
    x[M // 2] = 0.0
    c = dict(x=x[:, :K], w=torch.randn(N, K, generator=g, device=dev) / K ** 0.5,
             bias=torch.randn(N, generator=g, device=dev), scale=torch.rand(N, generator=g, device=dev) + 0.5,
             shift=torch.randn(N, generator=g, device=dev), R=torch.randn(M + 2, N + 3, generator=g, device=dev))
    c["bias"][N // 2] = 0.0
    return c


def _run(c, M, N, act, opt, general):
    """One launch into a fresh sentinel buffer (strided Y, strided residual) -> (buffer, amax value or None, class)"""
    dev = c["x"].device
    buf = torch.full((M + 3, N + 5), SENT, device=dev)
    kw = dict(act=act, out=buf[:M, 2:2 + N])
    if opt in ("affine", "all"):
        kw.update(scale=c["scale"], shift=c["shift"])
    if opt in ("residual", "all"):
        kw["residual"] = c["R"][:M, 1:1 + N]
    if opt in ("amax", "all"):
        kw["y_amax"] = True
    ops.gemm_force_epilogue(0 if general else -1)
    res = ops.linear(c["x"], c["w"], c["bias"], **kw)
    cls = ops.gemm_last_epilogue()
    amax = _slot_value(res[1]) if isinstance(res, tuple) else None
    return buf, amax, cls


def _compare(c, M, N, act, want, opt, tag):
    try:
        ref, ra, rc = _run(c, M, N, act, opt, True)
        got, ga, gc = _run(c, M, N, act, opt, False)
    finally:
        ops.gemm_force_epilogue(-1)
    assert rc == ops.EPI_GENERAL and gc == want, (tag, rc, gc)
    assert torch.equal(ref.view(torch.int32), got.view(torch.int32)), tag
    assert bool((ref[M:] == SENT).all()) and bool((ref[:, :2] == SENT).all()) and bool((ref[:, 2 + N:] == SENT).all()), tag
    assert ra == ga, (tag, ra, ga)


@pytest.fixture
def no_stream_k():
    ops.gemm_force_config(-1, 0)
    yield
    ops.gemm_force_config(-1, -1)


@pytest.mark.parametrize("opt", OPTIONS)
@pytest.mark.parametrize("cls", list(CLASSES))
def test_class_equals_general(device, no_stream_k, cls, opt):
    """M in {1, 33, 261} x N in {23, 100, 288} x K in {64, 96, 544} (two, three and seventeen slabs)"""
    act, want = CLASSES[cls]
    for M in (1, 33, 261):
        for N in (23, 100, 288):
            for K in (64, 96, 544):
                c = _inputs(M, N, K, device, 1009 * M + 31 * N + K)
                _compare(c, M, N, act, want, opt, (cls, opt, M, N, K))


@pytest.mark.parametrize("cls", list(CLASSES))
def test_inplace_residual(device, no_stream_k, cls):
    """R == Y (the accumulate form): every residual load of a tile precedes its stores"""
    act, want = CLASSES[cls]
    M, N, K = 261, 100, 96
    c = _inputs(M, N, K, device, 5)
    outs = []
    try:
        for general in (True, False):
            y = c["R"][:M, 1:1 + N].clone()
            ops.gemm_force_epilogue(0 if general else -1)
            ops.linear(c["x"], c["w"], c["bias"], act=act, residual=y, out=y)
            assert ops.gemm_last_epilogue() == (ops.EPI_GENERAL if general else want)
            outs.append(y)
    finally:
        ops.gemm_force_epilogue(-1)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("cfg", list(range(ops.GEMM_NUM_CONFIGS)))
def test_every_tile_configuration(device, cfg):
    M, N, K = 261, 200, 96
    c = _inputs(M, N, K, device, 77 + cfg)
    try:
        ops.gemm_force_config(cfg, 0)
        for cls, (act, want) in CLASSES.items():
            _compare(c, M, N, act, want, "all", (cls, cfg))
    finally:
        ops.gemm_force_config(-1, -1)


@pytest.mark.parametrize("cfg", list(range(ops.GEMM_NUM_CONFIGS)))
def test_several_tiles_per_workgroup(device, cfg):
    """M = BM t + 5 with t ceil(N / BN) >= 2 x resident workgroups + 1: every workgroup walks three tiles, so the
    tile boundary (next tile's prefetch under this tile's stores) is exercised; K = 64 and 544."""
    bm, bn, nw = CFGS[cfg]
    N = 2048
    resident = torch.cuda.get_device_properties(device).multi_processor_count * (2 if nw == 4 else 1)
    tiles_n = -(-N // bn)
    t = -(-(2 * resident + 1) // tiles_n)
    M = bm * t + 5
    try:
        ops.gemm_force_config(cfg, 0)
        for K in (64, 544):
            c = _inputs(M, N, K, device, 900 + cfg + K)
            for cls, (act, want) in CLASSES.items():
                _compare(c, M, N, act, want, "all", (cls, cfg, M, K))
    finally:
        ops.gemm_force_config(-1, -1)


@pytest.fixture(scope="module")
def pair_map(device):
    """6000 seeded points on a coarse grid: duplicate voxels, most of the 27 neighbours present"""
    s = make_scene(6000, 1, seed=11, unique_voxels=False)
    grid = torch.floor(s["means"] * 10).int()
    assert grid.unique(dim=0).shape[0] < grid.shape[0]
    return grid


@pytest.mark.parametrize("n,C,cfg", [(6000, 64, -1), (6000, 256, 6), (1, 64, -1)])
def test_pair_store_equals_general(device, pair_map, n, C, cfg):
    grid = pair_map[:n].to(device)
    smap = ops.subm_neighbors(grid, None, centre=True)
    g = torch.Generator(device=device).manual_seed(C + n)
    x = torch.randn(n, C, generator=g, device=device)
    x[::3] *= 1e3
    w = torch.randn(C, 3, 3, 3, C, generator=g, device=device) * 0.05
    b = torch.randn(C, generator=g, device=device)
    parts = []
    try:
        ops.gemm_force_config(cfg, 0)
        for general in (True, False):
            ops.gemm_force_epilogue(0 if general else -1)
            sp = ops.subm_conv(x, smap, w, b, partials=True)
            assert ops.gemm_last_epilogue() == (ops.EPI_GENERAL if general else ops.EPI_PAIR_STORE)
            parts.append(sp)
    finally:
        ops.gemm_force_epilogue(-1)
        ops.gemm_force_config(-1, -1)
    assert parts[0].num_pairs == parts[1].num_pairs >= n
    if C == 256:  # the eight-wave 128 x 256 tile on more tiles than the device holds workgroups
        off = smap.lists(True).off_host
        tiles = sum(-(-(off[k + 1] - off[k]) // 128) for k in range(27))
        assert tiles > 256, tiles
    assert torch.equal(parts[0].partials.view(torch.int32), parts[1].partials.view(torch.int32))
    assert bool(torch.isfinite(parts[1].partials).all())
