"""Fused Block MLP (csrc/mlp.hip) at the edges of its epilogue and prologue: the residual rows are loaded in one
run, finished in place of the accumulators and stored in one run, the parameter table is copied with 16-byte loads
and the weight ring is never drained by the compiler.  None of that may change what a lane loads or stores: ragged
point counts around the workgroup's point count, strided input and output with sentinels, in-place output,
run-to-run equal bits, every forced launch kind, and the training kinds.

The bar is test_gpu_mlp.py's (test_block_mlp_matches_fp64): relative L2 of the branch <= max(2e-6, 2 x torch fp32's
own error) against fp64, each row within 4 x its fp32 error + 1e-6, inputs with rows scaled by 1e3 and 1e-3."""
import functools

import pytest
import torch
import torch.nn.functional as F

from splatformer_amd import ptv3_ops as ops
from test_gpu_mlp import SPLIT_CASES, _mods, _ref
from test_gpu_ptv3 import rel_l2

pytestmark = pytest.mark.gpu

CHANNELS = ops.MLP_CHANNELS


@functools.lru_cache(maxsize=None)
def _case(C, M):
    """(modules on the CPU, x, fp64 reference, fp32 reference): computed once per shape, never modified"""
    ln, fc1, fc2 = _mods(C, C + M)
    x = torch.randn(M, C, generator=torch.Generator().manual_seed(M)) * 2.0
    x[::3] *= 1e3
    x[1::5] *= 1e-3
    return (ln, fc1, fc2), x, _ref(x, ln, fc1, fc2, torch.float64), _ref(x, ln, fc1, fc2, torch.float32).double()


def _dev_mods(C, M, device):
    import copy
    return [copy.deepcopy(m).to(device) for m in _case(C, M)[0]]


def _assert_bar(C, M, y):
    _, x, ref, r32 = _case(C, M)
    y = y.detach().cpu().double()
    assert torch.isfinite(y).all()
    br, bh, b32 = ref - x.double(), y - x.double(), r32 - x.double()
    e, e32 = rel_l2(bh, br), rel_l2(b32, br)
    print(f"C={C} M={M}: rel-L2 {e:.3e} (fp32 {e32:.3e})")
    assert e <= max(2e-6, 2 * e32), (e, e32)
    e_row = (bh - br).norm(dim=1) / br.norm(dim=1).clamp_min(1e-30)
    r_row = (b32 - br).norm(dim=1) / br.norm(dim=1).clamp_min(1e-30)
    assert bool((e_row <= 4 * r_row + 1e-6).all()), float((e_row - 4 * r_row).max())


def _ragged(pts):
    return [1, 31, 33, pts - 1, pts + 1, 2 * pts + 1]


def _run_ragged(device, C, pts, check_plan):
    """every ragged count of a pts-point workgroup at the fp64 bar, into rows [0, M) of a buffer whose rows past M
    hold a sentinel (a lane past M stores nothing)"""
    for M in _ragged(pts):
        mods = _dev_mods(C, M, device)
        x = _case(C, M)[1].to(device)
        buf = torch.full((M + 3, C), -7.25, device=device)
        ops.block_mlp(x, *mods, out=buf[:M])
        if check_plan:
            assert ops.block_mlp_last_plan()["pts"] == pts
        assert bool((buf[M:] == -7.25).all()), M
        _assert_bar(C, M, buf[:M])


@pytest.mark.parametrize("C", CHANNELS)
def test_ragged_point_counts(device, C):
    pts = 128
    if C >= 128:  # the plan picks the tile kind: its point count for a launch this small
        mods = _dev_mods(C, 33, device)
        ops.block_mlp(_case(C, 33)[1].to(device), *mods)
        pts = ops.block_mlp_last_plan()["pts"]
        assert pts in (64, 128)
    _run_ragged(device, C, pts, C >= 128)


@pytest.mark.parametrize("C,env,pts", [(128, ("SFX_MLP_HS", "0"), 128), (128, ("SFX_MLP_HS", "1"), 64),
                                       (256, ("SFX_MLP_HS", "0"), 128), (256, ("SFX_MLP_HS", "1"), 64),
                                       (64, ("SFX_MLP_WAVES", "8"), 256), (96, ("SFX_MLP_WAVES", "8"), 256),
                                       (128, ("SFX_MLP_WAVES", "8"), 256)])
def test_forced_kinds_ragged(device, monkeypatch, C, env, pts):
    """whole tiles / hidden-split tiles at C = 128 and 256, 256-point workgroups at C <= 128, at their ragged counts"""
    monkeypatch.setenv(*env)
    _run_ragged(device, C, pts, True)


@pytest.mark.parametrize("C", CHANNELS)
def test_strided_input_and_output(device, C):
    """X a column slice of a wider buffer, Y a column slice of another with rows past M: ldx != C, ldy != C; every
    sentinel and all of X's buffer keep their bits"""
    M = 197
    mods = _dev_mods(C, M, device)
    x = _case(C, M)[1].to(device)
    xb = torch.full((M, C + 24), 3.5, device=device)
    xb[:, 8:8 + C] = x
    xb0 = xb.clone()
    yb = torch.full((M + 5, C + 12), -1.75, device=device)
    xs, ys = xb[:, 8:8 + C], yb[:M, 4:4 + C]
    assert xs.stride(0) != C and ys.stride(0) != C and xs.data_ptr() % 16 == 0 and ys.data_ptr() % 16 == 0
    ops.block_mlp(xs, *mods, out=ys)
    assert torch.equal(xb.view(torch.int32), xb0.view(torch.int32))
    assert bool((yb[:, :4] == -1.75).all()) and bool((yb[:, 4 + C:] == -1.75).all()) and bool((yb[M:] == -1.75).all())
    _assert_bar(C, M, ys)
    # the same bits as the dense call
    assert torch.equal(ys.contiguous().view(torch.int32), ops.block_mlp(x, *mods).view(torch.int32))


@pytest.mark.parametrize("C", CHANNELS)
def test_in_place(device, C):
    """out = x2: every lane finishes the elements it stores from values it loaded itself"""
    M = 129
    mods = _dev_mods(C, M, device)
    x = _case(C, M)[1].to(device)
    y = ops.block_mlp(x, *mods)
    xi = x.clone()
    ops.block_mlp(xi, *mods, out=xi)
    assert torch.equal(xi.view(torch.int32), y.view(torch.int32))
    _assert_bar(C, M, y)


@pytest.mark.parametrize("C,M", [(C, 4097) for C in CHANNELS] + [c for c in SPLIT_CASES if c in
                                                                  ((128, 512 * 64 + 2000), (256, 256 * 64 + 1000))])
def test_reproducible(device, C, M):
    """two calls on the same inputs: equal bits, output and row exponents (which equal sfx_subm_rowexp of the output)"""
    ln, fc1, fc2 = [m.to(device) for m in _mods(C, 7 * C)]
    x = (torch.randn(M, C, generator=torch.Generator().manual_seed(M)) * 2.0).to(device)
    outs = []
    for _ in range(2):
        e = torch.full((M,), -999, device=device, dtype=torch.int32)
        outs.append((ops.block_mlp(x, ln, fc1, fc2, rowexp=e), e))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][1], ops.subm_rowexp(outs[0][0]))
    if M != 4097:
        assert ops.block_mlp_last_plan()["split"] > 1  # a split-tail shape


@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("M", [33, 65, 129])  # 33 and points-per-workgroup + 1 of both training tile kinds (64, 128)
def test_training_kinds(device, C, M):
    """block_mlp_train with a row scale that zeroes rows returns those rows bit-equal to X (the residual path with a
    zero keep factor); y, z and block_mlp_bwd at the bars of test_block_mlp_train_fwd_bwd"""
    g = torch.Generator().manual_seed(C + M)
    ln, fc1, fc2 = _mods(C, C + M)
    x = torch.randn(M, C, generator=g) * 2 + 0.3
    rs = (torch.rand(M, generator=g) > 0.3).float() / 0.7
    rs[0] = 0.0
    rs[M - 1] = 0.0
    dy = torch.randn(M, C, generator=g)
    xd = x.double()
    h2 = F.layer_norm(xd, (C,), ln.weight.double(), ln.bias.double(), ln.eps).detach().requires_grad_()
    z_ref = h2 @ fc1.weight.double().T + fc1.bias.double()
    y_ref = xd + rs.double()[:, None] * (F.gelu(z_ref) @ fc2.weight.double().T + fc2.bias.double())
    y_ref.backward(dy.double())
    mods = [m.to(device) for m in (ln, fc1, fc2)]
    z = torch.empty(M, 4 * C, device=device)
    xg = x.to(device)
    x0 = xg.clone()
    y = ops.block_mlp_train(xg, *mods, z, rowscale=rs.to(device))
    assert torch.equal(xg.view(torch.int32), x0.view(torch.int32))
    zero = (rs == 0).to(device)
    assert int(zero.sum()) >= 2
    assert torch.equal(y[zero].view(torch.int32), xg[zero].view(torch.int32))
    e_z, e_y, e_b = rel_l2(z.cpu(), z_ref), rel_l2(y.cpu(), y_ref), rel_l2((y - xg).cpu(), y_ref - xd)
    dh2 = ops.block_mlp_bwd(dy.to(device), *mods, z, rowscale=rs.to(device))
    e_d = rel_l2(dh2.cpu(), h2.grad)
    print(f"C={C} M={M}: z {e_z:.3e} y {e_y:.3e} branch {e_b:.3e} dh2 {e_d:.3e}")
    assert e_z < 2e-6 and e_y < 1e-6 and e_b < 2e-6 and e_d < 2e-6
    assert bool((dh2[zero] == 0).all())  # a dropped row has no gradient through the branch
