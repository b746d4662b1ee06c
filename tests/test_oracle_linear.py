"""oracle/linear_ref.py (the epilogue contract the GPU GEMM tests compare against) pinned to torch itself:
nn modules for the forward, autograd for the backward -- so the reference cannot share a mistake with the
kernel it judges.  CPU only, fp64."""
import pytest
import torch

from oracle import linear_ref as lr


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_unpooling_matches_torch_modules():
    """SerializedUnpooling's use: nn.Linear -> BatchNorm1d(eval) -> GELU -> + coarse[inverse], the BatchNorm
    folded to scale / shift; Ypre (pre_before_act = 0) is the skip value before the residual."""
    g = _g(0)
    M, N, K, Mc = 37, 12, 20, 9
    lin = torch.nn.Linear(K, N).double()
    bn = torch.nn.BatchNorm1d(N, eps=1e-3).double()
    with torch.no_grad():
        bn.running_mean.copy_(torch.randn(N, generator=g))
        bn.running_var.copy_(torch.rand(N, generator=g) + 0.3)
        bn.weight.copy_(torch.randn(N, generator=g))
        bn.bias.copy_(torch.randn(N, generator=g))
    bn.eval()
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    coarse = torch.randn(Mc, N, generator=g, dtype=torch.float64)
    inverse = torch.randint(0, Mc, (M,), generator=g)
    with torch.no_grad():
        skip = torch.nn.GELU()(bn(lin(x)))
        want = skip + coarse[inverse]
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    shift = bn.bias - bn.running_mean * scale
    y, pre = lr.linear_epilogue(x, lin.weight.detach(), lin.bias.detach(), scale.detach(), shift.detach(),
                                act=lr.ACT_GELU, R=coarse, residual_idx=inverse.int())
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(pre, skip, rtol=1e-12, atol=1e-12)
    # pre_before_act: Ypre is the BatchNorm output
    _, z = lr.linear_epilogue(x, lin.weight.detach(), lin.bias.detach(), scale.detach(), shift.detach(),
                              act=lr.ACT_GELU, R=coarse, residual_idx=inverse.int(), pre_before_act=True)
    with torch.no_grad():
        torch.testing.assert_close(z, bn(lin(x)), rtol=1e-12, atol=1e-12)


def test_droppath_matches_torch():
    """DropPath as x1 + mask * proj(a) (timm DropPath: mask = Bernoulli(keep) / keep per row)."""
    g = _g(1)
    M, C = 41, 16
    proj = torch.nn.Linear(C, C).double()
    a = torch.randn(M, C, generator=g, dtype=torch.float64)
    x1 = torch.randn(M, C, generator=g, dtype=torch.float64)
    mask = (torch.rand(M, generator=g) < 0.7).double() / 0.7
    assert 0 < int((mask == 0).sum()) < M
    with torch.no_grad():
        want = x1 + mask[:, None] * proj(a)
    y, pre = lr.linear_epilogue(a, proj.weight.detach(), proj.bias.detach(), rowscale=mask, R=x1)
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(y[mask == 0], x1[mask == 0])
    with torch.no_grad():
        torch.testing.assert_close(pre, mask[:, None] * proj(a), rtol=1e-12, atol=1e-12)


def test_out_rows_scatter_and_drop():
    """out_rows: GEMM row m lands on output row out_rows[m] (-1 dropped); rowscale / residual_idx are read at
    the OUTPUT row; rows nobody names stay NaN."""
    g = _g(2)
    M, N, K, T = 11, 5, 7, 17
    A = torch.randn(M, K, generator=g, dtype=torch.float64)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    rs = torch.rand(T, generator=g, dtype=torch.float64)
    R = torch.randn(4, N, generator=g, dtype=torch.float64)
    ridx = torch.randint(0, 4, (T,), generator=g)
    rows = torch.randperm(T, generator=g)[:M].clone()
    rows[3] = -1
    y, pre = lr.linear_epilogue(A, W, act=lr.ACT_TANH, act_ncols=2, rowscale=rs, R=R, residual_idx=ridx, out_rows=rows,
                                n_out_rows=T)
    named = torch.zeros(T, dtype=torch.bool)
    for m in range(M):
        o = int(rows[m])
        if o < 0:
            continue
        named[o] = True
        z = A[m] @ W.T
        v = torch.cat([torch.tanh(z[:2]), z[2:]]) * rs[o]
        torch.testing.assert_close(y[o], v + R[ridx[o]], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(pre[o], v, rtol=1e-12, atol=1e-12)
    assert bool(torch.isnan(y[~named]).all()) and bool(torch.isnan(pre[~named]).all()) and int(named.sum()) == M - 1


def test_grouped_is_block_diagonal():
    g = _g(3)
    M, G, N, K = 9, 3, 4, 6
    A = torch.randn(M, G * K, generator=g, dtype=torch.float64)
    W = torch.randn(G, N, K, generator=g, dtype=torch.float64)
    b = torch.randn(G, N, generator=g, dtype=torch.float64)
    y, _ = lr.linear_epilogue(A, W, b, act=lr.ACT_RELU, groups=G)
    want = torch.relu(A @ torch.block_diag(*W).T + b.flatten())
    torch.testing.assert_close(y, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("dact,ncols", [(lr.ACT_GELU, -1), (lr.ACT_GELU, 5), (lr.ACT_RELU, 5), (lr.ACT_RELU, 0),
                                        (lr.ACT_TANH, 5), (lr.ACT_TANH, 13)])
def test_bwd_data_matches_autograd(dact, ncols):
    """linear_bwd_data against autograd of y = rowscale[:, None] * (act(pre) @ W^T) w.r.t. pre, the activation
    on the first `ncols` columns only; tanh's derivative is given the activation's OUTPUT."""
    g = _g(10 * dact + ncols)
    M, N, K = 19, 8, 13
    pre = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    rs = (torch.rand(M, generator=g) < 0.6).double() / 0.6
    dY = torch.randn(M, N, generator=g, dtype=torch.float64)
    base = torch.randn(M, K, generator=g, dtype=torch.float64)
    n = K if ncols < 0 else ncols
    h = torch.cat([lr.activation(pre[:, :n], dact), pre[:, n:]], 1)
    y = rs[:, None] * (h @ W.T)
    (want,) = torch.autograd.grad(y, pre, dY)
    saved = h.detach() if dact == lr.ACT_TANH else pre.detach()
    got = lr.linear_bwd_data(dY, W, rs, dact, ncols, saved)
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(lr.linear_bwd_data(dY, W, rs, dact, ncols, saved, base), base + want, rtol=1e-11,
                               atol=1e-12)


def test_fp32_evaluation_keeps_dtype():
    """The same functions give the fp32 yardstick: everything is computed in the first argument's dtype."""
    g = _g(4)
    A = torch.randn(6, 8, generator=g)
    W = torch.randn(5, 8, generator=g).double()
    y, p = lr.linear_epilogue(A, W, act=lr.ACT_GELU)
    assert y.dtype == torch.float32 and p.dtype == torch.float32
    assert lr.linear_bwd_data(torch.randn(6, 5, generator=g), W).dtype == torch.float32
