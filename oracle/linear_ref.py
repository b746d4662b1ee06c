"""CPU restatement of the GEMM epilogue contract of sfx_linear / sfx_linear_bwd_data (include/sfx.h).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Plain torch, dtype-generic: every function computes in the dtype of its first argument, so the same code
gives the fp64 reference and the fp32 yardstick of the GPU tests.  The functions restate the header's
contract, not the kernel's code; tests/test_oracle_linear.py pins them to torch.nn modules and autograd.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3


def activation(z: torch.Tensor, act: int) -> torch.Tensor:
    """act: 0 none, 1 GELU (erf form), 2 ReLU, 3 tanh."""
    if act == ACT_NONE:
        return z
    if act == ACT_GELU:
        return F.gelu(z)  # approximate="none": the erf form
    if act == ACT_RELU:
        return torch.relu(z)
    if act == ACT_TANH:
        return torch.tanh(z)
    raise ValueError(f"activation {act}")


def activation_grad(pre: torch.Tensor, dact: int) -> torch.Tensor:
    """act'(.) as sfx_linear_bwd_data takes it: 1 GELU(erf) and 2 ReLU are given the pre-activation, 3 tanh is
    given the activation's output."""
    if dact == ACT_GELU:
        phi = torch.exp(-0.5 * pre * pre) * 0.3989422804014326779  # 1 / sqrt(2 pi)
        return 0.5 * (1.0 + torch.erf(pre * 0.7071067811865475244)) + pre * phi
    if dact == ACT_RELU:
        return (pre > 0).to(pre.dtype)
    if dact == ACT_TANH:
        return 1.0 - pre * pre
    raise ValueError(f"dact {dact}")


def _cols(t: torch.Tensor, ncols: int, fn) -> torch.Tensor:
    """fn applied to columns < ncols (-1 = all) of t."""
    n = t.shape[1] if ncols < 0 else min(ncols, t.shape[1])
    if n == 0:
        return t
    return torch.cat([fn(t[:, :n]), t[:, n:]], 1)


def linear_epilogue(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
                    scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                    act_ncols: int = -1, rowscale: Optional[torch.Tensor] = None, R: Optional[torch.Tensor] = None,
                    residual_idx: Optional[torch.Tensor] = None, out_rows: Optional[torch.Tensor] = None,
                    n_out_rows: Optional[int] = None, pre_before_act: bool = False,
                    groups: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """(Y, Ypre) of sfx_linear, both [n_out_rows, N] (groups > 1: [M, groups * N]).

    z = (A W^T + bias) * scale + shift;  v = rowscale * act(z) (act on columns < act_ncols);
    Y[o] = v[m] + R[residual_idx[o]] for o = out_rows[m] (o = m without out_rows; R[o] without residual_idx);
    Ypre[o] = z[m] with pre_before_act, else v[m].  GEMM rows with out_rows[m] == -1 are dropped; output rows
    that no GEMM row names hold NaN in both results (the kernel leaves them untouched).  rowscale and
    residual_idx are indexed by OUTPUT row.  Every floating operand is converted to A's dtype.

    groups > 1 (the block-diagonal heads): A [M, G * K], W [G, N, K], bias [G, N]; only bias and a full-width
    activation are defined there."""
    dt = A.dtype
    c = lambda t: None if t is None else t.to(dt)
    W, bias, scale, shift, rowscale, R = c(W), c(bias), c(scale), c(shift), c(rowscale), c(R)
    M = A.shape[0]
    if groups > 1:
        if any(t is not None for t in (scale, shift, rowscale, R, residual_idx, out_rows)) or act_ncols >= 0:
            raise ValueError("grouped linear: only bias and a full-width activation are defined")
        G, N, K = W.shape
        z = torch.cat([A[:, g * K:(g + 1) * K] @ W[g].T + (bias[g] if bias is not None else 0) for g in range(G)], 1)
        y = activation(z, act)
        return y, (z if pre_before_act else y)
    z = A @ W.T
    if bias is not None:
        z = z + bias
    if scale is not None:
        z = z * scale + shift
    v = _cols(z, act_ncols, lambda t: activation(t, act))
    if out_rows is None:
        o = torch.arange(M)
        n_out = M if n_out_rows is None else n_out_rows
    else:
        o = out_rows.long()
        if n_out_rows is None:
            raise ValueError("out_rows needs n_out_rows")
        n_out = n_out_rows
    keep = o >= 0
    ok = o[keep]
    if ok.unique().numel() != ok.numel():
        raise ValueError("out_rows must name every output row at most once")
    z, v = z[keep], v[keep]
    if rowscale is not None:
        v = v * rowscale[ok][:, None]
    y = v
    if R is not None:
        y = v + R[(residual_idx.long()[ok] if residual_idx is not None else ok)]
    Y = torch.full((n_out, z.shape[1]), float("nan"), dtype=dt)
    P = torch.full((n_out, z.shape[1]), float("nan"), dtype=dt)
    Y[ok] = y
    P[ok] = z if pre_before_act else v
    return Y, P


def linear_bwd_data(dY: torch.Tensor, W: torch.Tensor, rowscale: Optional[torch.Tensor] = None, dact: int = ACT_NONE,
                    dact_ncols: int = -1, dact_pre: Optional[torch.Tensor] = None,
                    base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX [M, K] of sfx_linear_bwd_data: base + rowscale[m] * (dY W) * act'(dact_pre) on columns < dact_ncols
    (-1 = all); W [N, K] (the kernel takes its transpose); base = the accumulated-into dX or None."""
    dt = dY.dtype
    d = dY @ W.to(dt)
    if rowscale is not None:
        d = d * rowscale.to(dt)[:, None]
    if dact != ACT_NONE:
        n = d.shape[1] if dact_ncols < 0 else min(dact_ncols, d.shape[1])
        if n > 0:
            d = torch.cat([d[:, :n] * activation_grad(dact_pre.to(dt)[:, :n], dact), d[:, n:]], 1)
    return d if base is None else base.to(dt) + d
