"""CPU restatement of the training step's normalisation, pooling, activation and optimiser operations
(csrc/train.hip; contracts in include/sfx.h).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).

Plain torch, dtype-generic: every function computes in the dtype of its first tensor argument, so the same
code gives the fp64 reference and the fp32 yardstick of the GPU tests.  Loops stand where the order is part
of the contract (the run order of a CSR segment).  The functions restate the formulas of torch
(F.layer_norm, BatchNorm1d.train(), clip_grad_norm_, optim.Adam) and of torch_scatter segment_csr, not the
kernels' code; tests/test_oracle_train.py pins them to those modules in fp64.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

ACT_NONE, ACT_GELU, ACT_RELU, ACT_TANH_OUT = 0, 1, 2, 3


# ---- LayerNorm ------------------------------------------------------------------------------------------
def _ln_stats(x: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)  # biased
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd, rstd


def layernorm_bwd(x: Tensor, gamma: Tensor, dy: Tensor, eps: float, dres: Optional[Tensor] = None) -> Tensor:
    """d x of LayerNorm(x) * gamma + beta given dy, plus the residual gradient dres when given."""
    xh, rstd = _ln_stats(x, eps)
    gy = dy * gamma
    dx = rstd * (gy - gy.mean(1, keepdim=True) - xh * (gy * xh).mean(1, keepdim=True))
    return dx if dres is None else dx + dres


def cpe_ln_bwd(u: Tensor, x1: Tensor, g_cpe: Tensor, g1: Tensor, dx2: Tensor, dh: Tensor,
               eps: float) -> Tuple[Tensor, Tensor]:
    """Block tail x1 = x + LN_cpe(u), h = LN1(x1):  dx1 = dx2 + LN1'(x1) dh,  du = LN_cpe'(u) dx1."""
    dx1 = layernorm_bwd(x1, g1, dh, eps, dx2)
    return dx1, layernorm_bwd(u, g_cpe, dx1, eps)


def layernorm_wgrad(x: Tensor, dy: Tensor, eps: float) -> Tuple[Tensor, Tensor]:
    """(dgamma, dbeta) = (sum_m dy * xhat, sum_m dy)."""
    xh, _ = _ln_stats(x, eps)
    return (dy * xh).sum(0), dy.sum(0)


# ---- activations ----------------------------------------------------------------------------------------
def gelu(z: Tensor) -> Tensor:
    return 0.5 * z * (1.0 + torch.erf(z * 0.7071067811865475244))


def act_grad(p: Tensor, act: int) -> Tensor:
    """act'(.): 1 GELU (erf form) and 2 ReLU are given the pre-activation, 3 tanh is given its output."""
    if act == ACT_GELU:
        return 0.5 * (1.0 + torch.erf(p * 0.7071067811865475244)) + p * torch.exp(-0.5 * p * p) * 0.3989422804014326779
    if act == ACT_RELU:
        return (p > 0).to(p.dtype)
    if act == ACT_TANH_OUT:
        return 1.0 - p * p
    raise ValueError(f"act {act}")


def act_bwd(dy: Tensor, pre: Tensor, act: int, ncols: int) -> Tensor:
    """dy * act'(pre) on the first ncols columns, dy on the others."""
    out = dy.clone()
    if ncols > 0:
        out[:, :ncols] = dy[:, :ncols] * act_grad(pre[:, :ncols], act)
    return out


# ---- train-mode BatchNorm1d (+ GELU) over summed statistics and an explicit global row count ---------------
def bn_sums(x: Tensor) -> Tensor:
    """This rank's (sum x, sum x^2) per column, [2, C]."""
    return torch.stack([x.sum(0), (x * x).sum(0)])


def bn_moments(x: Tensor) -> Tuple[Tensor, Tensor]:
    """(mean, biased variance) of one batch in two passes: equal to bn_stats_from_sums(bn_sums(x), M) in exact
    arithmetic, and the form that is well conditioned in fp32 (the yardstick's)."""
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).mean(0)


def bn_stats_from_sums(sums: Tensor, count: float) -> Tuple[Tensor, Tensor]:
    mean = sums[0] / count
    return mean, (sums[1] / count - mean * mean).clamp_min(0.0)


def bn_finalize(mean: Tensor, var: Tensor, count: float, gamma: Tensor, beta: Tensor, eps: float, momentum: float,
                running_mean: Optional[Tensor] = None, running_var: Optional[Tensor] = None):
    """(rstd, scale, shift, new running_mean, new running_var); the running variance takes the unbiased batch
    variance var * count / (count - 1), the running pair is (None, None) when not given."""
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    rm = rv = None
    if running_mean is not None:
        unbiased = var * (count / (count - 1.0)) if count > 1 else var
        rm = (1.0 - momentum) * running_mean + momentum * mean
        rv = (1.0 - momentum) * running_var + momentum * unbiased
    return rstd, scale, shift, rm, rv


def affine_act(x: Tensor, scale: Tensor, shift: Tensor, act: int, residual: Optional[Tensor] = None,
               ridx: Optional[Tensor] = None) -> Tensor:
    """act(x * scale + shift) (+ residual[ridx], or + residual row for row)."""
    v = x * scale + shift
    if act == ACT_GELU:
        v = gelu(v)
    if residual is not None:
        v = v + (residual if ridx is None else residual[ridx.long()])
    return v


def _bn_g(x, mean, rstd, gamma, beta, act, dy):
    xh = (x - mean) * rstd
    g = dy * act_grad(xh * gamma + beta, ACT_GELU) if act == ACT_GELU else dy
    return xh, g


def bn_bwd_sums(x: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, beta: Tensor, act: int, dy: Tensor) -> Tensor:
    """This rank's (sum g, sum g * xhat) per column, [2, C], g = dy * act'(BN(x)): (dbeta, dgamma) locally, and
    after the sum over ranks the two terms of the input gradient."""
    xh, g = _bn_g(x, mean, rstd, gamma, beta, act, dy)
    return torch.stack([g.sum(0), (g * xh).sum(0)])


def bn_bwd_apply(x: Tensor, mean: Tensor, rstd: Tensor, gamma: Tensor, beta: Tensor, act: int, dy: Tensor,
                 sums: Tensor, count: float) -> Tensor:
    """dx = gamma * rstd * (g - S0 / count - xhat * S1 / count) with the global sums and count."""
    xh, g = _bn_g(x, mean, rstd, gamma, beta, act, dy)
    return gamma * rstd * (g - sums[0] / count - xh * (sums[1] / count))


# ---- CSR segments (torch_scatter segment_csr) ---------------------------------------------------------------
def segment_max_arg(x: Tensor, idx_ptr: Sequence[int], sidx: Sequence[int]) -> Tuple[Tensor, Tensor]:
    """Per column the maximum over the rows sidx[idx_ptr[s] : idx_ptr[s + 1]] and the row that holds it: the FIRST
    such row in run order (a later row replaces the held one only when strictly greater, so +0.0 does not
    replace -0.0 nor the reverse).  An empty segment gives (-inf, -1)."""
    idx_ptr, sidx = [int(v) for v in idx_ptr], [int(v) for v in sidx]
    m, C = len(idx_ptr) - 1, x.shape[1]
    y = torch.full((m, C), -float("inf"), dtype=x.dtype)
    arg = torch.full((m, C), -1, dtype=torch.int64)
    for s in range(m):
        for p in range(idx_ptr[s], idx_ptr[s + 1]):
            r = sidx[p]
            take = (x[r] > y[s]) | (arg[s] < 0)
            y[s] = torch.where(take, x[r], y[s])
            arg[s] = torch.where(take, torch.full_like(arg[s], r), arg[s])
    return y, arg


def segment_max_bwd(dy: Tensor, arg: Tensor, n_rows: int) -> Tensor:
    """The arg-max row of each (segment, column) receives that gradient whole; every other entry is zero."""
    dx = [[0.0] * dy.shape[1] for _ in range(n_rows)]
    for arg_s, dy_s in zip(arg.tolist(), dy.tolist()):
        for c, (r, v) in enumerate(zip(arg_s, dy_s)):
            if r >= 0:
                dx[r][c] = v
    return torch.tensor(dx, dtype=dy.dtype).reshape(n_rows, dy.shape[1])


def segment_sum(x: Tensor, idx_ptr: Sequence[int], sidx: Sequence[int]) -> Tensor:
    idx_ptr, sidx = [int(v) for v in idx_ptr], [int(v) for v in sidx]
    y = torch.zeros(len(idx_ptr) - 1, x.shape[1], dtype=x.dtype)
    for s in range(len(idx_ptr) - 1):
        for p in range(idx_ptr[s], idx_ptr[s + 1]):
            y[s] = y[s] + x[sidx[p]]
    return y


# ---- optimiser ------------------------------------------------------------------------------------------------
def grad_norm(grads: Sequence[Tensor]) -> Tensor:
    """The 2-norm of all gradients taken as one vector."""
    return torch.sqrt(sum((g * g).sum() for g in grads))


def clip_coef(norm, max_norm: float):
    """clip_grad_norm_'s factor min(1, max_norm / (norm + 1e-6))."""
    return torch.clamp(max_norm / (torch.as_tensor(norm) + 1e-6), max=1.0)


def adam_step(p: Tensor, g: Tensor, m1: Tensor, m2: Tensor, step: int, lr: float, beta1: float, beta2: float,
              eps: float, weight_decay: float = 0.0, grad_scale=None) -> Tuple[Tensor, Tensor, Tensor]:
    """torch.optim.Adam's single-tensor update -> (p, exp_avg, exp_avg_sq): the gradient is scaled by grad_scale
    first, weight_decay is folded into it (L2, not AdamW), the moments are bias-corrected by 1 - beta^step."""
    dt = p.dtype
    gr = g.to(dt) if grad_scale is None else g.to(dt) * torch.as_tensor(grad_scale, dtype=dt)
    if weight_decay != 0.0:
        gr = gr + weight_decay * p
    m1 = m1.to(dt) + (1.0 - beta1) * (gr - m1.to(dt))
    m2 = beta2 * m2.to(dt) + (1.0 - beta2) * gr * gr
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    denom = torch.sqrt(m2) / bc2 ** 0.5 + eps
    return p - (lr / bc1) * m1 / denom, m1, m2
