"""Seeded fp32 inputs of the training-kernel edge tests, shared by tests/test_oracle_train.py (which shows on the
CPU that a wrong formula misses the bar on exactly these inputs) and tests/test_gpu_train_kernels.py.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).
"""
from __future__ import annotations

from typing import Dict, List

import torch

LN_EPS, BN_EPS, BN_MOMENTUM = 1e-5, 1e-3, 0.01


def gen(*key: int) -> torch.Generator:
    seed = 0
    for k in key:
        seed = seed * 100003 + int(k)
    return torch.Generator().manual_seed(seed)


def row_scales(M: int, g: torch.Generator, lo: float, hi: float) -> torch.Tensor:
    """[M, 1] magnitudes 10^lo .. 10^hi, log-uniform, the two ends present when M >= 2."""
    e = lo + (hi - lo) * torch.rand(M, 1, generator=g)
    if M >= 2:
        e[0], e[-1] = lo, hi
    return 10.0 ** e


def ln_case(M: int, C: int) -> Dict[str, torch.Tensor]:
    """LayerNorm backward / cpe tail / wgrad operands: rows 1e-3 .. 1e3 apart in magnitude, in x and in dy
    independently, and residual gradients of each row's own gradient magnitude (so a wrong LayerNorm term
    cannot hide under the residual, nor a small row under a large one)."""
    g = gen(1, M, C)
    sx, su, sd = row_scales(M, g, -3, 3), row_scales(M, g, -3, 3), row_scales(M, g, -3, 3)
    r = lambda *s: torch.randn(*s, generator=g)
    mag = sd / torch.sqrt(sx * sx + LN_EPS)  # |LN'(x) dy| of a row
    return {
        "x": (r(M, C) + 0.5) * sx, "dy": r(M, C) * sd, "dres": r(M, C) * mag,
        "gamma": torch.rand(C, generator=g) + 0.5,
        "u": (r(M, C) - 0.25) * su, "g_cpe": torch.rand(C, generator=g) + 0.5, "dx2": r(M, C) * mag,
    }


def bn_case(M: int, C: int) -> Dict[str, torch.Tensor]:
    """Train-mode BatchNorm operands; column C // 2 carries a +1e3 offset (mean >> spread)."""
    g = gen(2, M, C)
    r = lambda *s: torch.randn(*s, generator=g)
    x = r(M, C) * 3 + 1
    x[:, C // 2] += 1e3
    nres = M // 2 + 1
    return {
        "x": x, "dy": r(M, C), "gamma": torch.rand(C, generator=g) + 0.5, "beta": r(C),
        "running_mean": r(C), "running_var": torch.rand(C, generator=g) + 0.5,
        "res": r(nres, C), "ridx": torch.randint(0, nres, (M,), generator=g).int(), "res_rows": r(M, C),
        "base": r(M, C),
    }


def bn_chain_ref(c: Dict[str, torch.Tensor], act: int, residual: str, dtype: torch.dtype) -> Dict[str, torch.Tensor]:
    """oracle/train_ref.py's restatement of the whole train-mode BatchNorm chain on one bn_case, in `dtype`; residual
    = "idx" (res[ridx]), "rows" (res_rows, row for row) or "none".  fp64 goes through the summed statistics the
    kernels exchange; the fp32 yardstick takes two-pass moments (the sums of squares cancel in fp32)."""
    from . import train_ref as tr
    k = {n: (v.to(dtype) if v.is_floating_point() else v) for n, v in c.items()}
    M = float(k["x"].shape[0])
    two_pass = dtype != torch.float64
    mean, var = tr.bn_moments(k["x"]) if two_pass else tr.bn_stats_from_sums(tr.bn_sums(k["x"]), M)
    rstd, scale, shift, rm, rv = tr.bn_finalize(mean, var, M, k["gamma"], k["beta"], BN_EPS, BN_MOMENTUM,
                                                k["running_mean"], k["running_var"])
    res, ridx = {"idx": (k["res"], k["ridx"]), "rows": (k["res_rows"], None), "none": (None, None)}[residual]
    sums = tr.bn_bwd_sums(k["x"], mean, rstd, k["gamma"], k["beta"], act, k["dy"])
    return {"mean": mean, "rstd": rstd, "scale": scale, "shift": shift, "running_mean": rm, "running_var": rv,
            "y": tr.affine_act(k["x"], scale, shift, act, res, ridx), "bwd_sums": sums,
            "dx": tr.bn_bwd_apply(k["x"], mean, rstd, k["gamma"], k["beta"], act, k["dy"], sums, M)}


SEGMENT_LAYOUTS = ("one", "each", "mix", "reversed")


def segment_case(C: int, layout: str) -> Dict[str, object]:
    """A CSR pooling problem (idx_ptr, sorted_idx as int lists; x [n, C]; dy [m, C]; xs [n, C] finite, for the sum).

    one: a single segment of all 37 rows.  each: 37 segments of one row.  mix: runs of 1, 2, 3, 1000, 2, 1, 3
    rows.  reversed: runs of 5, 1, 8, 2, 16 rows whose run order is the reverse of the index order.  sorted_idx
    is a random permutation except in `reversed`.  In every run of >= 3 rows: the run's maximum of all columns is
    an exactly duplicated row pair whose first member in run order has the HIGHER row index; the last column is
    constant over the run; column 1 % C holds a -inf; column 2 % C holds only negative values and the zeros
    (-0.0, +0.0) in that run order -- (+0.0, -0.0) in every second such run.  A one-row run of `each` is -inf."""
    g = gen(3, C, SEGMENT_LAYOUTS.index(layout))
    sizes = {"one": [37], "each": [1] * 37, "mix": [1, 2, 3, 1000, 2, 1, 3], "reversed": [5, 1, 8, 2, 16]}[layout]
    n, m = sum(sizes), len(sizes)
    sidx = list(range(n - 1, -1, -1)) if layout == "reversed" else torch.randperm(n, generator=g).tolist()
    idx_ptr = [0]
    for s in sizes:
        idx_ptr.append(idx_ptr[-1] + s)
    x = torch.randn(n, C, generator=g)
    flip = False
    for s in range(m):
        beg, end = idx_ptr[s], idx_ptr[s + 1]
        if end - beg < 3:
            continue
        a, b = beg + 1, end - 1  # run positions of the duplicated pair, a first
        if sidx[a] < sidx[b]:
            sidx[a], sidx[b] = sidx[b], sidx[a]
        rows = sidx[beg:end]
        x[sidx[a]] = 10.0 + torch.rand(C, generator=g)
        x[sidx[b]] = x[sidx[a]]
        zc = 2 % C
        x[rows, zc] = -1.0 - torch.rand(len(rows), generator=g)
        x[sidx[beg], zc] = 0.0 if flip else -0.0
        x[sidx[beg + 2], zc] = -0.0 if flip else 0.0
        flip = not flip
        x[sidx[beg], 1 % C] = -float("inf")
        x[rows, C - 1] = 0.25
    if layout == "each":
        x[sidx[3]] = -float("inf")
    xs = torch.randn(n, C, generator=g) * row_scales(n, g, -3, 3)
    return {"n": n, "m": m, "idx_ptr": idx_ptr, "sidx": sidx, "x": x, "xs": xs, "dy": torch.randn(m, C, generator=g)}


def act_case(act: int) -> Dict[str, torch.Tensor]:
    """sfx_act_bwd operands at (500, 23): GELU' arguments out to |x| = 12, ReLU' arguments with exact +-0.0, tanh
    outputs in (-1, 1)."""
    g = gen(4, act)
    M, N = 500, 23
    dy = torch.randn(M, N, generator=g)
    pre = torch.randn(M, N, generator=g) * 3
    if act == 3:
        pre = torch.tanh(pre)
    else:
        pre[0, :8] = torch.tensor([12.0, -12.0, 0.0, -0.0, 6.0, -6.0, 1e-30, -1e-30])
        pre[-1, -4:] = torch.tensor([0.0, -0.0, 12.0, -12.0])
    return {"dy": dy, "pre": pre}


SUMSQ_SIZES = (1, 63, 64, 65, 255, 256, 257, 2048, 2049, 1024 * 2048 + 333)


def grads_case(n: int) -> List[torch.Tensor]:
    """Three gradient tensors (n, 65 and 2049 elements), magnitudes log-uniform over 1e-4 .. 1e2."""
    g = gen(5, n)
    return [torch.randn(k, generator=g) * row_scales(k, g, -4, 2)[:, 0] for k in (n, 65, 2049)]


def adam_case(n: int, steps: int = 4) -> Dict[str, object]:
    """Parameter and one gradient per step, magnitudes 1e-4 .. 1e2; every seventh gradient element (from index 3) is exactly 0."""
    g = gen(6, n)
    grads = []
    for _ in range(steps):
        gr = torch.randn(n, generator=g) * row_scales(n, g, -4, 2)[:, 0]
        gr[3::7] = 0.0
        grads.append(gr)
    return {"p": torch.randn(n, generator=g), "grads": grads}


# ---- the bars of the GPU tests (tests/test_gpu_train_ops.py's rule and test_gpu_train_all_params.py's) --------
BAR_TENSOR = 1e-5  # whole-tensor relative L2 to fp64
BAR_TIGHT = 1e-6   # segment ops, activation backward, optimiser


def rel_l2(a: torch.Tensor, ref: torch.Tensor) -> float:
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm().clamp_min(1e-30))


def slice_err(a: torch.Tensor, ref: torch.Tensor, dim: int) -> torch.Tensor:
    """Relative L2 error to `ref` (fp64) of every row (dim = 1) or column (dim = 0)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return (a - ref).norm(dim=dim) / ref.norm(dim=dim).clamp_min(1e-300)


def slice_bar(fp32_eval: torch.Tensor, ref: torch.Tensor, dim: int) -> torch.Tensor:
    """Per row / column: 4 x the error of the same formula evaluated in fp32 on the CPU, plus 1e-5."""
    return 4.0 * slice_err(fp32_eval, ref, dim) + 1e-5
