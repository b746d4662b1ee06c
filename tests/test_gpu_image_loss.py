"""sfx_image_loss (csrc/loss.hip) and splatformer_amd.losses on the device: the per-view terms and the derivative of
`l1_weight * mean|p - g| + ssim_weight * (1 - SSIM)` against the CPU oracle.

Shapes [V,H,W,C]: a single pixel, an image smaller than the window radius, one pixel past a 32 x 16 tile edge in
each direction with C = 1, several tiles and views, and 64 x 64 x 3.  Inputs (test_image_loss_host.make_inputs):
noise, indep and flat (white background, the ill-conditioned case).

Bars.  The SSIM term: 2e-6 absolute against the values captured from the reference (tests/golden/metrics.npz), the
bar metrics.ssim is held to; on flat inputs no further from fp64 than 4x the oracle's own fp32 evaluation + 1e-7.  The
L1 and mse terms: 1e-6 relative to fp64.  The gradient: with e_hip the relative L2 of d_pred to the oracle's fp64
autograd and e_ref32 that of the oracle's fp32 autograd on the same inputs, e_hip <= 4 e_ref32 + 1e-7, where
e_ref32 < 1e-3 (it measures 1.5e-7 .. 3.4e-6 on noise / indep and 7e-6 .. 2e-4 on flat; a halo, padding or tap
error shows at >= 1e-2).  The kernel's sums are fp64 and its maps fp32: e_hip / e_ref32 measures 0.03 .. 0.59 over
these cases (DESIGN.md "Training image loss"), the largest where e_hip is the 3e-8 of the fp32 store.
"""
import functools
import os

import numpy as np
import pytest
import torch

from splatformer_amd import losses
from test_image_loss_host import SHAPES, make_inputs, oracle_loss_and_grad, rel_l2, upstream

pytestmark = pytest.mark.gpu

ALL_SHAPES = SHAPES + [(2, 64, 64, 3)]
KINDS = ["noise", "indep", "flat"]
WEIGHTS = [(0.0, 1.0), (0.75, 0.25)]  # fp32-representable (l1_weight, ssim_weight)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, l1_weight, ssim_weight):
    """The oracle in fp64 and in fp32, computed once per case and shared: (l1, ssim, mse, grad) each."""
    pred, gt = make_inputs(shape, kind)
    up = upstream(shape[0])
    r64 = oracle_loss_and_grad(pred, gt, l1_weight, ssim_weight, up, torch.float64)
    r32 = oracle_loss_and_grad(pred, gt, l1_weight, ssim_weight, up, torch.float32)
    return r64, r32


def test_ssim_term_matches_reference_golden(device):
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics.npz"))
    for i in range(2):
        a = torch.from_numpy(d[f"b{i}_img1"]).permute(0, 2, 3, 1).contiguous().to(device)
        b = torch.from_numpy(d[f"b{i}_img2"]).permute(0, 2, 3, 1).contiguous().to(device)
        terms, _ = losses.image_loss_and_grad(a, b, 1.0, 0.2, None)
        err = float((terms[:, 1].cpu() - torch.from_numpy(d[f"b{i}_ssim"])).abs().max())
        print(f"\n[golden b{i}] |SSIM - reference| = {err:.2e}")
        assert err < 2e-6


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_terms_match_fp64(device, shape, kind):
    pred, gt = make_inputs(shape, kind)
    l1w, sw = WEIGHTS[1]
    (l1, ssim, mse, _), (_, ssim32, _, _) = reference(shape, kind, l1w, sw)
    terms, _ = losses.image_loss_and_grad(pred.to(device), gt.to(device), l1w, sw, None)
    t = terms.cpu().double()
    e_l1 = float(((t[:, 0] - l1).abs() / l1).max())
    e_mse = float(((t[:, 2] - mse).abs() / mse).max())
    e_ssim = float((t[:, 1] - ssim).abs().max())
    e_ssim32 = float((ssim32.double() - ssim).abs().max())
    print(f"\n[{shape} {kind}] l1 rel {e_l1:.2e}, mse rel {e_mse:.2e}, |SSIM - fp64| {e_ssim:.2e} "
          f"(fp32 oracle {e_ssim32:.2e})")
    assert e_l1 <= 1e-6 and e_mse <= 1e-6
    assert e_ssim <= (4 * e_ssim32 + 1e-7 if kind == "flat" else 2e-6)
    want = l1w * l1 + sw * (1.0 - ssim)
    assert float((t[:, 3] - want).abs().max()) <= 1e-6


@pytest.mark.parametrize("l1w,sw", WEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_gradient_as_close_to_fp64_as_the_fp32_oracle(device, shape, kind, l1w, sw):
    pred, gt = make_inputs(shape, kind)
    r64, r32 = reference(shape, kind, l1w, sw)
    _, d_pred = losses.image_loss_and_grad(pred.to(device), gt.to(device), l1w, sw,
                                           upstream(shape[0], torch.float32).to(device))
    assert bool(torch.isfinite(d_pred).all())
    e_hip, e_ref32 = rel_l2(d_pred.cpu(), r64[3]), rel_l2(r32[3], r64[3])
    print(f"\n[{shape} {kind} l1 {l1w} ssim {sw}] to fp64: HIP {e_hip:.2e}, fp32 oracle {e_ref32:.2e}, "
          f"ratio {e_hip / max(e_ref32, 1e-30):.3f}")
    assert e_ref32 < 1e-3
    assert e_hip <= 4 * e_ref32 + 1e-7


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_l1_only_gradient_is_exact(device, shape):
    pred, gt = make_inputs(shape, "noise")
    pred.view(-1)[::3] = gt.view(-1)[::3]  # entries with p == g: sign(0) = 0
    V, H, W, C = shape
    scale = upstream(V, torch.float32)
    terms, d_pred = losses.image_loss_and_grad(pred.to(device), gt.to(device), 0.75, 0.0, scale.to(device))
    coef = (0.75 * scale.double() / (C * H * W)).float().view(V, 1, 1, 1)
    want = torch.sign(pred - gt) * coef
    assert torch.equal(d_pred.cpu(), want)
    assert int((d_pred == 0).sum()) >= (pred.numel() + 2) // 3
    # the terms do not depend on the weights' derivative path: SSIM is still reported
    full, _ = losses.image_loss_and_grad(pred.to(device), gt.to(device), 0.75, 0.25, None)
    assert torch.equal(terms[:, :3], full[:, :3])


@pytest.mark.parametrize("shape", [(3, 37, 50, 3), (2, 64, 64, 3)])
def test_deterministic_and_forward_only(device, shape):
    pred, gt = make_inputs(shape, "indep")
    p, g = pred.to(device), gt.to(device)
    scale = upstream(shape[0], torch.float32).to(device)
    t0, d0 = losses.image_loss_and_grad(p, g, 0.75, 0.25, scale)
    t1, d1 = losses.image_loss_and_grad(p, g, 0.75, 0.25, scale)
    assert torch.equal(t0, t1) and torch.equal(d0, d1)
    with torch.no_grad():  # no gradient wanted: d_pred = NULL, pass B does not run
        loss, t2 = losses.image_loss(p, g, 0.75, 0.25, return_terms=True)
    assert torch.equal(t2, t0) and torch.equal(loss, t0[:, 3])


def test_image_loss_autograd(device):
    shape = (3, 37, 50, 3)
    pred, gt = make_inputs(shape, "noise")
    p = pred.to(device).requires_grad_()
    g = gt.to(device)
    go = upstream(shape[0], torch.float32).to(device)
    loss, terms = losses.image_loss(p, g, 0.75, 0.25, return_terms=True)
    assert loss.shape == (3,) and loss.requires_grad and not terms.requires_grad
    loss.backward(go)
    t_direct, d_direct = losses.image_loss_and_grad(p, g, 0.75, 0.25, go)
    assert torch.equal(terms, t_direct) and torch.equal(loss.detach(), t_direct[:, 3])
    # fl(fl(x) * go) against fl(x * go): three fp32 roundings apart at the most
    assert torch.allclose(p.grad, d_direct, rtol=4 * 2.0 ** -24, atol=0)
    # a list of [H,W,C] views is stacked
    views = [pred[v].to(device).requires_grad_() for v in range(3)]
    loss_l = losses.image_loss(views, [g[v] for v in range(3)], 0.75, 0.25)
    loss_l.backward(go)
    assert torch.equal(loss_l.detach(), loss.detach())
    for v in range(3):
        assert torch.equal(views[v].grad, p.grad[v])
    with pytest.raises(RuntimeError):
        losses.image_loss(pred, gt)
    with pytest.raises(ValueError):
        losses.image_loss(p, g, -1.0, 0.0)
