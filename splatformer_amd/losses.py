"""Training image loss on device: per view `l1_weight * mean|p - g| + ssim_weight * (1 - SSIM)` and its derivative
(csrc/loss.hip, sfx_image_loss).

The L1 term is the reference's image_l1 (train.py:275-280); the D-SSIM term uses the reference's own SSIM
(utils/metrics.py:93-135, the one `metrics.ssim` evaluates); the reference's LPIPS term is lpips.py's, on VGG
weights the user supplies.  Forward and derivative come from one kernel call; there is no CPU fallback.

`image_loss_and_grad` is the direct form for a caller that knows the upstream scale of every view (the Trainer);
`image_loss` wraps it as an autograd function.
"""
from __future__ import annotations

from typing import Optional, Sequence, Union

import torch
from torch import Tensor

from . import _lib
from ._lib import call, ptr, stream
from .metrics import device_taps

Images = Union[Tensor, Sequence[Tensor]]


def _stacked(x: Images) -> Tensor:
    return x if isinstance(x, Tensor) else torch.stack(list(x), 0)


def _check_weights(l1_weight: float, ssim_weight: float) -> None:
    if not (l1_weight >= 0.0 and ssim_weight >= 0.0):
        raise ValueError(f"loss weights must be >= 0, got l1 {l1_weight}, ssim {ssim_weight}")


def _run(pred: Tensor, gt: Tensor, l1_weight: float, ssim_weight: float, view_scale: Optional[Tensor],
         want_grad: bool):
    _lib.require_gpu(pred)
    _lib.require_gpu(gt)
    _check_weights(l1_weight, ssim_weight)
    if pred.shape != gt.shape or pred.dim() != 4:
        raise ValueError(f"image loss: expected two equal [V,H,W,C] tensors, got {tuple(pred.shape)}, "
                         f"{tuple(gt.shape)}")
    V, H, W, C = pred.shape
    p = pred.detach().float().contiguous()
    g = gt.detach().float().contiguous()
    dev = p.device
    if view_scale is not None:
        if view_scale.shape != (V,):
            raise ValueError(f"view_scale: expected [{V}], got {tuple(view_scale.shape)}")
        view_scale = view_scale.detach().to(device=dev, dtype=torch.float32).contiguous()
    taps = device_taps(dev)
    grad_ssim = want_grad and ssim_weight > 0.0
    nbytes = int(_lib.fn("sfx_image_loss_workspace_bytes")(V, H, W, C))
    if not grad_ssim:  # tile sums only (include/sfx.h): no room for the derivative maps
        nbytes -= 12 * p.numel()
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
    terms = torch.empty(V, 4, dtype=torch.float32, device=dev)
    d_pred = torch.empty_like(p) if want_grad else None
    call("sfx_image_loss", V, H, W, C, ptr(p), ptr(g), ptr(taps), float(l1_weight), float(ssim_weight),
         ptr(view_scale), ptr(terms), ptr(d_pred), ptr(ws), ws.numel(), stream())
    return terms, d_pred


def image_loss_terms(pred: Images, gt: Images, l1_weight: float = 1.0, ssim_weight: float = 0.0) -> Tensor:
    """Forward only: the terms [V,4] of image_loss_and_grad, no derivative (metrics.ssim is terms[:, 1])."""
    return _run(_stacked(pred), _stacked(gt), l1_weight, ssim_weight, None, False)[0]


def image_loss_and_grad(pred: Images, gt: Images, l1_weight: float = 1.0, ssim_weight: float = 0.0,
                        view_scale: Optional[Tensor] = None):
    """One kernel call -> (terms [V,4], d_pred [V,H,W,C]).  terms[v] = mean|p-g|, SSIM, mean (p-g)^2 and the
    weighted loss of view v (none of them scaled); d_pred[v] = view_scale[v] * d(weighted loss_v)/d pred
    (view_scale: [V] on the device, None = 1).  Nothing here is tracked by autograd: hand d_pred to
    `torch.autograd.backward(pred, d_pred)`."""
    return _run(_stacked(pred), _stacked(gt), l1_weight, ssim_weight, view_scale, True)


class _ImageLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, l1_weight, ssim_weight):
        terms, d_pred = _run(pred, gt, l1_weight, ssim_weight, None, ctx.needs_input_grad[0])
        ctx.d_pred = d_pred
        ctx.mark_non_differentiable(terms)
        return terms[:, 3].clone(), terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        return ctx.d_pred * grad_loss.reshape(-1, 1, 1, 1).to(ctx.d_pred.dtype), None, None, None


def image_loss(pred: Images, gt: Images, l1_weight: float = 1.0, ssim_weight: float = 0.0,
               return_terms: bool = False):
    """Per-view weighted loss [V], differentiable with respect to pred ([V,H,W,C], or a list of [H,W,C] that is
    stacked).  The forward runs the kernel once and keeps the derivative; the backward scales it by grad_out[v].
    return_terms: also the detached [V,4] terms (mean|p-g|, SSIM, mean (p-g)^2, weighted loss)."""
    loss, terms = _ImageLoss.apply(_stacked(pred), _stacked(gt), float(l1_weight), float(ssim_weight))
    return (loss, terms) if return_terms else loss
