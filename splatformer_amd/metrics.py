"""Evaluation metrics on device: uint8-quantised PSNR and SSIM (reference utils/metrics.py + train.py:104-113).

`psnr_u8(pred, gt)` mirrors the reference evaluation contract for synthetic (3-channel) targets:
- train.py:104-113: `gt = (gt*255).to(uint8)`, `pred = (pred*255).to(uint8)` (truncation), pred having
  been clamped to <= 1 by gs_utils.py:111;
- utils/metrics.py:26-29: each batch is divided by 255 only if its max exceeds 1 (the max is taken over
  the whole [V,H,W,3] batch);
- utils/metrics.py:89-91: psnr = 20 log10(1 / sqrt(mse)) per image.

`eval_metrics_u8(pred, gt, mask)` is the same contract with the object mask of a 'real' scene (train.py:104-109:
the prediction alone is multiplied by the mask before the truncation) and the SSIM of the same uint8 images.  Both
come from one fused HIP kernel (sfx_eval_metrics_u8) that reads an RGBA target in place: the quantisation, the
per-image exact integer moments and the SSIM; mse is formed on the host from the integer sums.  `image_stats_u8`,
`psnr_u8` and `ssim(quantize_u8=True)` are that kernel without a mask; `ssim` of unquantised images is the SSIM term
of the training loss's kernel (sfx_image_loss, forward only).

Divergence (documented): when a batch's max is <= 1 and the OTHER batch's is too, the reference subtracts two uint8
tensors (wrap-around) and then fails in `.mean()` on a Byte tensor; here the values are used unscaled instead.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._lib import call, ptr, stream


def _same_rgb(what: str, pred: torch.Tensor, gt: torch.Tensor) -> None:
    if pred.shape != gt.shape or pred.dim() != 4 or pred.shape[-1] != 3:
        raise ValueError(f"{what}: expected two equal [V,H,W,3] tensors, got {tuple(pred.shape)}, {tuple(gt.shape)}")


def image_stats_u8(pred: torch.Tensor, gt: torch.Tensor, clamp_pred: bool = True):
    """Per-image exact integer moments of the quantised [V,H,W,3] images: sums [V,3] (p², g², pg), maxes [V,2]."""
    _same_rgb("image_stats_u8", pred, gt)
    sums, maxes, _ = eval_stats_u8(pred, gt, clamp_pred=clamp_pred)
    return sums, maxes


def psnr_from_stats(sums: torch.Tensor, maxes: torch.Tensor, elems: int) -> torch.Tensor:
    """PSNR per image [V] (float64) from the integer moments and the batch-max scaling rule."""
    s = sums.to(torch.float64).cpu()
    m = maxes.cpu()
    a = 1.0 / 255.0 if int(m[:, 0].max()) > 1 else 1.0
    b = 1.0 / 255.0 if int(m[:, 1].max()) > 1 else 1.0
    sse = a * a * s[:, 0] + b * b * s[:, 1] - 2.0 * a * b * s[:, 2]
    mse = sse.clamp_min(0.0) / elems
    return 20.0 * torch.log10(1.0 / torch.sqrt(mse))


def psnr_u8(pred: torch.Tensor, gt: torch.Tensor, clamp_pred: bool = True) -> torch.Tensor:
    """[V,H,W,3] prediction and target in [0,1] -> per-image PSNR [V] (float64, on the host)."""
    sums, maxes = image_stats_u8(pred, gt, clamp_pred)
    return psnr_from_stats(sums, maxes, pred.numel() // max(pred.shape[0], 1))


def gaussian_taps(window_size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """The reference's normalised 1-D Gaussian in fp32 (metrics.py:93-96)."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)],
                     dtype=torch.float32)
    return g / g.sum()


def ssim_window(window_size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """The reference's 2-D window (metrics.py:93-101): normalised 1-D Gaussian (fp32), outer product."""
    g = gaussian_taps(window_size, sigma).unsqueeze(1)
    return g.mm(g.t()).float()


_TAPS = {}


def device_taps(dev: torch.device) -> torch.Tensor:
    """gaussian_taps() on `dev`, uploaded once: the `window` argument of sfx_eval_metrics_u8 and sfx_image_loss."""
    taps = _TAPS.get(dev)
    if taps is None:
        taps = _TAPS[dev] = gaussian_taps().to(dev)
    return taps


def ssim(img1: torch.Tensor, img2: torch.Tensor, quantize_u8: bool = False) -> torch.Tensor:
    """[V,H,W,C] images (HWC) -> SSIM per image [V] (float32 on the device), = MetricComputer's
    `ssim(x.permute(0,3,1,2), ..., window_size=11, size_average=False)` (metrics.py:15, :103-135): the SSIM term of
    a forward-only sfx_image_loss call.
    quantize_u8: score the uint8 images of the evaluation loop (truncation, img1 clamped to <= 1, /255) -- C must be
    3, the SSIM of eval_stats_u8; the batch-max rule of metrics.py:26-29 is taken as dividing (it differs only for
    images whose largest uint8 value is <= 1)."""
    if quantize_u8:
        _same_rgb("ssim(quantize_u8=True)", img1, img2)
        return eval_stats_u8(img1, img2, clamp_pred=True)[2]
    if img1.shape != img2.shape or img1.dim() != 4:
        raise ValueError(f"ssim: expected two equal [V,H,W,C] tensors, got {tuple(img1.shape)}, {tuple(img2.shape)}")
    from .losses import image_loss_terms  # losses imports this module's taps
    return image_loss_terms(img1, img2)[:, 1].contiguous()


def eval_stats_u8(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor | None = None,
                  clamp_pred: bool = True):
    """The launch of eval_metrics_u8 alone, nothing read back: (sums [V,3] int64, maxes [V,2] int32, ssim [V]
    float32), all on the device.  Shapes as eval_metrics_u8."""
    if pred.dim() != 4 or pred.shape[-1] != 3:
        raise ValueError(f"eval_metrics_u8: pred must be [V,H,W,3], got {tuple(pred.shape)}")
    if gt.dim() != 4 or gt.shape[-1] not in (3, 4) or gt.shape[:3] != pred.shape[:3]:
        raise ValueError(f"eval_metrics_u8: gt must be [V,H,W,3] or [V,H,W,4] over pred's {tuple(pred.shape[:3])} "
                         f"pixels, got {tuple(gt.shape)}")
    V, H, W, _ = pred.shape
    if mask is not None and tuple(mask.shape) not in ((V, H, W), (V, H, W, 1)):
        raise ValueError(f"eval_metrics_u8: mask must be [V,H,W] or [V,H,W,1] over pred's pixels, "
                         f"got {tuple(mask.shape)}")
    _lib.require_gpu(pred)
    pred = pred.float().contiguous()
    gt = gt.float().contiguous()
    gs = gt.shape[-1]
    if mask is not None:
        mask = mask.float().contiguous()
        mptr, ms = ptr(mask), 1
    elif gs == 4:
        mptr, ms = ptr(gt) + 3 * gt.element_size(), 4  # the 4th channel, where it lies
    else:
        mptr, ms = None, 0
    dev = pred.device
    taps = device_taps(dev)
    sums = torch.empty(V, 3, device=dev, dtype=torch.int64)
    maxes = torch.empty(V, 2, device=dev, dtype=torch.int32)
    out = torch.empty(V, dtype=torch.float32, device=dev)
    ws = torch.empty(max(int(_lib.fn("sfx_eval_metrics_workspace_bytes")(V, H, W)), 8), dtype=torch.uint8, device=dev)
    call("sfx_eval_metrics_u8", V, H, W, ptr(pred), ptr(gt), gs, mptr, ms, 1 if clamp_pred else 0, ptr(taps),
         ptr(sums), ptr(maxes), ptr(out), ptr(ws), ws.numel(), stream())
    return sums, maxes, out


def eval_metrics_u8(pred: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor | None = None,
                    clamp_pred: bool = True) -> dict:
    """PSNR and SSIM of the evaluation loop's uint8 images in one fused pass (sfx_eval_metrics_u8), with the
    object mask of a 'real' scene (train.py:104-113, branch `gt_imgs.shape[-1] == 4`): the prediction alone is
    multiplied by the mask before both images are truncated to uint8; the metrics run over all pixels.

    pred [V,H,W,3]; gt [V,H,W,3] or [V,H,W,4].  A 4-channel gt is read in place (no slice, no copy) and its 4th
    channel is the mask, unless `mask` ([V,H,W] or [V,H,W,1]) is given; a 3-channel gt without a mask is the
    unmasked evaluation.  Any other shape raises ValueError.
    Returns {"psnr": [V] float64 on the host (psnr_from_stats, with its batch-max rule), "ssim": [V] float32 on
    the device (of the uint8 images / 255, as ssim(quantize_u8=True)), "sums": [V,3] int64, "maxes": [V,2] int32}
    (sums / maxes as image_stats_u8)."""
    sums, maxes, out = eval_stats_u8(pred, gt, mask, clamp_pred)
    V = pred.shape[0]
    psnr = psnr_from_stats(sums, maxes, pred[0].numel()) if V else torch.empty(0, dtype=torch.float64)
    return {"psnr": psnr, "ssim": out, "sums": sums, "maxes": maxes}
