"""Evaluation loop of the hot path (reference train.py:76-176 `evaluation`, test branch).

For each scene of this rank's chunk (dataset/GS.py:54-67): refine with the FeaturePredictor (one scene
per forward, feature_predictor.py:244), render the V test views of the refined Gaussians
(gs_utils.rasterize_gaussians_to_multiimgs), quantise prediction and target to uint8 and accumulate the
per-image PSNR and SSIM sums (train.py:104-131, utils/metrics.py); finally reduce to rank 0
(train.py:170-176).  With `lpips=` (an lpips.LPIPS built from a VGG weight file the user supplies) the third
column of the reference's eval.csv, LPIPS (utils/metrics.py:13-17), is computed on the same quantised images.

Masked branch (train.py:104-109, 'real' scenes): a target with a fourth channel (dataset/GS.py:128-151, the
object mask appended by scene_io.read_image) takes `pred = pred * mask` before the uint8 truncation; the target
is used as composited and the metrics run over all pixels.  Both kinds of target are scored by one fused kernel
(metrics.eval_metrics_u8), which reads an RGBA target in place.
The per-scene, per-image record (MetricComputer.results_dict, utils/metrics.py:48, written as
metrics.rank{r}.json by :82-84 / train.py:165) and `compare_with_input` (train.py:127-136, :184-189) are
optional outputs of the same loop.
"""
from __future__ import annotations

import json
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch

from . import _lib, dist
from .gs_render import rasterize_gaussians_to_multiimgs
from .metrics import eval_metrics_u8


def _score(pred: torch.Tensor, gt: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-image (psnr, ssim), float64 on the host, of rendered `pred` [V,H,W,3] against gt [V,H,W,3 or 4]: one
    fused pass; a 4th channel of gt is the mask that multiplies the prediction (train.py:104-109)."""
    m = eval_metrics_u8(pred, gt, clamp_pred=False)  # rgbs are already clamped (gs_utils.py:111)
    return m["psnr"], m["ssim"].double().cpu()


def _lpips(net, pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """Per-image LPIPS, float64 on the host, on the uint8-quantised images / 255; an RGBA target's mask multiplies
    the prediction first (train.py:104-113, metrics.py:26-29)."""
    if gt.shape[-1] == 4:
        return net(pred, gt[..., :3].contiguous(), quantize_u8=True, mask=gt[..., 3].contiguous()).double().cpu()
    return net(pred, gt, quantize_u8=True).double().cpu()


def _record(results: Optional[dict], name: str, psnr: torch.Tensor, ssim_: torch.Tensor,
            lpips_: Optional[torch.Tensor] = None) -> None:
    if results is not None:
        results[name] = {"psnr": psnr.tolist(), "ssim": ssim_.tolist()}
        if lpips_ is not None:
            results[name]["lpips"] = lpips_.tolist()


@torch.no_grad()
def evaluate_scenes(model, scenes: Sequence[dict], cameras: Sequence[dict],
                    targets: Callable[[int], torch.Tensor], device: torch.device,
                    evaluate_input: bool = False, *, results: Optional[dict] = None,
                    names: Optional[Sequence[str]] = None, compare_with_input: bool = False,
                    results_input: Optional[dict] = None, lpips=None) -> Dict[str, float]:
    """Evaluate this rank's chunk of `scenes`.

    scenes[i]: normalized Gaussian dict (device tensors); cameras[i]: camera dict (device tensors);
    targets(i): [V,H,W,3] ground-truth images in [0,1] for scene i (device), or [V,H,W,4] for a 'real' scene: the
    composited RGB plus the object mask (scene_io.read_image), scored through the mask.  A chunk may mix the two.
    results: a dict filled in place with this rank's record, results[name][metric] = [one float per image], metric
    in ("psnr", "ssim") -- the reference's MetricComputer.results_dict; name is str(i), or names[i] when `names`
    is given.  write_metrics() writes it as the reference's metrics.rank{r}.json.
    compare_with_input: also render scenes[i] itself and score it against the same targets and mask
    (train.py:127-136); the return value gains "psnr_input" and "ssim_input", reduced like the others.  Its
    per-image record goes to a second dict, `results_input` (same layout; the reference's
    metrics_input.rank{r}.json), not under a key of `results`.
    lpips: an lpips.LPIPS; the return value and the records gain "lpips" (and "lpips_input" with
    compare_with_input).  Without it the keys are "psnr" and "ssim" only.
    Returns the rank-0 reduced means ({} on other ranks)."""
    rank, ws = dist.world()
    mine = dist.scene_chunk(len(scenes), rank, ws)
    keys = ("psnr", "ssim") + (("psnr_input", "ssim_input") if compare_with_input else ())
    if lpips is not None:
        keys += ("lpips",) + (("lpips_input",) if compare_with_input else ())
    total = {k: torch.zeros((), dtype=torch.float64) for k in keys}
    num_images = 0
    for i in mine:
        gs = scenes[i] if evaluate_input else model([scenes[i]], [i])[0]
        rgbs, _ = rasterize_gaussians_to_multiimgs(gs, cameras[i])
        pred = torch.stack(rgbs, 0)
        gt = targets(i)
        name = str(i) if names is None else names[i]
        psnr, ssim_ = _score(pred, gt)
        lp = _lpips(lpips, pred, gt) if lpips is not None else None
        total["psnr"] += psnr.sum()
        total["ssim"] += ssim_.sum()
        if lp is not None:
            total["lpips"] += lp.sum()
        _record(results, name, psnr, ssim_, lp)
        if compare_with_input:
            if not evaluate_input:  # otherwise the prediction IS the input's render
                rgbs, _ = rasterize_gaussians_to_multiimgs(scenes[i], cameras[i])
                pred_in = torch.stack(rgbs, 0)
                psnr, ssim_ = _score(pred_in, gt)
                lp = _lpips(lpips, pred_in, gt) if lpips is not None else None
            total["psnr_input"] += psnr.sum()
            total["ssim_input"] += ssim_.sum()
            if lp is not None:
                total["lpips_input"] += lp.sum()
            _record(results_input, name, psnr, ssim_, lp)
        num_images += pred.shape[0]
        if not evaluate_input and hasattr(model, "check_refine"):
            model.check_refine()  # the refine's deferred pooling checks, at the readback that consumes it
        else:
            _lib.check_lookback("evaluate_scenes")  # the render's intersection scans / sorts
    return dist.reduce_metrics(total, num_images, len(mine),
                               device=device if ws > 1 and device.type == "cuda" else None)


def write_metrics(results: dict, path: str) -> None:
    """MetricComputer.write_to_file (utils/metrics.py:82-84): the per-scene, per-image record as JSON."""
    with open(path, "w") as f:
        json.dump(results, f, indent=4)
