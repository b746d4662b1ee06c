"""Training step of SplatFormer on MI355X (reference train.py:236-303, configs C/D).

Per scene: FeaturePredictor forward in train mode (ptv3_train), the refined Gaussians rendered to the
training views through the gsplat-compatible autograd path (gs_render / gsplat_compat HIP kernels; or, with
render="batched", through the eval path's single batched pass and its two-launch backward), the
image L1 loss `sum_v |pred_v - gt_v|.mean() / num_images / len(batch)` (train.py:272-283, image_l1 weight 1;
Trainer(lpips_loss_weight=..., lpips=LPIPS.from_files(...)) adds the reference's LPIPS term on VGG weights the
user supplies, lpips.py / csrc/lpips.hip, off by default because no weights are shipped; Trainer(ssim_loss_weight=...)
adds a D-SSIM term `1 - SSIM`, losses.py / csrc/loss.hip), backward through the
renderer to the packed refined record, then the hand-written refiner backward.  Every `accumulate_step`
micro-steps: gradient all-reduce (DDP average, one flat bucket over RCCL), clip_grad_norm_(2.0) and
Adam(lr 3e-5, eps 1e-15) on the trainable parameters (by default attn.qkv, utils/optimizers.py:48-52,
configs/train/default.gin; Trainer(finetune_list=...) selects any other set, None all of them, with a learning
rate per parameter group as the reference's lr_dict).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib
from . import losses
from . import lpips as lpips_mod
from . import ptv3_ops as ops
from . import ptv3_train as pt
from . import train_ops as tops
from .dist import allreduce_mean_
from .feature_predictor import ALL_FEATURES, FeaturePredictor
from .gs_render import rasterize_gaussians_to_multiimgs, rasterize_packed_to_multiimgs_batched

RENDER_MODES = ("per_view", "batched")


# ---- FeaturePredictor train forward / backward --------------------------------------------------------------
def refine_train(fp: FeaturePredictor, gs: Dict[str, Tensor], masks, perms=None, group=None):
    """refine_packed in train mode -> (packed [N, sum of output widths] refined record, tape)."""
    means = gs["means"]
    dev = means.device
    n = means.shape[0]
    cb = fp.backbone.output_dim
    h0, feat, grid, gmax = fp.pack_input(gs)
    depth = int(gmax.item()).bit_length()
    data = {"coord": means, "grid_coord": grid, "offset": [n], "feat": feat, "serialized_depth": depth}
    _, bb_tape = pt.backbone_forward(fp.backbone.backbone, data, masks, perms=perms, out=h0[:, :cb], group=group)
    w1, b1, mids, wl, bl, out_dim = fp._packed_heads()
    x = h0[:, :w1.shape[1]]
    hs = [ops.linear(x, w1, b1, act=ops.ACT_RELU)]
    for wm, bm in mids:
        hs.append(ops.grouped_linear(hs[-1], wm, bm, len(fp.output_features), act=ops.ACT_RELU))
    n_tanh = fp.ch["means"] if fp.output_features[0] == "means" else 0
    if fp.base_wiring:
        tab = None
        o = torch.empty(n, out_dim, device=dev, dtype=torch.float32)
        packed = ops.linear(hs[-1], wl, bl, act=ops.ACT_TANH, act_ncols=n_tanh, residual=feat, pre_out=o)
    else:  # any other wiring: the per-column epilogue; `o` keeps what its derivative reads
        tab = fp.col_table(dev)
        o = ops.linear(hs[-1], wl, bl)
        packed = ops.col_epilogue(o, tab, h0)
    # the heads' first-layer input is kept only when a head trains (its weight gradient reads it)
    return packed, dict(bb=bb_tape, hs=hs, o=o, n_tanh=n_tanh, cb=cb, tab=tab,
                        x=x if pt.trains(fp.features_outputhead) else None)


def scatter_head_grads(fp: FeaturePredictor, dw1: Tensor, db1: Tensor, dmids, dwl: Tensor, dbl: Tensor) -> None:
    """Add the gradients of the packed head matrices (FeaturePredictor._packed_heads: w1 [G*W, kpad] / b1, per mid
    layer (wm [G, W, W], bm [G, W]), the block-structured last layer wl [out_dim, G*W] / bl) to .grad of the
    per-feature features_outputhead[f] parameters that require grad: head g's row block of w1 without the pad
    columns, wm[g], and its own rows and hidden units of the last layer."""
    W = fp.width
    r = 0
    for g, f in enumerate(fp.output_features):
        head = fp.features_outputhead[f]
        c = fp.ch[f]
        sl = slice(g * W, (g + 1) * W)
        pieces = [(head[0].weight, dw1[sl, :fp.head_in]), (head[0].bias, db1[sl])]
        for li, (dwm, dbm) in enumerate(dmids):
            pieces += [(head[2 * (li + 1)].weight, dwm[g]), (head[2 * (li + 1)].bias, dbm[g])]
        pieces += [(head[-1].weight, dwl[r:r + c, sl]), (head[-1].bias, dbl[r:r + c])]
        for p, grad in pieces:
            if p.requires_grad:
                if p.grad is None:
                    p.grad = torch.zeros_like(p)
                p.grad += grad
        r += c


def _epilogue_bwd(tape: dict, d_packed: Tensor, out: Optional[Tensor]) -> Tensor:
    """d(loss)/d(packed record) -> d(loss)/d(last-layer output): tanh on the leading columns (ptv3_base.gin's
    wiring), or the column table's derivative."""
    if tape.get("tab") is None:
        return tops.act_bwd(d_packed, tape["o"], tops.DACT_TANH_OUT, ncols=tape["n_tanh"], out=out)
    return tops.col_epilogue_bwd(d_packed, tape["o"], tape["tab"], out=out)


def refine_backward(fp: FeaturePredictor, tape: dict, d_packed: Tensor) -> None:
    """d(loss)/d(packed record) -> gradients of every refiner parameter that requires grad (the input attributes
    are not trained)."""
    w1, b1, mids, wl, bl, out_dim = fp._packed_heads()
    G, W = len(fp.output_features), fp.width
    hs = tape["hs"]
    heads = tape.get("x") is not None
    dev = d_packed.device
    n = d_packed.shape[0]
    if heads:  # the last layer's weight gradient wants a multiple of 4 output columns: dz in zero-padded rows
        npad = (out_dim + 3) // 4 * 4
        dzp = torch.zeros(n, npad, device=dev, dtype=torch.float32)
        dz = _epilogue_bwd(tape, d_packed.contiguous(), dzp[:, :out_dim])
        dwl = torch.zeros(npad, G * W, device=dev, dtype=torch.float32)
        dbl = torch.zeros(npad, device=dev, dtype=torch.float32)
        tops.linear_wgrad(dzp, hs[-1], dwl, dbl)
        dmids = [(torch.zeros_like(wm), torch.zeros_like(bm)) for wm, bm in mids]
    else:
        dz = _epilogue_bwd(tape, d_packed.contiguous(), None)
    dh = tops.linear_bwd_data(dz, pt.wt(wl), dact=tops.DACT_RELU, dact_pre=hs[-1])
    for li in reversed(range(len(mids))):
        wm = mids[li][0]
        prev = hs[li]
        dprev = torch.empty_like(prev)
        for g in range(G):
            sl = slice(g * W, (g + 1) * W)
            if heads:
                tops.linear_wgrad(dh[:, sl], prev[:, sl], dmids[li][0][g], dmids[li][1][g])
            tops.linear_bwd_data(dh[:, sl], pt.wt(wm[g]), dact=tops.DACT_RELU, dact_pre=prev[:, sl], out=dprev[:, sl])
        dh = dprev
    if heads:
        dw1 = torch.zeros_like(w1)
        db1 = torch.zeros_like(b1)
        tops.linear_wgrad(dh, tape["x"], dw1, db1)
        scatter_head_grads(fp, dw1, db1, dmids, dwl, dbl)
    dx = tops.linear_bwd_data(dh, pt.wt(w1))
    pt.backbone_backward(tape["bb"], dx[:, :tape["cb"]].contiguous())


def unpack_leaf(fp: FeaturePredictor, packed: Tensor, gs: Dict[str, Tensor]):
    """The refined Gaussians as views of one grad-tracking leaf (render autograd lands in leaf.grad)."""
    leaf = packed.detach().requires_grad_()
    out = fp.unpack(leaf)
    for key in ALL_FEATURES:
        if fp.sh_degree == 0 and key == "features_rest":
            continue
        if key not in out:
            out[key] = gs[key]
    return leaf, out


def image_l1(pred: Sequence[Tensor], gt: Sequence[Tensor]) -> Tensor:
    """train.py:276-283: sum over views of mean |pred - gt| (normalised by the caller)."""
    loss = None
    for p, g in zip(pred, gt):
        v = (p - g).abs().mean()
        loss = v if loss is None else loss + v
    return loss


# ---- optimiser ------------------------------------------------------------------------------------------------
def select_trainable(model: torch.nn.Module, finetune_list) -> None:
    """utils/optimizers.py:4-16 filter_grads: a parameter requires grad iff its name contains one of the substrings;
    None or an empty list selects every parameter."""
    names = tuple(finetune_list or ())
    for name, p in model.named_parameters():
        p.requires_grad_(not names or any(s in name for s in names))


def param_lrs(model: FeaturePredictor, lr) -> Dict[int, float]:
    """id(parameter) -> learning rate.  `lr` is one number, or the reference's lr_dict
    (utils/optimizers.py:49-54, configs/train/default.gin): 'backbone' for every backbone parameter, one optional
    key per head feature ('means', 'scales', ...), 'base' for whatever has no key of its own."""
    if not isinstance(lr, dict):
        return {id(p): float(lr) for p in model.parameters()}
    if "base" not in lr:
        raise ValueError("an lr dict needs a 'base' entry (the fallback of utils/optimizers.py)")
    out = {id(p): float(lr["base"]) for p in model.parameters()}
    for p in model.backbone.parameters():
        out[id(p)] = float(lr.get("backbone", lr["base"]))
    for f, head in model.features_outputhead.items():
        for p in head.parameters():
            out[id(p)] = float(lr.get(f, lr["base"]))
    return out


class Trainer:
    """FeaturePredictor training on libsfx: filter_grads(finetune_list), flat gradient bucket (one RCCL
    all-reduce per optimiser step under DDP), clip_grad_norm_ + Adam on device.

    finetune_list: substrings of parameter names, with the semantics of the reference's filter_grads -- a
    parameter trains iff its name contains one of them.  The default ("attn.qkv",) is the reference's fine-tuning
    recipe (utils/optimizers.py:46-47); None or () trains every parameter (training from scratch), and any other
    list works too, e.g. ("mlp.fc", "features_outputhead").  The backward computes the gradients of exactly the
    selected parameters; a block whose mlp.fc1 / fc2 train runs the unfused MLP branch.
    lr: one learning rate, or a dict in the shape of the reference's lr_dict: 'backbone', one key per head feature
    ('means', 'scales', 'opacities', 'quats', 'features_dc', 'features_rest') and 'base' as the fallback; applied
    per parameter in optimizer_step."""

    def __init__(self, model: FeaturePredictor, lr=3e-5, eps: float = 1e-15, betas=(0.9, 0.999),
                 grad_clip_norm: float = 2.0, accumulate_step: int = 1, group=None, generator=None,
                 precision: Optional[str] = None, render: Optional[str] = None, finetune_list=("attn.qkv",),
                 image_l1_loss_weight: float = 1.0, ssim_loss_weight: float = 0.0, lpips_loss_weight: float = 0.0,
                 lpips=None):
        """image_l1_loss_weight, ssim_loss_weight, lpips_loss_weight: the per-view loss is
        `image_l1_loss_weight * mean|p - g| + ssim_loss_weight * (1 - SSIM(p, g)) + lpips_loss_weight * LPIPS(p, g)`,
        summed over the views and divided by num_images, len(scenes) and accumulate_step (the normalisation the
        reference gives image_l1 and its LPIPS term, train.py:277-286).  The L1 weight is the reference's
        (train.py:206, default 1).  The LPIPS term is the reference's (training.lpips_loss_weight, default 1 there;
        0 here, because it needs `lpips`, an lpips.LPIPS built from a weight file the user supplies: a weight above 0
        without one raises).  Its weights are frozen and are no part of state_dict.  The D-SSIM term (the
        reference's own SSIM, utils/metrics.py:93-135) is an option of this project and off by default.  With
        ssim_loss_weight == 0 the L1 term is the torch image_l1; above 0 one losses.image_loss_and_grad call per
        scene computes loss and derivative, and `last_metrics` holds the batch's image_l1, ssim and train_psnr
        (train.py:278, :283) as device tensors; with the LPIPS term it also holds "lpips".
        precision: "fp32" (default; fp32-accurate refiner forward + backward) or "amp", the reference's
        `training.enable_amp` (train.py:214-299, configs/train/default.gin:11): refiner forward and backward in
        the autocast precision class (ptv3_ops.precision); the renderer, loss and optimiser stay fp32 as in the
        reference (its rasterisation runs outside the autocast region).  No loss scale: the GEMMs scale every
        operand row by its own power of two, so fp16 range limits never flush or overflow a gradient; GradScaler's
        skip of a step with non-finite gradients is kept (optimizer_step).
        Default from SFX_TRAIN_PREC.
        render: "per_view" (default; the reference's loop over the views through the gsplat-compatible autograd ops)
        or "batched": all views of a scene in the eval path's single pass, the packed leaf handed to
        gs_render.rasterize_packed_to_multiimgs_batched, whose backward writes leaf.grad in one launch.  Default
        from SFX_TRAIN_RENDER."""
        self.model = model
        self.render = render or os.environ.get("SFX_TRAIN_RENDER", "per_view")
        if self.render not in RENDER_MODES:
            raise ValueError(f"render {self.render!r}: expected one of {RENDER_MODES}")
        self.precision = precision or os.environ.get("SFX_TRAIN_PREC", "fp32")
        if self.precision not in ops.PRECISIONS:
            raise ValueError(f"precision {self.precision!r}: expected one of {sorted(ops.PRECISIONS)}")
        if not (image_l1_loss_weight >= 0.0 and ssim_loss_weight >= 0.0):
            raise ValueError(f"loss weights must be >= 0, got image_l1_loss_weight {image_l1_loss_weight}, "
                             f"ssim_loss_weight {ssim_loss_weight}")
        if not lpips_loss_weight >= 0.0:
            raise ValueError(f"loss weights must be >= 0, got lpips_loss_weight {lpips_loss_weight}")
        if lpips_loss_weight > 0.0 and lpips is None:
            raise ValueError("lpips_loss_weight > 0 needs `lpips`, an lpips.LPIPS built from a VGG weight file "
                             "(LPIPS.from_files); no weights are shipped")
        self.image_l1_loss_weight = float(image_l1_loss_weight)
        self.ssim_loss_weight = float(ssim_loss_weight)
        self.lpips_loss_weight = float(lpips_loss_weight)
        self.lpips = lpips  # frozen, not a module: no parameter of it trains or is saved
        # filled by micro_step when ssim_loss_weight > 0 or lpips_loss_weight > 0
        self.last_metrics: Optional[Dict[str, Tensor]] = None
        if isinstance(finetune_list, str):
            finetune_list = (finetune_list,)
        self.finetune_list = tuple(finetune_list or ())
        select_trainable(model, self.finetune_list)    # utils/optimizers.py:4-16, :48-52
        pt.check_trainable(model.backbone.backbone)
        self.params = [p for p in model.parameters() if p.requires_grad]
        if not self.params:
            raise ValueError(f"finetune_list {self.finetune_list!r} selects no parameter")
        lrs = param_lrs(model, lr)
        self.param_lr = [lrs[id(p)] for p in self.params]
        dev = self.params[0].device
        total = sum(p.numel() for p in self.params)
        self.flat_grad = torch.zeros(total, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.lr, self.eps, self.betas, self.clip = lr, eps, betas, grad_clip_norm
        self.accumulate_step = accumulate_step
        self.group = group
        self.world = torch.distributed.get_world_size(group) if group is not None else 1
        self.masks = pt.device_drop_masks(generator)
        self.step_count = 0
        self.skipped_steps = 0  # amp: optimiser steps skipped for non-finite gradients (GradScaler semantics)
        self.micro = 0
        self.last_norm: Optional[Tensor] = None

    def micro_step(self, scenes: List[Dict[str, Tensor]], cameras: List[dict], images: List[List[Tensor]],
                   masks=None, perms=None) -> float:
        """Forward + backward of one batch (train.py:240-289); gradients accumulate in the flat bucket."""
        self.model.train()
        masks = masks or self.masks
        total = 0.0
        num_images = sum(len(im) for im in images)  # counted over the whole batch (train.py:273-281)
        fused = self.ssim_loss_weight > 0.0  # L1 + D-SSIM and its derivative from one kernel call per scene
        with_lpips = self.lpips_loss_weight > 0.0
        norm = 1.0 / num_images / len(scenes) / self.accumulate_step
        sums = None
        lpips_sum = None
        for gs, cams, imgs in zip(scenes, cameras, images):
            with ops.precision(self.precision):
                packed, tape = refine_train(self.model, gs, masks, perms=perms, group=self.group)
            batched = self.render == "batched"
            if batched:  # the packed record itself is the leaf: its gradient is written by one launch
                leaf, out_gs = packed.detach().requires_grad_(), None
                extra = {k: v for k, v in gs.items() if not (self.model.sh_degree == 0 and k == "features_rest")}
            else:
                leaf, out_gs = unpack_leaf(self.model, packed, gs)
            with torch.enable_grad():
                if batched:
                    preds, _ = rasterize_packed_to_multiimgs_batched(leaf, self.model.columns(), cams, extra=extra)
                else:
                    preds, _ = rasterize_gaussians_to_multiimgs(out_gs, cams)
                if fused:
                    stacked = torch.stack(list(preds), 0)
                    terms, d_pred = losses.image_loss_and_grad(
                        stacked, imgs, self.image_l1_loss_weight, self.ssim_loss_weight,
                        torch.full((len(preds),), norm, device=stacked.device, dtype=torch.float32))
                    loss = terms[:, 3].sum() * norm
                    if with_lpips:  # its derivative joins the fused one: one backward through the renderer
                        lp, d_lp = self.lpips.value_and_grad(
                            stacked, imgs, torch.full((len(preds),), norm * self.lpips_loss_weight,
                                                      device=stacked.device, dtype=torch.float32))
                        d_pred += d_lp
                        loss = loss + lp.sum() * (norm * self.lpips_loss_weight)
                        lpips_sum = lp.sum() if lpips_sum is None else lpips_sum + lp.sum()
                        del d_lp
                    torch.autograd.backward(stacked, d_pred)
                    # sums over the views of mean|p-g|, SSIM and the unquantised PSNR 20 log10(1 / sqrt(mse))
                    m = torch.stack([terms[:, 0].sum(), terms[:, 1].sum(), (-10.0 * torch.log10(terms[:, 2])).sum()])
                    sums = m if sums is None else sums + m
                    del stacked, d_pred
                else:
                    loss = image_l1(preds, imgs)
                    if self.image_l1_loss_weight != 1.0:  # (the default adds no launch)
                        loss = loss * self.image_l1_loss_weight
                    if with_lpips:
                        lp = lpips_mod.lpips_loss(preds, imgs, self.lpips)
                        loss = loss + lp.sum() * self.lpips_loss_weight
                        lpips_sum = lp.detach().sum() if lpips_sum is None else lpips_sum + lp.detach().sum()
                    loss = loss / num_images / len(scenes) / self.accumulate_step
                    loss.backward()
            with ops.precision(self.precision):
                refine_backward(self.model, tape, leaf.grad)
            total = total + loss.detach()  # summed on the device: one host read per micro-step, not per scene
            del tape, packed, leaf, out_gs, preds
        self.micro += 1
        if fused:  # averaged as train.py:283 averages train_psnr; device tensors, no host read
            avg = sums / num_images / len(scenes)
            self.last_metrics = {"image_l1": avg[0], "ssim": avg[1], "train_psnr": avg[2]}
        if with_lpips:
            self.last_metrics = dict(self.last_metrics or {}) if fused else {}
            self.last_metrics["lpips"] = lpips_sum / num_images / len(scenes)
        loss = float(total)  # (drains the stream)
        _lib.check_lookback("Trainer.micro_step")  # the step's scans / radix passes (pooling, intersection sort)
        return loss

    def optimizer_step(self) -> None:
        if self.group is not None and self.world > 1:
            allreduce_mean_(self.flat_grad, self.group)  # DDP: average over ranks, one bucket
        coef = None
        if self.clip > 0:
            coef, self.last_norm = tops.grad_clip_coef([self.flat_grad], self.clip)
        if self.precision == "amp":
            # GradScaler.step (train.py:297-298) skips the optimiser step when a gradient is inf / NaN; with no loss
            # scale to halve (the per-row operand scales need none) the skip is all that remains.  One 8-byte read
            # per optimiser step: the micro-steps' loss reads have drained the stream already.
            norm = self.last_norm if self.last_norm is not None else self.flat_grad.square().sum()
            if not bool(torch.isfinite(norm).all()):
                self.skipped_steps += 1
                self.flat_grad.zero_()
                self.micro = 0
                return
        self.step_count += 1
        for p, m1, m2, lr in zip(self.params, self.exp_avg, self.exp_avg_sq, self.param_lr):
            tops.adam_step(p.data, p.grad, m1, m2, self.step_count, lr, self.betas, self.eps, grad_scale=coef)
            # adam_step writes through a raw pointer, which torch does not see: bump the parameter's version so
            # every cache keyed on it (fp16x2 pre-split ops.weight_split, W^T ptv3_train.wt) is rebuilt
            if lr != 0.0:  # (lr 0: the moments move, the parameter keeps its bits)
                torch.autograd.graph.increment_version(p)
        self.flat_grad.zero_()
        self.micro = 0

    def state_dict(self) -> dict:
        """Optimiser state for a resume: Adam moments, step counts and the DropPath mask counter (so a resumed
        run draws new masks instead of replaying step 0's)."""
        return {"exp_avg": [t.detach().cpu() for t in self.exp_avg],
                "exp_avg_sq": [t.detach().cpu() for t in self.exp_avg_sq],
                "step_count": self.step_count, "skipped_steps": self.skipped_steps,
                "masks": self.masks.state_dict() if hasattr(self.masks, "state_dict") else None}

    def load_state_dict(self, sd: dict) -> None:
        """The moments follow self.params, i.e. the finetune_list the state was saved with."""
        shapes = [tuple(t.shape) for t in sd["exp_avg"]]
        if shapes != [tuple(p.shape) for p in self.params]:
            raise ValueError("optimiser state does not match the trainable parameters (saved with another "
                             "finetune_list?)")
        for dst, src in zip(self.exp_avg + self.exp_avg_sq, list(sd["exp_avg"]) + list(sd["exp_avg_sq"])):
            dst.copy_(src)
        self.step_count = int(sd["step_count"])
        self.skipped_steps = int(sd.get("skipped_steps", 0))
        if sd.get("masks") is not None and hasattr(self.masks, "load_state_dict"):
            self.masks.load_state_dict(sd["masks"])

    def step(self, scenes, cameras, images, masks=None, perms=None) -> float:
        loss = self.micro_step(scenes, cameras, images, masks=masks, perms=perms)
        if self.micro % self.accumulate_step == 0:
            self.optimizer_step()
        return loss
