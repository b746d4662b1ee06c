"""Training forward + hand-written backward of the refiner (configs C/D) on libsfx HIP kernels.

Reference: train.py:236-303 trains FeaturePredictor with `model.train()` semantics --
- DropPath (timm, per point) on the attention and MLP branches with the schedule of
  pointtransformer_v3.py:280-339 (drop_path=0.3, :145);
- BatchNorm1d with batch statistics (SyncBatchNorm under DDP, train.py:404) in the embedding, the pooling
  and the unpooling projections, running statistics updated;
- the same randperm(4) order shuffles as evaluation;
and by default only the parameters whose name contains 'attn.qkv' require grad (utils/optimizers.py:48-52
`finetune_list=['attn.qkv']; filter_grads(...)`).  The backward propagates the input gradient through every
layer from the loss down to the first encoder block (to the embedding when it trains) and accumulates the
gradient of every parameter that requires grad: with the default list the qkv projections' only, and then it
launches nothing else; with any other list (train.Trainer finetune_list) also the CPE conv / Linear
(sfx_subm_conv_wgrad on the folded conv, unfolded), the LayerNorms (sfx_layernorm_wgrad), attn.proj / mlp.fc2
(sfx_linear_wgrad_rs, the DropPath mask as row scale), mlp.fc1, the pooling / unpooling / embedding Linears and
their BatchNorms (the sums of the BN backward).

The forward keeps per-layer state on a tape (saved activations, not an autograd graph); `backward`
replays it in reverse.  Every op is a libsfx kernel (train_ops / ptv3_ops); torch only allocates.
"""
from __future__ import annotations

import os
import re
from typing import Callable, Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import ptv3_ops as ops
from . import train_ops as tops
from .ptv3 import (Block, Point, PointTransformerV3, SerializedPooling, SerializedUnpooling, point_windows,
                   point_windows_flash)

MaskFn = Callable[[str, int, float], Optional[Tensor]]


def wt(w: Tensor) -> Tensor:
    """W^T of a [N, K...] weight (flattened to [N, K]), cached on the tensor that owns the storage until the
    weight changes (the cache lives and dies with that tensor, so a reused allocation never hits it)."""
    holder = w._base if w._base is not None else w
    w2 = w.detach().reshape(w.shape[0], -1)
    key = (w2.storage_offset(), tuple(w2.shape), w2.stride(0), w._version)
    cache = holder.__dict__.setdefault("_sfx_wt", {})
    t = cache.get(key)
    if t is None:
        if len(cache) > 64:
            cache.clear()
        t = tops.transpose(w2)
        cache[key] = t
    return t


_MASK_STREAMS = [0]  # DropMasks objects created in this process (each gets its own seed stream)


class DropMasks:
    """timm DropPath per point: keep ~ Bernoulli(1-p), scaled by 1/(1-p); None when p == 0 (Identity).  One
    sfx_drop_mask launch per mask, hash-seeded from (base seed, rank, stream id, draw counter): reproducible for a
    seeded generator with no device read, different on every DDP rank (timm draws each rank's masks from its own
    device RNG state), and different for every DropMasks of the process (a second Trainer, or one re-created in
    the same process, does not replay the first one's masks).  state_dict / load_state_dict carry the counter
    across a checkpoint resume (Trainer.state_dict)."""

    def __init__(self, generator: Optional[torch.Generator] = None, rank: Optional[int] = None):
        self.base = int(generator.initial_seed()) if generator is not None else int(torch.initial_seed())
        if rank is None:
            dist = torch.distributed
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.rank = int(rank)
        self.stream_id = _MASK_STREAMS[0]
        _MASK_STREAMS[0] += 1
        self.k = 0

    def seed(self) -> int:
        m = 0xFFFFFFFFFFFFFFFF
        s = (self.base * 0x9E3779B97F4A7C15) & m
        s = (s ^ ((self.rank + 1) * 0xBF58476D1CE4E5B9)) & m
        s = (s ^ (self.stream_id * 0x94D049BB133111EB)) & m
        return (s + self.k * 0xD1B54A32D192ED03) & m

    def __call__(self, name: str, n: int, p: float, device=None) -> Optional[Tensor]:
        if p <= 0.0:
            return None
        self.k += 1
        return tops.drop_mask(n, 1.0 - p, self.seed(), device)

    def state_dict(self) -> dict:
        return {"base": self.base, "rank": self.rank, "stream_id": self.stream_id, "k": self.k}

    def load_state_dict(self, sd: dict) -> None:
        self.base, self.rank, self.stream_id, self.k = (int(sd[k]) for k in ("base", "rank", "stream_id", "k"))


def device_drop_masks(generator: Optional[torch.Generator] = None, rank: Optional[int] = None) -> MaskFn:
    """The default DropPath mask source of the training step (DropMasks)."""
    return DropMasks(generator, rank)


def _grad_buffers(lin: torch.nn.Linear):
    for p in (lin.weight, lin.bias):
        if p is not None and p.requires_grad and p.grad is None:
            p.grad = torch.zeros_like(p)
    return (lin.weight.grad if lin.weight.requires_grad else None,
            lin.bias.grad if lin.bias is not None and lin.bias.requires_grad else None)


# ---- parameter gradients of the layers other than qkv (each accumulates into .grad of the parameters that
# require grad and costs nothing for a frozen module) -------------------------------------------------------------
def trains(*mods) -> bool:
    """Whether any parameter of these modules / parameters requires grad."""
    for m in mods:
        ps = (m,) if isinstance(m, Tensor) else m.parameters()
        if any(p.requires_grad for p in ps):
            return True
    return False


def _grad(p: Optional[Tensor]) -> Optional[Tensor]:
    if p is None or not p.requires_grad:
        return None
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


def linear_param_grads(lin: torch.nn.Linear, dy: Tensor, x: Tensor, rowscale: Optional[Tensor] = None) -> None:
    """dW += (rowscale o dy)^T x, db += colsum(rowscale o dy) of an nn.Linear, for whichever of the two trains."""
    gw, gb = _grad(lin.weight), _grad(lin.bias)
    if gw is None and gb is None:
        return
    w2 = gw.reshape(gw.shape[0], -1) if gw is not None else torch.zeros_like(lin.weight)  # (bias alone: dW dropped)
    if x.shape[1] % 4 or x.stride(0) % 4 or x.data_ptr() % 16:
        if rowscale is not None:
            raise NotImplementedError("row-scaled weight gradient of an input that is not 16-byte aligned")
        tops.linear_wgrad_padk(dy, x, w2, gb)
    else:
        tops.linear_wgrad_rs(dy, x, rowscale, w2, gb)


def layernorm_param_grads(ln: torch.nn.LayerNorm, x: Tensor, dy: Tensor) -> None:
    gg, gb = _grad(ln.weight), _grad(ln.bias)
    if gg is not None or gb is not None:
        tops.layernorm_wgrad(x, dy, ln.eps, gg, gb)


def cpe_unfold_grads(dwf: Tensor, dbf: Tensor, w_conv: Tensor, b_conv: Tensor, w_lin: Tensor, mm=None):
    """Gradients of the folded CPE conv (W'_k = W_lin W_k, b' = W_lin b_conv + b_lin; dwf [C, 27*C], dbf [C]) ->
    (dW_conv [C, 27*C], db_conv, dW_lin, db_lin).  `mm(a, b)` = a @ b on weight-sized matrices (default torch;
    the training step passes the library GEMM)."""
    mm = mm or (lambda a, b: a @ b)
    wc = w_conv.reshape(w_conv.shape[0], -1)
    dw_lin = mm(dwf, wc.t()) + torch.outer(dbf, b_conv)
    dw_conv = mm(w_lin.t(), dwf)
    db_conv = mm(dbf[None, :], w_lin)[0]
    return dw_conv, db_conv, dw_lin, dbf


def _lib_mm(a: Tensor, b: Tensor) -> Tensor:
    """a @ b through the library GEMM (ops.linear computes x W^T)."""
    a = a.contiguous()
    bt = b.t()
    if not bt.is_contiguous():
        bt = tops.transpose(b.contiguous())
    return ops.linear(a, bt)


def cpe_param_grads(blk: Block, du: Tensor, conv_in: Tensor, smap) -> None:
    """cpe.0 (SubMConv3d) and cpe.1 (Linear): the weight gradient of the folded conv the forward ran
    (sfx_subm_conv_wgrad), unfolded into the two modules' parameters."""
    conv, lin = blk.cpe[0], blk.cpe[1]
    C = blk.channels
    dwf = torch.zeros(C, 27 * C, device=du.device, dtype=torch.float32)
    dbf = torch.zeros(C, device=du.device, dtype=torch.float32)
    tops.subm_conv_wgrad(du, conv_in, smap, dwf, dbf)
    dwc, dbc, dwl, dbl = cpe_unfold_grads(dwf, dbf, conv.weight.detach(), conv.bias.detach(), lin.weight.detach(),
                                          mm=_lib_mm)
    for p, g in ((conv.weight, dwc), (conv.bias, dbc), (lin.weight, dwl), (lin.bias, dbl)):
        pg = _grad(p)
        if pg is not None:
            pg += g.view_as(pg)


def bn_param_grads(bn: torch.nn.BatchNorm1d, sums: Tensor) -> None:
    """gamma / beta gradients of a train-mode BatchNorm from the (sum g, sum g*xhat) of its backward reduction --
    this rank's sums, before SyncBatchNorm's all-reduce (torch computes them per rank; the gradient all-reduce
    averages them)."""
    Cc = bn.weight.shape[0]
    gg, gb = _grad(bn.weight), _grad(bn.bias)
    if gb is not None:
        gb += sums[:Cc].float()
    if gg is not None:
        gg += sums[Cc:2 * Cc].float()


# ---- Block ------------------------------------------------------------------------------------------------
# SFX_MLP_TRAIN_FUSED=0: the training MLP tail as LayerNorm + two GEMMs forward and two GEMMs backward (the [n, 4C]
# GELU output and hidden gradient through HBM) instead of sfx_block_mlp_train / sfx_block_mlp_bwd
MLP_TRAIN_FUSED = os.environ.get("SFX_MLP_TRAIN_FUSED", "1") != "0"


def mlp_train_fused_ok(x2: Tensor, C: int) -> bool:
    return MLP_TRAIN_FUSED and C in ops.MLP_CHANNELS and x2.is_contiguous() and x2.data_ptr() % 16 == 0
def block_forward(blk: Block, name: str, point: Point, masks: MaskFn, conv_in: Optional[Tensor] = None,
                  out: Optional[Tensor] = None) -> dict:
    x = point.feat
    n, C = x.shape
    ln_c = blk.cpe[2]
    ln1, ln2, mlp = blk.norm1[0], blk.norm2[0], blk.mlp[0]
    wf, bf = blk.cpe_fused()  # Linear folded into the conv (when they train: cpe_param_grads unfolds the gradient)
    u = ops.subm_conv(x if conv_in is None else conv_in, point.nbr, wf, bf)
    x1, h = ops.cpe_residual_ln(u, x, ln_c.weight, ln_c.bias, ln1.weight, ln1.bias, ln1.eps)
    qkv = ops.linear(h, blk.attn.qkv.weight, blk.attn.qkv.bias)
    order = point.order_phys[point.order_type[blk.attn.order_index]]
    if blk.attn.enable_flash:  # K = 1024 windows cut at cu_seqlens
        K, win, nw = point_windows_flash(point, blk.attn.patch_size_max)
        a = ops.window_attention_varlen(qkv, order, win, nw, K, blk.attn.num_heads, C)
    else:
        K, win, nw = point_windows(point, blk.attn.patch_size_max)
        a = ops.window_attention(qkv, order, win, nw, K, blk.attn.num_heads, C)
    ma = masks(name + ".attn", n, blk.drop_prob, x.device)
    x2 = ops.linear(a, blk.attn.proj.weight, blk.attn.proj.bias, residual=x1, rowscale=ma)
    z = torch.empty(n, mlp.fc1.weight.shape[0], device=x.device, dtype=torch.float32)
    mm = masks(name + ".mlp", n, blk.drop_prob, x.device)
    # a block whose fc1 / fc2 train needs the hidden gradient and GELU(z) in HBM: it takes the unfused branch
    fused = mlp_train_fused_ok(x2, C) and not trains(mlp.fc1, mlp.fc2)
    if fused:  # LN2 + fc1 (z stored) + GELU + fc2 + mask + residual in one launch (csrc/mlp.hip MLP_TRAIN)
        point.feat = ops.block_mlp_train(x2, ln2, mlp.fc1, mlp.fc2, z, rowscale=mm, out=out)
    else:
        h2 = ops.layernorm(x2, ln2.weight, ln2.bias, ln2.eps)
        m = ops.linear(h2, mlp.fc1.weight, mlp.fc1.bias, act=ops.ACT_GELU, pre_out=z, pre_before_act=True)
        del h2
        point.feat = ops.linear(m, mlp.fc2.weight, mlp.fc2.bias, residual=x2, rowscale=mm, out=out)
    # the conv's input is kept only for a block whose CPE conv / Linear trains (their weight gradient reads it)
    cpe_in = (x if conv_in is None else conv_in) if trains(blk.cpe[0], blk.cpe[1]) else None
    return dict(kind="block", blk=blk, name=name, u=u, x1=x1, h=h, qkv=qkv, a=a, x2=x2, z=z, ma=ma, mm=mm,
                order=order, win=win, nw=nw, K=K, smap=point.nbr, sep_conv_in=conv_in is not None, mlp_fused=fused,
                cpe_in=cpe_in)


_TRACE: Optional[list] = None  # debugging: set to a list to record (tag, tensor) of the backward


def _trace(tag: str, t: Optional[Tensor]) -> None:
    if _TRACE is not None and t is not None:
        _TRACE.append((tag, t.detach().clone()))


def block_backward(rec: dict, dy: Tensor, need_input: bool):
    """-> (d block input, d separate conv input or None); the gradients of the block's parameters that require grad
    are accumulated (qkv only: the launches of the fine-tuning recipe, nothing else)."""
    blk: Block = rec["blk"]
    nm = rec["name"]
    for k in ("u", "x1", "h", "qkv", "x2", "z"):
        _trace(f"{nm}.fwd.{k}", rec[k])
    _trace(f"{nm}.dy", dy)
    C = blk.channels
    ln_c = blk.cpe[2]
    ln1, ln2, mlp = blk.norm1[0], blk.norm2[0], blk.mlp[0]
    if rec.get("mlp_fused"):  # fc2^T, GELU', fc1^T in one launch: the [n, 4C] hidden gradient stays on chip
        dh2 = ops.block_mlp_bwd(dy, ln2, mlp.fc1, mlp.fc2, rec["z"], rowscale=rec["mm"])
    else:
        dm = tops.linear_bwd_data(dy, wt(mlp.fc2.weight), rowscale=rec["mm"], dact=tops.DACT_GELU, dact_pre=rec["z"])
        dh2 = tops.linear_bwd_data(dm, wt(mlp.fc1.weight))
        _trace(f"{nm}.dm", dm)
        if trains(mlp.fc2):  # dW2 = (mask o dy)^T GELU(z)
            linear_param_grads(mlp.fc2, dy, tops.gelu(rec["z"]), rowscale=rec["mm"])
        if trains(mlp.fc1):  # dW1 = dm^T LN2(x2)
            linear_param_grads(mlp.fc1, dm, ops.layernorm(rec["x2"], ln2.weight, ln2.bias, ln2.eps))
        del dm
    layernorm_param_grads(ln2, rec["x2"], dh2)
    dx2 = tops.layernorm_bwd(rec["x2"], ln2.weight, dh2, ln2.eps, dres=dy)
    _trace(f"{nm}.dh2", dh2)
    _trace(f"{nm}.dx2", dx2)
    del dh2
    linear_param_grads(blk.attn.proj, dx2, rec["a"], rowscale=rec["ma"])
    da = tops.linear_bwd_data(dx2, wt(blk.attn.proj.weight), rowscale=rec["ma"])
    if blk.attn.enable_flash:
        dqkv = tops.window_attention_varlen_bwd(rec["qkv"], rec["order"], rec["win"], rec["nw"], rec["K"],
                                                blk.attn.num_heads, C, da)
    else:
        dqkv = tops.window_attention_bwd(rec["qkv"], rec["order"], rec["win"], rec["nw"], rec["K"],
                                         blk.attn.num_heads, C, da, attn_out=rec["a"])
    _trace(f"{nm}.da", da)
    _trace(f"{nm}.dqkv", dqkv)
    del da
    gw, gb = _grad_buffers(blk.attn.qkv)
    if gw is not None:
        tops.linear_wgrad(dqkv, rec["h"], gw, gb)
    elif gb is not None:
        linear_param_grads(blk.attn.qkv, dqkv, rec["h"])
    if not need_input and not trains(ln1, blk.cpe):
        return None, None
    dh = tops.linear_bwd_data(dqkv, wt(blk.attn.qkv.weight))
    del dqkv
    layernorm_param_grads(ln1, rec["x1"], dh)
    dx1, du = tops.cpe_ln_bwd(rec["u"], rec["x1"], ln_c.weight, ln1.weight, dx2, dh, ln1.eps)
    del dh, dx2
    layernorm_param_grads(ln_c, rec["u"], dx1)
    if rec.get("cpe_in") is not None:
        cpe_param_grads(blk, du, rec["cpe_in"], rec["smap"])
    if not need_input:
        return None, None
    dt = du
    wct = wt(blk.cpe_fused()[0])  # fused [Cout, 27*Cin] -> [27*Cin, Cout]
    if rec["sep_conv_in"]:
        dci = torch.zeros_like(dx1)
        tops.subm_conv_bwd_data(dt, rec["smap"], wct, dci)
        return dx1, dci
    tops.subm_conv_bwd_data(dt, rec["smap"], wct, dx1)  # residual gradient + conv gradient
    return dx1, None


# ---- pooling / unpooling -----------------------------------------------------------------------------------
def pool_forward(pool: SerializedPooling, point: Point, perm: Sequence[int], group=None):
    new, sidx, idx_ptr, m = pool.geometry(point, perm)
    pf = ops.linear(point.feat, pool.proj.weight, pool.proj.bias)
    s, arg = tops.segment_max_arg(pf, idx_ptr, sidx, m)
    del pf
    new.feat, st = tops.bn_train_forward(s, pool.norm[0], ops.ACT_GELU, group=group)
    new.pool_sidx, new.pool_idx_ptr = sidx, idx_ptr
    return new, dict(kind="pool", mod=pool, arg=arg, st=st, n_parent=point.feat.shape[0], group=group,
                     x=point.feat if trains(pool.proj) else None)


def _bn_sums_hook(bn: torch.nn.BatchNorm1d):
    return (lambda sums: bn_param_grads(bn, sums)) if trains(bn) else None


def pool_backward(rec: dict, dfeat: Tensor) -> Tensor:
    pool: SerializedPooling = rec["mod"]
    ds = tops.bn_act_bwd(rec["st"], pool.norm[0], ops.ACT_GELU, dfeat, group=rec["group"],
                         local_sums=_bn_sums_hook(pool.norm[0]))
    dpf = tops.segment_max_bwd(ds, rec["arg"], rec["n_parent"])
    if rec["x"] is not None:
        linear_param_grads(pool.proj, dpf, rec["x"])
    return tops.linear_bwd_data(dpf, wt(pool.proj.weight))


def unpool_forward(up: SerializedUnpooling, point: Point, group=None):
    parent = point.pop("pooling_parent")
    inverse = point.pop("pooling_inverse")
    zc = ops.linear(point.feat, up.proj[0].weight, up.proj[0].bias)
    coarse, stc = tops.bn_train_forward(zc, up.proj[1], ops.ACT_GELU, group=group)
    zs = ops.linear(parent.feat, up.proj_skip[0].weight, up.proj_skip[0].bias)
    skip, sts = tops.bn_train_forward(zs, up.proj_skip[1], ops.ACT_GELU, group=group)
    rec = dict(kind="unpool", mod=up, stc=stc, sts=sts, sidx=point.pool_sidx, idx_ptr=point.pool_idx_ptr,
               m=point.feat.shape[0], group=group, xc=point.feat if trains(up.proj[0]) else None,
               xs=parent.feat if trains(up.proj_skip[0]) else None)
    parent.feat = tops.bn_apply(sts, ops.ACT_GELU, residual=coarse, residual_idx=inverse)
    parent.stale_conv_feat = skip  # Pointcept quirk (see SerializedUnpooling.run)
    return parent, rec


def unpool_backward(rec: dict, dfeat: Tensor, dstale: Optional[Tensor]):
    """-> (d coarse input feature, d encoder skip feature)"""
    up: SerializedUnpooling = rec["mod"]
    dskip = dfeat if dstale is None else dfeat + dstale
    dcoarse = tops.segment_sum(dfeat, rec["idx_ptr"], rec["sidx"], rec["m"])
    dzs = tops.bn_act_bwd(rec["sts"], up.proj_skip[1], ops.ACT_GELU, dskip, group=rec["group"],
                          local_sums=_bn_sums_hook(up.proj_skip[1]))
    if rec["xs"] is not None:
        linear_param_grads(up.proj_skip[0], dzs, rec["xs"])
    d_enc = tops.linear_bwd_data(dzs, wt(up.proj_skip[0].weight))
    del dzs
    dzc = tops.bn_act_bwd(rec["stc"], up.proj[1], ops.ACT_GELU, dcoarse, group=rec["group"],
                          local_sums=_bn_sums_hook(up.proj[1]))
    if rec["xc"] is not None:
        linear_param_grads(up.proj[0], dzc, rec["xc"])
    d_coarse_in = tops.linear_bwd_data(dzc, wt(up.proj[0].weight))
    return d_coarse_in, d_enc


# ---- whole backbone ---------------------------------------------------------------------------------------
def check_trainable(bb: PointTransformerV3) -> None:
    """Raise for a trainable backbone parameter the hand-written backward has no gradient for.  Every parameter
    of the embedding, the blocks (cpe.0-2, norm1, attn.qkv / proj, norm2, mlp.fc1 / fc2), the poolings (proj, norm)
    and the unpoolings (proj, proj_skip) is covered; anything else (a module this backbone does not have today) is
    not."""
    known = re.compile(r"^(embedding\.[01]|(enc|dec)\.\w+\.block\d+\.(cpe\.[012]|norm[12]\.0|attn\.(qkv|proj)|"
                       r"mlp\.0\.fc[12])|enc\.\w+\.down\.(proj|norm\.0)|dec\.\w+\.up\.(proj|proj_skip)\.[01])"
                       r"\.(weight|bias)$")
    bad = [n for n, p in bb.named_parameters() if p.requires_grad and not known.match(n)]
    if bad:
        raise NotImplementedError(f"the training backward has no gradient for these parameters: {bad[:4]}...")


def backbone_forward(bb: PointTransformerV3, data_dict, masks: MaskFn, perms=None, out: Optional[Tensor] = None,
                     group=None):
    """PointTransformerV3.forward in train mode; -> (Point, tape)."""
    point = bb.prepare(data_dict, perms)
    emb, bnm = bb.embedding[0], bb.embedding[1]
    z = ops.linear(data_dict["feat"], emb.weight, emb.bias)
    point.feat, st = tops.bn_train_forward(z, bnm, ops.ACT_GELU, group=group)
    # the embedding's backward state (its Linear output and input) is kept only when the embedding trains
    emb_rec = dict(st=st, x=data_dict["feat"], group=group) if trains(emb, bnm) else None
    del z, st
    enc_recs: List[List[dict]] = []
    k = 1
    for s in range(bb.num_stages):
        stage = getattr(bb.enc, f"enc{s}")
        recs = []
        for name, mod in stage.named_children():
            if name == "down":
                point, r = pool_forward(mod, point, bb._draw_perm(perms, k), group)
                k += 1
            else:
                r = block_forward(mod, f"enc.enc{s}.{name}", point, masks)
            recs.append(r)
        enc_recs.append(recs)
    dec_recs: List[List[dict]] = []
    dec_names = [f"dec{s}" for s in reversed(range(bb.num_stages - 1))]
    for di, dn in enumerate(dec_names):
        stage = getattr(bb.dec, dn)
        children = list(stage.named_children())
        recs = []
        for ci, (name, mod) in enumerate(children):
            if name == "up":
                point, r = unpool_forward(mod, point, group)
            else:
                conv_in = point.pop("stale_conv_feat", None)
                last = di == len(dec_names) - 1 and ci == len(children) - 1
                r = block_forward(mod, f"dec.{dn}.{name}", point, masks, conv_in=conv_in, out=out if last else None)
            recs.append(r)
        dec_recs.append(recs)
    return point, dict(enc=enc_recs, dec=dec_recs, emb=emb_rec, bb=bb)


def embedding_backward(bb: PointTransformerV3, rec: dict, dfeat: Tensor) -> None:
    """Embedding = Linear + train-mode BatchNorm + GELU: gamma / beta from the BN sums, dW against the input
    attributes (Cin = 23 / 59 columns: tops.linear_wgrad_padk)."""
    emb, bnm = bb.embedding[0], bb.embedding[1]
    dz = tops.bn_act_bwd(rec["st"], bnm, ops.ACT_GELU, dfeat, group=rec["group"], local_sums=_bn_sums_hook(bnm))
    linear_param_grads(emb, dz, rec["x"])


def backbone_backward(tape: dict, dout: Tensor) -> None:
    """Accumulate, for d(loss)/d(backbone output) = dout, the gradient of every backbone parameter that requires
    grad."""
    g = dout
    skip_grads: Dict[int, Tensor] = {}
    n_dec = len(tape["dec"])
    for di in reversed(range(n_dec)):        # dec0 (last executed) first
        recs = tape["dec"][di]
        s = n_dec - 1 - di                   # decoder stage index (dec3 executed first)
        dstale = None
        for r in reversed(recs):
            if r["kind"] == "block":
                g, dci = block_backward(r, g, need_input=True)
                if dci is not None:
                    dstale = dci
            else:
                g, skip_grads[s] = unpool_backward(r, g, dstale)
    for s in reversed(range(len(tape["enc"]))):
        if s in skip_grads:
            g = g + skip_grads.pop(s)
        recs = tape["enc"][s]
        for i, r in enumerate(reversed(recs)):
            first = i == len(recs) - 1
            if r["kind"] == "block":
                lowest = s == 0 and first
                g, _ = block_backward(r, g, need_input=not lowest or tape.get("emb") is not None)
            else:
                g = pool_backward(r, g)
    if tape.get("emb") is not None:
        embedding_backward(tape["bb"], tape["emb"], g)
