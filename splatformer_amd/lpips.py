"""LPIPS(net='vgg') as an evaluation metric and a training loss on libsfx (csrc/lpips.hip).

The reference trains with `training.lpips_loss_weight = 1.0` (configs/train/default.gin:12, train.py:269-282,
loss_utils.lpips_loss_fn) and reports LPIPS next to PSNR and SSIM (utils/metrics.py:13-17).  The network weights
are a file the user supplies (nothing is shipped or fetched); the arithmetic is the library's: a frozen VGG16
feature stack of 3x3 convolutions (MFMA), 2x2 max pools and the five-tap normalised distance, forward and data
backward, with no torch fallback.

Definition (written from the `lpips` package, version 0.1.4; parity with the package itself is not pinned by a
test, the definition below is -- tests/lpips_ref.py restates it in fp64):

  x, y: [V,H,W,3] fp32 in [0,1], H, W >= 16
  u_c = ((2 x_c - 1) - shift_c) / scale_c, shift (-0.030, -0.088, -0.188), scale (0.458, 0.448, 0.450)
  VGG16 `features`: convs (3x3, stride 1, zero padding 1, bias, ReLU) at torchvision indices
      0,2 | 5,7 | 10,12,14 | 17,19,21 | 24,26,28   (| = 2x2 max pool, stride 2, floor)
  taps f_l after the ReLUs of convs 2, 7, 14, 21, 28:  f^ = f / (sqrt(sum_c f^2) + 1e-10),
  LPIPS = sum_l mean_{h,w} sum_c w_{l,c} (f^x - f^y)^2, one value per image.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _lib
from ._lib import call, ptr, stream

Images = Union[Tensor, Sequence[Tensor]]

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)   # torchvision vgg16.features indices of the convs
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
           (512, 512), (512, 512), (512, 512), (512, 512))
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))  # lpips.LPIPS net.slice{1..5}
POOL_BEFORE = (2, 4, 7, 10)   # positions (0..12) of the convs that read a pooled map
TAPS = (1, 3, 6, 9, 12)       # positions of the tapped convs (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3)
TAP_CH = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
MIN_SIZE = 16


# ---- weight files -----------------------------------------------------------------------------------------------
def _take(sd: dict, key: str, shape: Tuple[int, ...]) -> Tensor:
    if key not in sd:
        raise KeyError(f"LPIPS weights: missing key '{key}'")
    t = sd[key]
    if not isinstance(t, Tensor) or tuple(t.shape) != tuple(shape):
        got = tuple(t.shape) if isinstance(t, Tensor) else type(t).__name__
        raise ValueError(f"LPIPS weights: key '{key}' has shape {got}, expected {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


def parse_state_dict(sd: dict, lin_sd: Optional[dict] = None) -> Tuple[List[Tuple[Tensor, Tensor]], List[Tensor]]:
    """(13 x (weight [Cout,Cin,3,3], bias [Cout]), 5 x lin weight [C]) from either layout:
    one `lpips.LPIPS(net='vgg')` state dict (net.slice{s}.{idx}.weight|bias, lin{l}.model.1.weight, optional
    scaling_layer.shift|scale; the duplicate `lins.*` keys are ignored), or a torchvision VGG16 state dict
    (features.{idx}.weight|bias) plus the package's vgg.pth (lin{l}.model.1.weight) as `lin_sd`.
    Strict: a missing key or a wrong shape raises and names the key."""
    two_files = lin_sd is not None
    convs = []
    for pos, idx in enumerate(CONV_IDX):
        cin, cout = CONV_CH[pos]
        if two_files:
            base = f"features.{idx}"
        else:
            s = next(i for i, sl in enumerate(SLICES) if idx in sl) + 1
            base = f"net.slice{s}.{idx}"
        convs.append((_take(sd, base + ".weight", (cout, cin, 3, 3)), _take(sd, base + ".bias", (cout,))))
    src = lin_sd if two_files else sd
    lins = [_take(src, f"lin{l}.model.1.weight", (1, c, 1, 1)).reshape(c).contiguous() for l, c in enumerate(TAP_CH)]
    for key, want in (("scaling_layer.shift", SHIFT), ("scaling_layer.scale", SCALE)):
        if key in src:  # optional: the kernels carry the package's constants, a file that disagrees is refused
            got = src[key].detach().double().reshape(-1)
            if got.numel() != 3 or not torch.allclose(got, torch.tensor(want, dtype=torch.float64), atol=1e-6):
                raise ValueError(f"LPIPS weights: key '{key}' = {got.tolist()} differs from the built-in {want}")
    return convs, lins


def _stacked(x: Images) -> Tensor:
    return x if isinstance(x, Tensor) else torch.stack(list(x), 0)


class LPIPS:
    """LPIPS(net='vgg') with frozen weights on one device.  The weights are packed once (forward at construction,
    the rotated / transposed set of the data backward at the first gradient call); they are plain tensors, not
    parameters: nothing here trains or enters a state_dict."""

    # views are processed in chunks of at most this many pixels, so the saved activations (about 1.1 kB per pixel:
    # 0.7 GB per 800 x 800 image, derived) stay bounded and every operand stays below 2 GiB
    max_chunk_pixels = 4 * 800 * 800

    def __init__(self, convs: Sequence[Tuple[Tensor, Tensor]], lins: Sequence[Tensor], device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("LPIPS runs on the GPU only (libsfx has no CPU fallback)")
        _lib.require_gpu()
        if len(convs) != 13 or len(lins) != 5:
            raise ValueError("LPIPS: expected 13 convolutions and 5 lin layers")
        self.device = dev
        self.w = [w.to(dev, torch.float32).contiguous() for w, _ in convs]
        self.b = [b.to(dev, torch.float32).contiguous() for _, b in convs]
        self.lin = [l.to(dev, torch.float32).contiguous() for l in lins]
        for pos, (w, b) in enumerate(zip(self.w, self.b)):
            cin, cout = CONV_CH[pos]
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"LPIPS: conv {CONV_IDX[pos]} has shapes {tuple(w.shape)}, {tuple(b.shape)}")
        self.fwd = [pack_conv(w, False) for w in self.w]
        self._bwd: Optional[List[Tensor]] = None

    @classmethod
    def from_state_dict(cls, sd: dict, lin_sd: Optional[dict] = None, device="cuda") -> "LPIPS":
        return cls(*parse_state_dict(sd, lin_sd), device=device)

    @classmethod
    def from_files(cls, path: str, lin_path: Optional[str] = None, device="cuda") -> "LPIPS":
        sd = torch.load(path, map_location="cpu", weights_only=True)
        lin_sd = torch.load(lin_path, map_location="cpu", weights_only=True) if lin_path is not None else None
        return cls.from_state_dict(sd, lin_sd, device=device)

    # ---- pieces ------------------------------------------------------------------------------------------------
    def _bwd_packs(self) -> List[Tensor]:
        if self._bwd is None:
            self._bwd = [pack_conv(w, True) for w in self.w]
        return self._bwd

    def _chunks(self, V: int, H: int, W: int):
        n = max(1, min(V, self.max_chunk_pixels // (H * W), (2 ** 31 - 1) // (H * W * 64 * 4)))
        return [(a, min(V, a + n)) for a in range(0, V, n)]

    def _forward(self, x: Tensor, quantize_u8: bool, mask: Optional[Tensor], keep: bool, on_tap=None) -> List[Tensor]:
        """The 13 post-ReLU activations of a chunk (keep), or only what `on_tap(level, activation)` makes of the
        five taps (the others are released as the network advances)."""
        cur = lpips_input(x, mask=mask, quantize_u8=quantize_u8)
        acts = []
        for pos in range(13):
            if pos in POOL_BEFORE:
                cur = maxpool2x2(cur)
            cin, cout = CONV_CH[pos]
            cur = conv3x3(cur, self.fwd[pos], cout, bias=self.b[pos], relu=True)
            if keep:
                acts.append(cur)
            if on_tap is not None and pos in TAPS:
                on_tap(TAPS.index(pos), cur)
        return acts

    def _prep(self, pred: Images, gt: Images, mask: Optional[Tensor]):
        p, g = _stacked(pred), _stacked(gt)
        _lib.require_gpu(p)
        _lib.require_gpu(g)
        if p.shape != g.shape or p.dim() != 4 or p.shape[-1] != 3:
            raise ValueError(f"LPIPS: expected two equal [V,H,W,3] tensors, got {tuple(p.shape)}, {tuple(g.shape)}")
        V, H, W, _ = p.shape
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPS: images of {H} x {W}; the VGG stack needs at least {MIN_SIZE} x {MIN_SIZE}")
        if mask is not None:
            if tuple(mask.shape) != (V, H, W):
                raise ValueError(f"LPIPS: mask of shape {tuple(mask.shape)}, expected {(V, H, W)}")
            mask = mask.detach().float().contiguous()
        return p.detach().float().contiguous(), g.detach().float().contiguous(), mask

    def _gt_taps(self, g: Tensor, quantize_u8: bool) -> List[Tensor]:
        taps: List[Optional[Tensor]] = [None] * 5

        def keep_tap(level, f):
            taps[level] = tap_normalize(f)
        self._forward(g, quantize_u8, None, False, keep_tap)
        return taps

    # ---- public ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_with_tape(self, x: Images) -> List[Tensor]:
        """The 13 post-ReLU activations [V,h,w,C] of x [V,H,W,3] (one chunk: the caller bounds V)."""
        x = _stacked(x).detach().float().contiguous()
        _lib.require_gpu(x)
        return self._forward(x, False, None, True)

    @torch.no_grad()
    def __call__(self, pred: Images, gt: Images, quantize_u8: bool = False, mask: Optional[Tensor] = None) -> Tensor:
        """LPIPS(pred, gt) [V].  quantize_u8: both images go through the evaluation's uint8 truncation / 255
        (metrics.eval_metrics_u8's); mask [V,H,W] multiplies the prediction before it (train.py:104-109)."""
        p, g, mask = self._prep(pred, gt, mask)
        V, H, W, _ = p.shape
        out = torch.zeros(V, dtype=torch.float32, device=p.device)
        for a, b in self._chunks(V, H, W):
            taps = self._gt_taps(g[a:b], quantize_u8)
            self._forward(p[a:b], quantize_u8, None if mask is None else mask[a:b], False,
                          lambda level, f: tap_dist(f, taps[level], self.lin[level], out[a:b], accumulate=True))
        return out

    @torch.no_grad()
    def value_and_grad(self, pred: Images, gt: Images, view_scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """(LPIPS [V], d_pred [V,H,W,3]) with d_pred[v] = view_scale[v] * d LPIPS_v / d pred (None: 1).  Nothing here
        is tracked by autograd: hand d_pred to `torch.autograd.backward(pred, d_pred)`."""
        p, g, _ = self._prep(pred, gt, None)
        V, H, W, _ = p.shape
        dev = p.device
        if view_scale is None:
            view_scale = torch.ones(V, dtype=torch.float32, device=dev)
        elif tuple(view_scale.shape) != (V,):
            raise ValueError(f"view_scale: expected [{V}], got {tuple(view_scale.shape)}")
        view_scale = view_scale.detach().to(device=dev, dtype=torch.float32).contiguous()
        bwd = self._bwd_packs()
        out = torch.zeros(V, dtype=torch.float32, device=dev)
        d_pred = torch.empty_like(p)
        for a, b in self._chunks(V, H, W):
            taps = self._gt_taps(g[a:b], False)
            acts = self._forward(p[a:b], False, None, True,
                                 lambda level, f: tap_dist(f, taps[level], self.lin[level], out[a:b], accumulate=True))
            dz = None
            for pos in reversed(range(13)):
                if pos in TAPS:
                    level = TAPS.index(pos)
                    f = acts[pos]
                    d = tap_dist_bwd(f, taps[level], self.lin[level], view_scale[a:b] / float(f.shape[1] * f.shape[2]),
                                     relu_mask=True)
                    if dz is not None:  # dz: the gradient of this tap's pooled map
                        maxpool2x2_bwd(f, dz, d, relu_mask=True)
                    dz = d
                cin, cout = CONV_CH[pos]
                mask_src = None if (pos == 0 or pos in POOL_BEFORE) else acts[pos - 1]
                dz = conv3x3(dz, bwd[pos], cin, mask_src=mask_src)
                acts[pos] = None
            lpips_input_bwd(dz, d_pred[a:b])
            del acts, taps, dz
        return out, d_pred


# ---- ops (one libsfx entry each) ----------------------------------------------------------------------------------
def conv_tile() -> Tuple[int, int]:
    """(rows, columns) of the MFMA convolution's pixel tile."""
    import ctypes as C
    th, tw = C.c_int(0), C.c_int(0)
    _lib.fn("sfx_conv3x3_tile")(C.addressof(th), C.addressof(tw))
    return th.value, tw.value


def pack_conv(w: Tensor, transpose_flip: bool = False) -> Tensor:
    """Pack torch Conv2d weights [Cout,Cin,3,3] for conv3x3; transpose_flip: for the layer's data backward (a
    convolution from Cout to Cin channels with the taps rotated by 180 degrees)."""
    _lib.require_gpu(w)
    w = w.detach().float().contiguous()
    cout, cin = (w.shape[1], w.shape[0]) if transpose_flip else (w.shape[0], w.shape[1])
    nbytes = int(_lib.fn("sfx_conv3x3_pack_bytes")(cin, cout))
    packed = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=w.device)
    call("sfx_conv3x3_pack", cin, cout, ptr(w), int(transpose_flip), ptr(packed), stream())
    return packed


def conv3x3(x: Tensor, packed: Tensor, cout: int, bias: Optional[Tensor] = None, relu: bool = False,
            mask_src: Optional[Tensor] = None) -> Tensor:
    """relu?(conv3x3(x) + bias) [* (mask_src > 0)] of x [V,H,W,Cin] with weights from pack_conv."""
    V, H, W, cin = x.shape
    y = torch.empty(V, H, W, cout, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(_lib.fn("sfx_conv3x3_workspace_bytes")(V)), dtype=torch.uint8, device=x.device)
    call("sfx_conv3x3", V, H, W, cin, cout, ptr(x, torch.float32), ptr(packed), ptr(bias), ptr(mask_src), int(relu),
         ptr(y), ptr(ws), ws.numel(), stream())
    return y


def maxpool2x2(x: Tensor) -> Tensor:
    V, H, W, C = x.shape
    y = torch.empty(V, H // 2, W // 2, C, dtype=torch.float32, device=x.device)
    call("sfx_maxpool2x2", V, H, W, C, ptr(x, torch.float32), ptr(y), stream())
    return y


def maxpool2x2_bwd(x: Tensor, dy: Tensor, dx: Tensor, relu_mask: bool = False) -> Tensor:
    """dx[first maximum of each 2x2 window of x] += dy, in place."""
    V, H, W, C = x.shape
    if tuple(dy.shape) != (V, H // 2, W // 2, C) or dx.shape != x.shape:
        raise ValueError("maxpool2x2_bwd: shapes do not match")
    call("sfx_maxpool2x2_bwd", V, H, W, C, ptr(x, torch.float32), ptr(dy, torch.float32), int(relu_mask),
         ptr(dx, torch.float32), stream())
    return dx


def lpips_input(x: Tensor, mask: Optional[Tensor] = None, quantize_u8: bool = False) -> Tensor:
    V, H, W, _ = x.shape
    u = torch.empty(V, H, W, 3, dtype=torch.float32, device=x.device)
    call("sfx_lpips_input", V, H, W, ptr(x, torch.float32), ptr(mask), int(quantize_u8), ptr(u), stream())
    return u


def lpips_input_bwd(du: Tensor, dx: Optional[Tensor] = None) -> Tensor:
    V, H, W, _ = du.shape
    dx = torch.empty_like(du) if dx is None else dx
    call("sfx_lpips_input_bwd", V, H, W, ptr(du, torch.float32), ptr(dx, torch.float32), stream())
    return dx


def tap_normalize(f: Tensor) -> Tensor:
    out = torch.empty_like(f)
    call("sfx_tap_normalize", f.numel() // f.shape[-1], f.shape[-1], ptr(f, torch.float32), ptr(out), stream())
    return out


def tap_dist(fx: Tensor, fhat_y: Tensor, w: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """out[v] (+)= mean_{h,w} sum_c w_c (fx^ - fhat_y)^2."""
    V, h, wd, C = fx.shape
    out = torch.empty(V, dtype=torch.float32, device=fx.device) if out is None else out
    ws = torch.empty(V * h * wd * 4, dtype=torch.uint8, device=fx.device)
    call("sfx_tap_dist", V, h * wd, C, ptr(fx, torch.float32), ptr(fhat_y, torch.float32), ptr(w, torch.float32),
         int(accumulate), ptr(out, torch.float32), ptr(ws), ws.numel(), stream())
    return out


def tap_dist_bwd(fx: Tensor, fhat_y: Tensor, w: Tensor, image_scale: Tensor, relu_mask: bool = False) -> Tensor:
    """image_scale[v] * d/d fx of the image's pixel sum of the tap distance."""
    V, h, wd, C = fx.shape
    dfx = torch.empty_like(fx)
    call("sfx_tap_dist_bwd", V, h * wd, C, ptr(fx, torch.float32), ptr(fhat_y, torch.float32), ptr(w, torch.float32),
         ptr(image_scale.contiguous(), torch.float32), int(relu_mask), ptr(dfx), stream())
    return dfx


# ---- autograd --------------------------------------------------------------------------------------------------
class _LpipsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, net):
        if ctx.needs_input_grad[0]:
            vals, ctx.d_pred = net.value_and_grad(pred, gt)
        else:
            vals, ctx.d_pred = net(pred, gt), None
        return vals

    @staticmethod
    def backward(ctx, grad_vals):
        return ctx.d_pred * grad_vals.reshape(-1, 1, 1, 1).to(ctx.d_pred.dtype), None, None


def lpips_loss(pred: Images, gt: Images, net: LPIPS) -> Tensor:
    """Per-view LPIPS [V], differentiable with respect to pred ([V,H,W,3], or a list of [H,W,3] that is stacked):
    the reference's loss_utils.lpips_loss_fn (train.py:269-282) on `net`'s frozen weights.  The forward keeps the
    derivative; the backward scales it by grad_out[v]."""
    return _LpipsLoss.apply(_stacked(pred), _stacked(gt), net)
