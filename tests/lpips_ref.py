"""fp64 restatement of the LPIPS(net='vgg') definition of splatformer_amd/lpips.py (test infrastructure; CPU torch).

`lpips` is the plain form (F.conv2d, F.max_pool2d).  `lpips_frozen` takes the discontinuous decisions as data: ReLU
is `z * mask`, pooling a gather at given indices -- with the decisions an fp32 implementation actually took, its
gradient is a smooth function that fp64 autograd pins without flakiness at units within rounding of 0.
Images are [V,H,W,3] in [0,1]; activations here are NCHW float64.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CONV_CH = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512),
           (512, 512), (512, 512), (512, 512), (512, 512))
SLICES = ((0, 2), (5, 7), (10, 12, 14), (17, 19, 21), (24, 26, 28))
POOL_BEFORE = (2, 4, 7, 10)
TAPS = (1, 3, 6, 9, 12)
TAP_CH = (64, 128, 256, 512, 512)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def make_weights(seed: int = 0):
    """Seeded fp32 weights: conv N(0, 2 / (9 Cin)), bias N(0, 0.1^2), lin U[0, 1)."""
    g = torch.Generator().manual_seed(seed)
    convs = []
    for cin, cout in CONV_CH:
        w = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
        convs.append((w, torch.randn(cout, generator=g) * 0.1))
    lins = [torch.rand(c, generator=g) for c in TAP_CH]
    return convs, lins


def package_state_dict(convs, lins, duplicates: bool = True, scaling: bool = True) -> dict:
    """The key layout of one lpips.LPIPS(net='vgg') state dict."""
    sd = {}
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor(SHIFT).view(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(SCALE).view(1, 3, 1, 1)
    for pos, idx in enumerate(CONV_IDX):
        s = next(i for i, sl in enumerate(SLICES) if idx in sl) + 1
        sd[f"net.slice{s}.{idx}.weight"], sd[f"net.slice{s}.{idx}.bias"] = convs[pos]
    for l, w in enumerate(lins):
        sd[f"lin{l}.model.1.weight"] = w.view(1, -1, 1, 1)
        if duplicates:
            sd[f"lins.{l}.model.1.weight"] = w.view(1, -1, 1, 1)
    return sd


def torchvision_state_dicts(convs, lins) -> Tuple[dict, dict]:
    """(torchvision VGG16 state dict, the package's vgg.pth)."""
    feats = {}
    for pos, idx in enumerate(CONV_IDX):
        feats[f"features.{idx}.weight"], feats[f"features.{idx}.bias"] = convs[pos]
    feats["classifier.0.bias"] = torch.zeros(4)  # (the classifier's keys ride along unused)
    return feats, {f"lin{l}.model.1.weight": w.view(1, -1, 1, 1) for l, w in enumerate(lins)}


def input_stage(x: torch.Tensor) -> torch.Tensor:
    """[V,H,W,3] -> u [V,3,H,W] float64."""
    t = 2.0 * x.double().permute(0, 3, 1, 2) - 1.0
    return (t - torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)) / \
        torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)


def quantize_u8(x: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The evaluation's quantisation in the fp32 steps the reference takes: p * m, (p * 255).to(uint8) / 255."""
    p = x.float()
    if mask is not None:
        p = p * mask.float().unsqueeze(-1)
    q = (p * torch.tensor(255.0)).to(torch.int32).clamp(0, 255)
    return q.float() / torch.tensor(255.0)


def first_max_index(a: torch.Tensor) -> torch.Tensor:
    """Flat (h * W + w) index of the first maximum, in row-major window order, of every 2x2 / stride 2 window of
    a [V,C,H,W] (floor: an odd last row / column belongs to no window) -> int64 [V,C,H//2,W//2]."""
    V, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    oy = torch.arange(Ho).view(Ho, 1) * 2
    ox = torch.arange(Wo).view(1, Wo) * 2
    best = a[:, :, 0:2 * Ho:2, 0:2 * Wo:2]
    idx = (oy * W + ox).expand(V, C, Ho, Wo).clone()
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        v = a[:, :, dy:2 * Ho:2, dx:2 * Wo:2]
        take = v > best
        best = torch.where(take, v, best)
        idx = torch.where(take, ((oy + dy) * W + ox + dx).expand_as(idx), idx)
    return idx


def pool_gather(a: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    return a.flatten(2).gather(2, idx.flatten(2)).view_as(idx)


def features(u: torch.Tensor, convs, masks: Optional[Sequence[torch.Tensor]] = None,
             pool_idx: Optional[Sequence[torch.Tensor]] = None):
    """-> (13 post-ReLU activations, 13 pre-activations).  masks / pool_idx: the frozen decisions (13 masks
    [V,C,h,w], 4 index maps as first_max_index gives); None: the plain network."""
    acts, pres = [], []
    cur = u
    k = 0
    for pos, (w, b) in enumerate(convs):
        if pos in POOL_BEFORE:
            cur = F.max_pool2d(cur, 2) if pool_idx is None else pool_gather(cur, pool_idx[k])
            k += 1
        z = F.conv2d(cur, w.double(), b.double(), padding=1)
        cur = torch.relu(z) if masks is None else z * masks[pos].to(z.dtype)
        pres.append(z)
        acts.append(cur)
    return acts, pres


def normalize(f: torch.Tensor) -> torch.Tensor:
    return f / (f.square().sum(1, keepdim=True).sqrt() + 1e-10)


def tap_distance(fx: torch.Tensor, fy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[V,C,h,w] x 2, w [C] -> [V]: mean over pixels of sum_c w_c (fx^ - fy^)^2."""
    d = (normalize(fx) - normalize(fy)).square() * w.double().view(1, -1, 1, 1)
    return d.sum(1).mean((1, 2))


def decisions(acts: Sequence[torch.Tensor]):
    """(masks, pool indices) that a list of 13 post-ReLU NCHW activations took."""
    return [a > 0 for a in acts], [first_max_index(acts[p - 1]) for p in POOL_BEFORE]


def lpips(x: torch.Tensor, y: torch.Tensor, convs, lins) -> torch.Tensor:
    fx, _ = features(input_stage(x), convs)
    fy, _ = features(input_stage(y), convs)
    return sum(tap_distance(fx[p], fy[p], lins[l]) for l, p in enumerate(TAPS))


def lpips_frozen(x: torch.Tensor, y: torch.Tensor, convs, lins, masks, pool_idx) -> torch.Tensor:
    """LPIPS with x's ReLU and pool decisions supplied (y's branch is the plain network)."""
    fx, _ = features(input_stage(x), convs, masks, pool_idx)
    fy, _ = features(input_stage(y), convs)
    return sum(tap_distance(fx[p], fy[p], lins[l]) for l, p in enumerate(TAPS))
