"""Host side of the fused L1 + D-SSIM training loss (no GPU needed).

* The closed-form derivative csrc/loss.hip implements, restated in fp64 torch (`ssim_grad_closed_form`), against
  autograd through the oracle's SSIM: relative L2 <= 1e-10 (fp64 rounding of two different evaluation orders; it
  measures <= 2e-13).  This pins the formula without a device.
* sfx_image_loss validates its arguments before any launch.
* The additions leave the ABI number at 16, and the Trainer has the two loss-weight keywords.

`make_inputs`, `oracle_loss_and_grad` and `ssim_grad_closed_form` are shared with tests/test_gpu_image_loss.py.
"""
import inspect

import pytest
import torch
import torch.nn.functional as F

from oracle import metrics_ref

C1, C2 = 0.01 ** 2, 0.03 ** 2
SHAPES = [(1, 1, 1, 3), (2, 3, 4, 3), (2, 17, 33, 1), (3, 37, 50, 3)]   # [V, H, W, C]


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def make_inputs(shape, kind, seed=0):
    """(pred, gt) [V,H,W,C] fp32 on the CPU.  noise: gt uniform, pred = gt + 0.05 randn clamped to [0,1]; indep: two
    independent uniform images; flat: gt = 1, pred = 1 - 0.02 rand (white background: e11 - mu1^2 cancels)."""
    g = torch.Generator().manual_seed(seed * 1000003 + shape[1] * 131 + shape[2] * 7 + shape[3])
    if kind == "noise":
        gt = torch.rand(shape, generator=g)
        pred = (gt + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    elif kind == "indep":
        gt = torch.rand(shape, generator=g)
        pred = torch.rand(shape, generator=g)
    elif kind == "flat":
        gt = torch.ones(shape)
        pred = 1 - 0.02 * torch.rand(shape, generator=g)
    else:
        raise ValueError(kind)
    return pred, gt


def upstream(V, dtype=torch.float64):
    """A non-uniform upstream gradient / view scale (fp32-representable values)."""
    return (0.25 + 0.375 * torch.arange(V, dtype=torch.float32)).to(dtype)


def oracle_loss_and_grad(pred, gt, l1_weight, ssim_weight, up, dtype):
    """Per-view terms and d(sum_v up[v] * loss_v)/d pred by autograd through oracle.metrics_ref.ssim, evaluated in
    `dtype` on the CPU.  pred/gt: [V,H,W,C].  -> (l1 [V], ssim [V], mse [V], grad [V,H,W,C])."""
    p = pred.to(dtype).clone().requires_grad_()
    g = gt.to(dtype)
    V = p.shape[0]
    ssim = metrics_ref.ssim(p.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2), 11, size_average=False)
    l1 = (p - g).abs().reshape(V, -1).mean(1)
    mse = ((p - g) ** 2).reshape(V, -1).mean(1)
    loss = l1_weight * l1 + ssim_weight * (1.0 - ssim)
    (loss * up.to(dtype)).sum().backward()
    return l1.detach(), ssim.detach(), mse.detach(), p.grad


def ssim_grad_closed_form(pred, gt, up):
    """d(sum_v up[v] * SSIM_v)/d pred in fp64 by the closed form of csrc/loss.hip: the five windowed moments, the
    SSIM map m = A1 A2 / (B1 B2), its partial derivatives with respect to mu1, e11 and e12, and the adjoint of the
    (symmetric, zero-padded) window applied to each.  -> (SSIM [V], grad [V,H,W,C])."""
    p = pred.double().permute(0, 3, 1, 2)
    g = gt.double().permute(0, 3, 1, 2)
    V, C, H, W = p.shape
    w = metrics_ref._window(11, C).double()
    conv = lambda x: F.conv2d(x, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2, e11, e22, e12 = conv(p), conv(g), conv(p * p), conv(g * g), conv(p * g)
    A1 = 2 * mu1 * mu2 + C1
    A2 = 2 * (e12 - mu1 * mu2) + C2
    B1 = mu1 ** 2 + mu2 ** 2 + C1
    B2 = (e11 - mu1 ** 2) + (e22 - mu2 ** 2) + C2
    m = A1 * A2 / (B1 * B2)
    G = 1.0 / (C * H * W)
    d_mu1 = 2 * mu2 * (A2 - A1) / (B1 * B2) - 2 * mu1 * m / B1 + 2 * mu1 * m / B2
    d_e11 = -m / B2
    d_e12 = 2 * A1 / (B1 * B2)
    d = conv(G * d_mu1) + 2 * p * conv(G * d_e11) + g * conv(G * d_e12)
    d = d * up.double().view(V, 1, 1, 1)
    return m.mean((1, 2, 3)), d.permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("kind", ["noise", "indep", "flat"])
@pytest.mark.parametrize("shape", SHAPES)
def test_closed_form_derivative_matches_autograd(shape, kind):
    pred, gt = make_inputs(shape, kind)
    up = upstream(shape[0])
    _, ssim, _, grad = oracle_loss_and_grad(pred, gt, 0.0, 1.0, up, torch.float64)
    s, d = ssim_grad_closed_form(pred, gt, up)
    assert float((s - ssim).abs().max()) <= 1e-12
    err = rel_l2(-d, grad)  # the loss term is 1 - SSIM
    print(f"\n[{shape} {kind}] closed form vs fp64 autograd: rel-L2 {err:.2e}")
    assert err <= 1e-10


# ---- the C entry validates on the host ---------------------------------------------------------------------------
P = 1 << 20  # a non-null, 8-byte aligned address that is never dereferenced: every call below is refused first


def _lib():
    from splatformer_amd import _lib
    return _lib.load()


def _call(lib, V=2, H=8, W=8, C=3, pred=P, gt=2 * P, window=3 * P, l1=1.0, ssim=0.2, scale=None, terms=4 * P,
          d_pred=5 * P, ws=6 * P, ws_bytes=1 << 30):
    return lib.sfx_image_loss(V, H, W, C, pred, gt, window, l1, ssim, scale, terms, d_pred, ws, ws_bytes, None)


def test_entries_declared_and_abi_unchanged():
    from splatformer_amd import _lib as L
    lib = _lib()
    for name in ("sfx_image_loss", "sfx_image_loss_workspace_bytes"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert len(L.SIGNATURES["sfx_image_loss"]) == 15
    assert lib.sfx_abi_version() == 17


@pytest.mark.parametrize("kw,word", [
    (dict(V=-1), b"bad sizes"), (dict(H=0), b"bad sizes"), (dict(W=0), b"bad sizes"), (dict(C=0), b"bad sizes"),
    (dict(V=30000, C=3), b"65535"),                       # V * C above one grid dimension
    (dict(V=1, H=2 ** 21, W=2 ** 21, C=1), b"bad sizes"),  # more than 2^40 elements
    (dict(V=1, H=16 * 65535 + 1, W=1, C=1), b"height"),
    (dict(pred=None), b"null buffer"), (dict(gt=None), b"null buffer"), (dict(window=None), b"null buffer"),
    (dict(terms=None), b"null buffer"), (dict(ws=None), b"null buffer"),
    (dict(ws=6 * P + 4), b"aligned"),
    (dict(ws_bytes=8), b"workspace too small"),
    (dict(l1=-1.0), b"negative"), (dict(ssim=-0.5), b"negative"), (dict(ssim=float("nan")), b"negative"),
    (dict(d_pred=P), b"aliases"), (dict(d_pred=2 * P + 4), b"aliases"),
])
def test_bad_arguments_are_refused_before_any_launch(kw, word):
    lib = _lib()
    rc = _call(lib, **kw)
    assert rc < 0
    msg = lib.sfx_last_error()
    assert b"sfx_image_loss" in msg and word in msg, msg


def test_workspace_sizes():
    lib = _lib()
    V, H, W, C = 2, 17, 33, 3
    tiles = ((W + 31) // 32) * ((H + 15) // 16)
    full = lib.sfx_image_loss_workspace_bytes(V, H, W, C)
    assert full == 24 * V * C * tiles + 12 * V * H * W * C
    assert lib.sfx_image_loss_workspace_bytes(V, 0, W, C) == 0
    # forward only (d_pred NULL) and L1 only need the tile sums alone; with d_pred and SSIM the maps as well
    sums = 24 * V * C * tiles
    for kw in (dict(d_pred=None, ws_bytes=sums - 1), dict(ssim=0.0, ws_bytes=sums - 1), dict(ws_bytes=full - 1)):
        assert _call(lib, V=V, H=H, W=W, C=C, **kw) < 0
        assert b"workspace too small" in lib.sfx_last_error()


def test_python_wrappers_refuse_cpu_tensors_and_negative_weights():
    from splatformer_amd import losses
    x = torch.rand(1, 4, 4, 3)
    with pytest.raises(RuntimeError):
        losses.image_loss(x, x)
    with pytest.raises(RuntimeError):
        losses.image_loss_and_grad([x[0]], [x[0]], 1.0, 0.2, None)
    from splatformer_amd import metrics
    t = metrics.gaussian_taps()
    assert torch.equal(metrics.ssim_window(), t[:, None].mm(t[None, :]))
    assert t.dtype == torch.float32 and t.shape == (11,)
    assert torch.equal(t[:, None].mm(t[None, :]), metrics_ref._window(11, 1)[0, 0])  # the reference's window


def test_trainer_has_the_loss_weight_keywords():
    from splatformer_amd.train import Trainer
    prm = inspect.signature(Trainer.__init__).parameters
    assert prm["image_l1_loss_weight"].default == 1.0
    assert prm["ssim_loss_weight"].default == 0.0
