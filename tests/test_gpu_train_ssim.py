"""Trainer with the fused L1 + D-SSIM loss (Trainer(ssim_loss_weight > 0), losses.image_loss_and_grad), in both
render modes, against the CPU oracle on the images the refined scene renders to.

Set-up as tests/test_gpu_train.py::test_trainer_step_runs_and_updates (3000 Gaussians, SH degree 1, 2 views of
64 x 64), with the DropPath masks and order shuffles fixed as tests/test_gpu_render_views_bwd.py fixes them, so the
refined scene can be rendered a second time.  Loss bar 4e-4: both render forwards are within the project's 2e-4
image bar of the oracle and the loss is a weighted mean of absolute image differences and of an SSIM in [-1, 1]
(the argument of test_gpu_render_views_bwd.py:363-365).
"""
import pytest
import torch

from oracle import metrics_ref
from splatformer_amd import losses
from splatformer_amd import train as strain
from splatformer_amd.feature_predictor import FeaturePredictor
from splatformer_amd.gs_render import rasterize_gaussians_to_multiimgs, rasterize_packed_to_multiimgs_batched
from splatformer_amd.scenes import make_cameras, make_scene, to_device

pytestmark = pytest.mark.gpu

W_L1, W_SSIM = 0.8, 0.2
PERMS = [[0, 1, 2, 3]] * 5


class _FixedMasks:
    """DropPath masks from a seeded CPU generator: the same sequence for every trainer built with the same seed."""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, name, n, p, device=None):
        if p <= 0.0:
            return None
        keep = 1.0 - p
        return ((torch.rand(n, generator=self.g) < keep).float() / keep).to(device)


@pytest.fixture(scope="module")
def setup(device):
    torch.manual_seed(0)
    sd0 = FeaturePredictor(sh_degree=1, zeroinit=False).state_dict()
    s = to_device(make_scene(3000, 1, seed=2), device)
    cams = to_device(make_cameras(64, 64, n_views=2), device)
    gt = [torch.rand(64, 64, 3, generator=torch.Generator().manual_seed(v)).to(device) for v in range(2)]
    return sd0, s, cams, gt


def _trainer(sd0, device, **kw):
    model = FeaturePredictor(sh_degree=1, zeroinit=False)
    model.load_state_dict(sd0)
    model = model.to(device)
    return model, strain.Trainer(model, lr=1e-3, **kw)


def _render_again(model, mode, s, cams):
    """The refined scene of the same masks and shuffles, rendered without grad by the mode's own forward."""
    with torch.no_grad():
        packed, _ = strain.refine_train(model, s, _FixedMasks(5), perms=PERMS)
        if mode == "batched":
            extra = {k: v for k, v in s.items()}
            preds, _ = rasterize_packed_to_multiimgs_batched(packed, model.columns(), cams, extra=extra)
        else:
            _, out_gs = strain.unpack_leaf(model, packed, s)
            preds, _ = rasterize_gaussians_to_multiimgs({k: v.detach() for k, v in out_gs.items()}, cams)
    return torch.stack(list(preds), 0).cpu()


def test_trainer_ssim_loss_both_render_modes(device, setup):
    sd0, s, cams, gt = setup
    g = torch.stack(gt, 0).cpu()
    out = {}
    for mode in ("per_view", "batched"):
        model, tr = _trainer(sd0, device, render=mode, ssim_loss_weight=W_SSIM, image_l1_loss_weight=W_L1)
        assert tr.last_metrics is None
        loss = tr.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
        grad = tr.flat_grad.clone()
        metrics = {k: float(v) for k, v in tr.last_metrics.items()}
        assert all(v.is_cuda for v in tr.last_metrics.values())
        p = _render_again(model, mode, s, cams)
        l1 = (p - g).abs().reshape(2, -1).mean(1)
        ssim = metrics_ref.ssim(p.permute(0, 3, 1, 2), g.permute(0, 3, 1, 2), 11, size_average=False)
        want = float((W_L1 * l1 + W_SSIM * (1.0 - ssim)).sum()) / 2 / 1 / 1  # / num_images / scenes / accumulate
        psnr = float(metrics_ref.psnr(p, g).mean())
        print(f"\n[{mode}] loss {loss:.6f} (oracle {want:.6f}), train_psnr {metrics['train_psnr']:.4f} "
              f"(oracle {psnr:.4f}), ssim {metrics['ssim']:.5f}, image_l1 {metrics['image_l1']:.5f}")
        assert abs(loss - want) <= 4e-4
        assert abs(metrics["train_psnr"] - psnr) <= 1e-3
        assert abs(metrics["image_l1"] - float(l1.mean())) <= 4e-4
        assert abs(metrics["ssim"] - float(ssim.mean())) <= 4e-4
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
        # the same L1 weight without the SSIM term: another gradient
        _, tr0 = _trainer(sd0, device, render=mode, ssim_loss_weight=0.0, image_l1_loss_weight=W_L1)
        tr0.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
        assert tr0.last_metrics is None
        diff = float((grad - tr0.flat_grad).norm() / tr0.flat_grad.norm())
        print(f"[{mode}] |grad - grad(L1 only)| / |grad(L1 only)| = {diff:.3f}")
        assert diff > 1e-2
        out[mode] = loss
    assert abs(out["per_view"] - out["batched"]) <= 4e-4, out


def test_zero_ssim_weight_runs_the_torch_l1_path(device, setup, monkeypatch):
    sd0, s, cams, gt = setup
    calls = []
    for name in ("image_loss", "image_loss_and_grad", "_run"):
        fn = getattr(losses, name)
        monkeypatch.setattr(losses, name, lambda *a, _fn=fn, _n=name, **kw: (calls.append(_n), _fn(*a, **kw))[1])
    _, tr = _trainer(sd0, device, ssim_loss_weight=0.0)
    loss = tr.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert calls == [] and tr.last_metrics is None
    _, tr_default = _trainer(sd0, device)
    assert tr_default.image_l1_loss_weight == 1.0 and tr_default.ssim_loss_weight == 0.0
    want = tr_default.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert abs(loss - want) <= 1e-6 * abs(want)
    # the L1 weight scales that loss
    _, tr_half = _trainer(sd0, device, image_l1_loss_weight=0.5)
    half = tr_half.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert abs(half - 0.5 * want) <= 1e-6 * abs(want)
    assert calls == []
    # and the spy does count: the fused path goes through losses
    _, tr_ssim = _trainer(sd0, device, ssim_loss_weight=0.2)
    tr_ssim.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert "image_loss_and_grad" in calls


def test_negative_weights_raise(device, setup):
    sd0 = setup[0]
    model = FeaturePredictor(sh_degree=1, zeroinit=False)
    model.load_state_dict(sd0)
    model = model.to(device)
    with pytest.raises(ValueError, match="ssim_loss_weight"):
        strain.Trainer(model, ssim_loss_weight=-0.1)
    with pytest.raises(ValueError, match="image_l1_loss_weight"):
        strain.Trainer(model, image_l1_loss_weight=-1.0)
