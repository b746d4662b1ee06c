"""Fused masked evaluation metrics (sfx_eval_metrics_u8, metrics.eval_metrics_u8, evaluate_scenes on RGBA targets)
vs torch on the CPU and the oracle restatements of train.py:104-113 + utils/metrics.py.

Shapes: a single pixel, 16 x 16 (half a 32 x 16 tile), one pixel over a tile edge in each axis, a height below the
window radius with several tiles across, several tiles in both axes, 130 x 97, and exactly one tile -- the
smallest sizes at which tiling, halo, zero padding and the image edges can go wrong.

Bars.  Integer moments and maxima: equality -- both sides do the same two IEEE fp32 multiplies and a truncation.
PSNR: 1e-4 dB against the oracle's float32 mean (the bar of test_gpu_metrics.py; the HIP side is exact integers).
SSIM: 2e-6 against the reference formula evaluated in float64 on the same quantised images (the reference's own
float32 evaluation stays within 1.3e-7 of that on these inputs, so the bar is not met by a shared rounding; the
kernel measured 2.8e-8)."""
import functools
import json

import pytest
import torch

from oracle import gsplat_ref, metrics_ref
from splatformer_amd import metrics

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (2, 16, 16), (2, 17, 33), (1, 5, 70), (3, 64, 48), (2, 130, 97)]
# mask kind -> composite the target through it?
KINDS = {"blob": True, "random": True, "ones": False, "zeros": True}
# an uncomposited target under a zero mask; a prediction whose quantised max is <= 1; exactly one 32 x 16 tile
EXTRA = [((2, 17, 33), "zeros_raw"), ((3, 64, 48), "tiny"), ((1, 16, 32), "blob")]
CASES = [(s, k) for s in SHAPES for k in KINDS] + EXTRA
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{k}" for s, k in CASES]


def blob_mask(V, H, W):
    """A smooth ellipse with a soft edge, each value k / 255 as scene_io.read_image produces."""
    y = torch.arange(H, dtype=torch.float32).view(1, H, 1) / max(H - 1, 1)
    x = torch.arange(W, dtype=torch.float32).view(1, 1, W) / max(W - 1, 1)
    cx = 0.45 + 0.05 * torch.arange(V, dtype=torch.float32).view(V, 1, 1)
    d = torch.sqrt(((x - cx) / 0.38) ** 2 + ((y - 0.5) / 0.3) ** 2)
    k = torch.round(((1.0 - d) / 0.25 + 0.5).clamp(0, 1) * 255)
    return k / 255.0


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """CPU inputs and the expected quantised images and integer moments; computed once, never modified."""
    V, H, W = shape
    g = torch.Generator().manual_seed(1000 * H + W + len(kind))
    gt = torch.rand(V, H, W, 3, generator=g)
    pred = (gt + 0.05 * torch.randn(V, H, W, 3, generator=g)).clamp_min(0) * 1.02  # some values > 1
    n = pred.numel()
    pred.view(-1)[0 % n] = 1.0
    pred.view(-1)[(n // 2 + 1) % n] = 0.0
    gt.view(-1)[1 % n] = 1.0
    gt.view(-1)[(n // 3 + 2) % n] = 0.0
    if kind == "blob":
        m = blob_mask(V, H, W)
    elif kind == "random":
        m = torch.randint(0, 256, (V, H, W), generator=g).float() / 255.0
    elif kind == "ones":
        m = torch.ones(V, H, W)
    elif kind == "tiny":
        m = torch.full((V, H, W), 1.0) / 255.0
    else:
        m = torch.zeros(V, H, W)
    gt3 = gt * m[..., None] if KINDS.get(kind, False) else gt
    pm = pred.clamp(max=1.0) * m[..., None]
    pu = (pm * 255).to(torch.uint8)
    gu = (gt3 * 255).to(torch.uint8)
    a, b = pu.to(torch.int64).reshape(V, -1), gu.to(torch.int64).reshape(V, -1)
    sums = torch.stack([(a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1)
    maxes = torch.stack([a.max(1).values, b.max(1).values], 1).to(torch.int32)
    rgba = torch.cat([gt3, m[..., None]], -1).contiguous()
    return dict(pred=pred, gt3=gt3.contiguous(), mask=m, rgba=rgba, pm=pm, pu=pu, gu=gu, sums=sums, maxes=maxes)


@functools.lru_cache(maxsize=None)
def ssim64(shape, kind):
    c = case(shape, kind)
    q = lambda u: u.float().div(255).permute(0, 3, 1, 2).double()  # noqa: E731
    return metrics_ref.ssim(q(c["pu"]), q(c["gu"]), 11, size_average=False)


@functools.lru_cache(maxsize=None)
def run(shape, kind, dev):
    c = case(shape, kind)
    out = metrics.eval_metrics_u8(c["pred"].to(dev), c["rgba"].to(dev))
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_integer_moments_and_maxima_are_exact(device, shape, kind):
    c, got = case(shape, kind), run(shape, kind, str(device))
    assert got["sums"].dtype == torch.int64 and got["maxes"].dtype == torch.int32
    assert torch.equal(got["sums"], c["sums"]), (got["sums"], c["sums"])
    assert torch.equal(got["maxes"], c["maxes"]), (got["maxes"], c["maxes"])


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_psnr_matches_oracle(device, shape, kind):
    c, got = case(shape, kind), run(shape, kind, str(device))
    want = gsplat_ref.psnr_u8(c["pm"], c["gt3"]).reshape(-1).double()
    print(f"psnr {shape} {kind}: got {got['psnr'].tolist()} want {want.tolist()}")
    assert got["psnr"].dtype == torch.float64 and got["psnr"].shape == want.shape
    assert torch.allclose(got["psnr"], want, atol=1e-4, rtol=0)
    if kind == "zeros":  # an all-zero mask over a composited target: both images are zero
        assert torch.isinf(got["psnr"]).all() and (got["psnr"] > 0).all()
    if kind == "tiny":  # the masked prediction is NOT divided by 255 (metrics.py:26-29), the target is
        assert int(c["maxes"][:, 0].max()) <= 1 < int(c["maxes"][:, 1].max())
        assert torch.isfinite(got["psnr"]).all()


@pytest.mark.parametrize("shape,kind", CASES, ids=IDS)
def test_ssim_matches_float64_reference(device, shape, kind):
    got, want = run(shape, kind, str(device))["ssim"], ssim64(shape, kind)
    err = float((got.double() - want).abs().max())
    print(f"ssim {shape} {kind}: max |hip - ref64| = {err:.3e}")
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert err <= 2e-6
    if kind == "zeros":
        assert torch.equal(got, torch.ones_like(got))


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s in SHAPES])
def test_unmasked_agrees_with_the_existing_kernels(device, shape):
    """An RGB target without a mask: the integer moments torch forms on the CPU, the float64 SSIM, and the same bits
    as the RGBA form with an all-ones mask and as the thin callers psnr_u8 / image_stats_u8 / ssim(quantize_u8)."""
    c = case(shape, "ones")
    pred, gt3 = c["pred"].to(device), c["gt3"].to(device)
    got = metrics.eval_metrics_u8(pred, gt3)
    assert torch.equal(got["sums"].cpu(), c["sums"]) and torch.equal(got["maxes"].cpu(), c["maxes"])
    assert float((got["ssim"].cpu().double() - ssim64(shape, "ones")).abs().max()) <= 2e-6
    assert torch.equal(got["psnr"], metrics.psnr_u8(pred, gt3))
    sums, maxes = metrics.image_stats_u8(pred, gt3)
    assert torch.equal(got["sums"], sums) and torch.equal(got["maxes"], maxes)
    assert torch.equal(got["ssim"], metrics.ssim(pred, gt3, quantize_u8=True))
    ones = run(shape, "ones", str(device))  # the same target as RGBA with an all-ones mask
    assert torch.equal(ones["sums"], got["sums"].cpu()) and torch.equal(ones["ssim"], got["ssim"].cpu())


@pytest.mark.parametrize("shape,kind", [((2, 17, 33), "blob"), ((1, 5, 70), "random"), ((2, 130, 97), "blob"),
                                        ((1, 1, 1), "random")])
def test_in_place_mask_equals_separate_mask_and_calls_repeat(device, shape, kind):
    c = case(shape, kind)
    pred, rgba = c["pred"].to(device), c["rgba"].to(device)
    keep = rgba.clone()
    a = metrics.eval_metrics_u8(pred, rgba)
    assert torch.equal(rgba, keep)  # consumed in place, not modified
    b = metrics.eval_metrics_u8(pred, rgba[..., :3].contiguous(), mask=rgba[..., 3].contiguous())
    d = metrics.eval_metrics_u8(pred, rgba, mask=rgba[..., 3:].contiguous())  # stride-4 target, dense [V,H,W,1] mask
    again = metrics.eval_metrics_u8(pred, rgba)
    for other in (b, d, again):
        for k in ("sums", "maxes", "ssim", "psnr"):
            assert torch.equal(a[k], other[k]), k


def test_clamp_pred_off_saturates_like_the_existing_kernel(device):
    """clamp_pred=False leaves values above 1 to the truncation (below 256 / 255) and the uint8 saturation (above).
    Without a mask the clamp cannot show in the moments (a value above 1 quantises to 255 either way), so each form
    is held to what torch forms on the CPU from the same quantisation, and the two agree; under a mask the clamp
    comes before the multiply (p = 1.2, m = 0.5: 153 unclamped, 127 clamped), and the two sets of moments differ."""
    c = case((2, 17, 33), "random")
    pred = c["pred"].clone()
    pred[:, ::3, ::2] *= 1.3  # values in (1, 256 / 255) and well above: up to 1.02 * 1.3 * 1.2
    gt3, ones = c["gt3"], torch.ones_like(c["mask"])
    assert int((pred > 256 / 255).sum()) > 100 and int(((pred > 1) & (pred * 255 < 256)).sum()) > 0

    def moments(p, m):  # saturating, as the kernel documents: torch's own uint8 conversion wraps above 255
        a = ((p * m[..., None]) * 255).to(torch.int64).clamp(0, 255).reshape(2, -1)
        b = c["gu"].to(torch.int64).reshape(2, -1)
        return (torch.stack([(a * a).sum(1), (b * b).sum(1), (a * b).sum(1)], 1),
                torch.stack([a.max(1).values, b.max(1).values], 1).to(torch.int32))

    assert not torch.equal(moments(pred, c["mask"])[0], moments(pred.clamp(max=1.0), c["mask"])[0])
    assert torch.equal(moments(pred, ones)[0], moments(pred.clamp(max=1.0), ones)[0])
    on_dev = pred.to(device), gt3.to(device)
    for clamp in (False, True):
        p = pred.clamp(max=1.0) if clamp else pred
        got = metrics.eval_metrics_u8(*on_dev, clamp_pred=clamp)  # an RGB target, no mask
        sums, maxes = moments(p, ones)
        assert torch.equal(got["sums"].cpu(), sums) and torch.equal(got["maxes"].cpu(), maxes), clamp
        s2, m2 = metrics.image_stats_u8(*on_dev, clamp_pred=clamp)
        assert torch.equal(got["sums"], s2) and torch.equal(got["maxes"], m2)
        got = metrics.eval_metrics_u8(*on_dev, mask=c["mask"].to(device), clamp_pred=clamp)
        sums, maxes = moments(p, c["mask"])
        assert torch.equal(got["sums"].cpu(), sums) and torch.equal(got["maxes"].cpu(), maxes), clamp


def test_empty_batch(device):
    got = metrics.eval_metrics_u8(torch.zeros(0, 8, 8, 3, device=device), torch.zeros(0, 8, 8, 4, device=device))
    assert got["psnr"].shape == (0,) and got["ssim"].shape == (0,) and got["sums"].shape == (0, 3)


def test_evaluate_scenes_on_real_style_targets(device, tmp_path):
    """Scene 0 has an RGBA target (render + noise composited through a blob mask, the mask as channel 4), scene 1
    a plain RGB one.  evaluate_input=True keeps the check deterministic (the refiner's order shuffle draws from the
    global RNG on every forward)."""
    from splatformer_amd.evaluate import evaluate_scenes, write_metrics
    from splatformer_amd.feature_predictor import FeaturePredictor
    from splatformer_amd.gs_render import rasterize_gaussians_to_multiimgs
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    torch.manual_seed(0)
    model = FeaturePredictor(sh_degree=1, zeroinit=False).eval().to(device)
    scenes = [to_device(make_scene(3000, sh_degree=1, seed=s), device) for s in range(2)]
    cams = [to_device(make_cameras(64, 64, n_views=3), device) for _ in range(2)]
    noise = torch.Generator().manual_seed(1)
    renders = []
    for s in range(2):
        with torch.no_grad():
            rgbs, _ = rasterize_gaussians_to_multiimgs(scenes[s], cams[s])
        renders.append(torch.stack(rgbs, 0).cpu())
    noisy = [(r + 0.02 * torch.rand(3, 64, 64, 3, generator=noise)).clamp(0, 1) for r in renders]
    m = blob_mask(3, 64, 64)
    targets = [torch.cat([noisy[0] * m[..., None], m[..., None]], -1), noisy[1]]
    on_dev = [t.to(device) for t in targets]

    results = {}
    got = evaluate_scenes(model, scenes, cams, lambda i: on_dev[i], device, evaluate_input=True, results=results)
    q = lambda x: (x * 255).to(torch.uint8).float().div(255.0).permute(0, 3, 1, 2)  # noqa: E731
    masked = renders[0].clamp(max=1) * m[..., None]
    want_psnr = torch.cat([gsplat_ref.psnr_u8(masked, targets[0][..., :3]).reshape(-1),
                           gsplat_ref.psnr_u8(renders[1], targets[1]).reshape(-1)]).double()
    want_ssim = torch.cat([metrics_ref.ssim(q(masked), q(targets[0][..., :3]), 11, size_average=False),
                           metrics_ref.ssim(q(renders[1].clamp(max=1)), q(targets[1]), 11, size_average=False)])
    assert got["num_images"] == 6 and got["num_scenes"] == 2
    assert got["psnr"] == pytest.approx(float(want_psnr.mean()), abs=1e-4)
    assert got["ssim"] == pytest.approx(float(want_ssim.double().mean()), abs=2e-6)
    assert sorted(results) == ["0", "1"]
    for name in results:
        assert sorted(results[name]) == ["psnr", "ssim"]
        assert all(len(results[name][k]) == 3 and all(isinstance(v, float) for v in results[name][k])
                   for k in ("psnr", "ssim"))
    for k in ("psnr", "ssim"):
        assert sum(results["0"][k] + results["1"][k]) / 6 == pytest.approx(got[k], abs=1e-12)
    path = tmp_path / "metrics.rank0.json"
    write_metrics(results, str(path))
    assert json.loads(path.read_text()) == results

    alone = {}
    evaluate_scenes(model, scenes[1:], cams[1:], lambda i: on_dev[1], device, evaluate_input=True, results=alone,
                    names=["second"])
    assert alone == {"second": results["1"]}  # the 3-channel path is untouched by a masked neighbour

    both, inp = {}, {}
    refined = evaluate_scenes(model, scenes, cams, lambda i: on_dev[i], device, compare_with_input=True,
                              results=both, results_input=inp)
    assert refined["psnr_input"] == got["psnr"] and refined["ssim_input"] == got["ssim"]
    assert inp == results and sorted(both) == ["0", "1"]
    assert refined["num_images"] == 6
    assert all(v == v and abs(v) != float("inf") for v in (refined["psnr"], refined["ssim"]))


def test_evaluate_scenes_scores_rgb_and_all_ones_rgba_alike(device):
    """Two scenes with the same pixels, one scored against an RGB target and one against that target as RGBA with an
    all-ones mask: one path, so the per-image records are equal as floats."""
    from splatformer_amd.evaluate import evaluate_scenes
    from splatformer_amd.gs_render import rasterize_gaussians_to_multiimgs
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    scene = to_device(make_scene(2000, sh_degree=1, seed=3), device)
    cams = to_device(make_cameras(40, 33, n_views=2), device)
    with torch.no_grad():
        rgbs, _ = rasterize_gaussians_to_multiimgs(scene, cams)
    render = torch.stack(rgbs, 0).cpu()
    rgb = (render + 0.03 * torch.rand(render.shape, generator=torch.Generator().manual_seed(5))).clamp(0, 1)
    targets = [rgb.to(device), torch.cat([rgb, torch.ones_like(rgb[..., :1])], -1).to(device)]
    results = {}
    evaluate_scenes(None, [scene, scene], [cams, cams], lambda i: targets[i], device, evaluate_input=True,
                    results=results)
    assert results["0"] == results["1"]
    assert len(results["0"]["psnr"]) == 2 and all(v == v and v < 100 for v in results["0"]["psnr"])
    assert all(0 < v < 1 for v in results["0"]["ssim"])
