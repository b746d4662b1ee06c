"""LPIPS(net='vgg') on the GPU (splatformer_amd/lpips.py, csrc/lpips.hip) against the fp64 restatement
tests/lpips_ref.py, on seeded weights.

Bars are the project's own: rel-L2 <= 1e-5 for values (README), <= 1e-4 for gradients; the whole
network's value |hip - ref64| <= 1e-5 ref64 per image.

Whole-network gradient: ReLU and pool decisions are discontinuous, and a unit whose fp64 pre-activation is within
rounding of 0 may legitimately flip in fp32 (one flip moves d_pred by about 1e-3 rel-L2), so a plain autograd
comparison would be flaky for any fp32 implementation.  Instead the decisions the GPU took (forward_with_tape)
(1) may differ from the fp64 ones only at units with |z_ref| <= 1e-4 rms(z_ref of the layer), and (2) d_pred is
compared with fp64 autograd through the frozen-decision restatement under those decisions.

Shapes (V,H,W): (1,16,16) -- conv5 is 1x1, all 8 neighbours padding; (2,35,52) -- odd sizes at every pool, two
images (a leak across the image boundary shows); (1, 2 TH + 1, TW + 1) -- one pixel past the conv kernel's pixel tile
in each direction (the whole network needs H >= 16, so two tile rows + 1); the per-op conv runs (2, TH + 1, TW + 1).
"""
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from splatformer_amd import lpips as L

pytestmark = pytest.mark.gpu

CLASSES = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512)]


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(0)


@pytest.fixture(scope="module")
def net(device, weights):
    return L.LPIPS(*weights, device=device)


def conv_shape():
    th, tw = L.conv_tile()
    return 2, th + 1, tw + 1


def net_shapes():
    th, tw = L.conv_tile()
    return [(1, 16, 16), (2, 35, 52), (1, max(16, 2 * th + 1), max(16, tw + 1))]


def class_weights(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    return w, torch.randn(cout, generator=g) * 0.1, g


# ---- per op --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", CLASSES)
def test_conv_forward(device, cin, cout):
    """Two images of very different magnitude (the activation scale is per image), bias + ReLU."""
    V, H, W = conv_shape()
    w, b, g = class_weights(cin, cout, cin * 1000 + cout)
    x = torch.randn(V, H, W, cin, generator=g)
    x[1] *= 300.0
    ref = torch.relu(F.conv2d(nchw(x).double(), w.double(), b.double(), padding=1))
    packed = L.pack_conv(w.to(device))
    y = L.conv3x3(x.to(device), packed, cout, bias=b.to(device), relu=True)
    assert y.shape == (V, H, W, cout)
    errs = [rel_l2(nchw(y.cpu())[v], ref[v]) for v in range(V)]
    print(f"\nconv {cin}->{cout} forward, {V}x{H}x{W}: rel-L2 per image {errs[0]:.2e} {errs[1]:.2e}")
    assert max(errs) <= 1e-5
    y2 = L.conv3x3(x.to(device), packed, cout, bias=b.to(device), relu=True)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 2, 3), (1, 16, 33)])
def test_conv_forward_small_and_wide_maps(device, shape):
    """512 -> 512 on 1x1 (every neighbour is padding), 2x3, and a map of two tile rows by three tile columns."""
    V, H, W = shape
    w, b, g = class_weights(512, 512, 7)
    x = torch.randn(V, H, W, 512, generator=g)
    ref = F.conv2d(nchw(x).double(), w.double(), b.double(), padding=1)
    y = L.conv3x3(x.to(device), L.pack_conv(w.to(device)), 512, bias=b.to(device), relu=False)
    err = rel_l2(nchw(y.cpu()), ref)
    print(f"\nconv 512->512 forward {shape}: rel-L2 {err:.2e}")
    assert err <= 1e-5


def test_conv_other_channel_counts_run_the_general_valu_kernel(device):
    """Channel counts outside the MFMA classes and the two first-layer kernels (here 5 -> 7, forward and backward)."""
    V, H, W = conv_shape()
    w, b, g = class_weights(5, 7, 57)
    x = torch.randn(V, H, W, 5, generator=g)
    ref = torch.relu(F.conv2d(nchw(x).double(), w.double(), b.double(), padding=1))
    y = L.conv3x3(x.to(device), L.pack_conv(w.to(device)), 7, bias=b.to(device), relu=True)
    assert rel_l2(nchw(y.cpu()), ref) <= 1e-5
    dz = torch.randn(V, H, W, 7, generator=g)
    xr = torch.zeros(V, 5, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), None, padding=1).backward(nchw(dz).double())
    got = L.conv3x3(dz.to(device), L.pack_conv(w.to(device), transpose_flip=True), 5, mask_src=x.to(device))
    assert rel_l2(nchw(got.cpu()), xr.grad * (nchw(x) > 0)) <= 1e-4


@pytest.mark.parametrize("cin,cout", CLASSES)
def test_conv_backward_with_mask(device, cin, cout):
    """d a_prev's pre-activation of a = relu(conv(a_prev)): the transposed, rotated weights, masked by a_prev > 0
    (the first layer's input is no ReLU output: no mask there)."""
    V, H, W = conv_shape()
    w, _, g = class_weights(cin, cout, cin * 1000 + cout + 1)
    dz = torch.randn(V, H, W, cout, generator=g) * 1e-4
    dz[1] *= 50.0
    a_prev = torch.randn(V, H, W, cin, generator=g).clamp_min(0)
    x = torch.zeros(V, cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, padding=1).backward(nchw(dz).double())
    ref = x.grad if cin == 3 else x.grad * (nchw(a_prev) > 0)
    got = L.conv3x3(dz.to(device), L.pack_conv(w.to(device), transpose_flip=True), cin,
                    mask_src=None if cin == 3 else a_prev.to(device))
    err = rel_l2(nchw(got.cpu()), ref)
    print(f"\nconv {cin}->{cout} data backward: rel-L2 {err:.2e}")
    assert err <= 1e-4
    if cin != 3:
        assert bool((got.cpu()[a_prev <= 0] == 0).all())


@pytest.mark.parametrize("shape", [(2, 9, 17, 64), (1, 2, 2, 512), (2, 35, 52, 64), (1, 3, 3, 128)])
def test_pool_forward_and_backward(device, shape):
    V, H, W, C = shape
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(shape, generator=g)
    y = L.maxpool2x2(x.to(device))
    xr = nchw(x).double().requires_grad_()
    yr = F.max_pool2d(xr, 2)
    assert torch.equal(nchw(y.cpu()).double(), yr.detach())
    dy = torch.randn(V, H // 2, W // 2, C, generator=g)
    yr.backward(nchw(dy).double())
    g0 = torch.randn(shape, generator=g)  # the gradient already in dx (the tap's)
    dx = g0.clone().to(device)
    L.maxpool2x2_bwd(x.to(device), dy.to(device), dx)
    err = rel_l2(nchw(dx.cpu()), nchw(g0).double() + xr.grad)
    print(f"\npool backward {shape}: rel-L2 {err:.2e}")
    assert err <= 1e-4
    # ReLU-masked form, on a ReLU output (ties at 0 get nothing) -- first maximum in row-major order
    a = x.clamp_min(0)
    dx = torch.zeros(shape).to(device)
    L.maxpool2x2_bwd(a.to(device), dy.to(device), dx, relu_mask=True)
    idx = R.first_max_index(nchw(a))
    want = torch.zeros(V, C, H * W, dtype=torch.float64)
    want.scatter_(2, idx.flatten(2), (nchw(dy).double() * (R.pool_gather(nchw(a), idx) > 0)).flatten(2))
    assert rel_l2(nchw(dx.cpu()).flatten(2), want) <= 1e-4


@pytest.mark.parametrize("shape", [(2, 5, 7, 64), (1, 1, 1, 512), (2, 9, 4, 256)])
def test_tap_distance_forward_and_backward(device, shape):
    V, h, w, C = shape
    g = torch.Generator().manual_seed(C + h)
    fx = torch.randn(shape, generator=g).clamp_min(0)
    fy = torch.randn(shape, generator=g).clamp_min(0)
    lin = torch.rand(C, generator=g)
    up = torch.tensor([0.25, 0.625])[:V]
    xr = nchw(fx).double().requires_grad_()
    ref = R.tap_distance(xr, nchw(fy).double(), lin)
    (ref * up.double()).sum().backward()
    fhy = L.tap_normalize(fy.to(device))
    assert rel_l2(nchw(fhy.cpu()), R.normalize(nchw(fy).double())) <= 1e-5
    out = L.tap_dist(fx.to(device), fhy, lin.to(device))
    err = float(((out.cpu().double() - ref.detach()).abs() / ref.detach()).max())
    out2 = L.tap_dist(fx.to(device), fhy, lin.to(device), out=out.clone(), accumulate=True)
    assert torch.equal(out2, out + out)
    d = L.tap_dist_bwd(fx.to(device), fhy, lin.to(device), (up / (h * w)).to(device))
    dm = L.tap_dist_bwd(fx.to(device), fhy, lin.to(device), (up / (h * w)).to(device), relu_mask=True)
    gerr = rel_l2(nchw(d.cpu()), xr.grad)
    gmerr = rel_l2(nchw(dm.cpu()), xr.grad * (nchw(fx) > 0))
    print(f"\ntap distance {shape}: value rel {err:.2e}, gradient rel-L2 {gerr:.2e}, masked {gmerr:.2e}")
    assert err <= 1e-5 and gerr <= 1e-4 and gmerr <= 1e-4


def test_input_stage(device):
    V, H, W = 2, 16, 17
    g = torch.Generator().manual_seed(3)
    x = torch.rand(V, H, W, 3, generator=g) * 1.2 - 0.1   # some values below 0 and above 1
    x[0, 0, :, 0] = torch.arange(W) / 255.0               # exact k / 255 boundaries
    mask = (torch.rand(V, H, W, generator=g) > 0.3).float() * torch.rand(V, H, W, generator=g)
    u = L.lpips_input(x.to(device))
    assert rel_l2(nchw(u.cpu()), R.input_stage(x)) <= 1e-5
    shift, scale = torch.tensor(R.SHIFT).double(), torch.tensor(R.SCALE).double()
    for m in (None, mask):
        q = R.quantize_u8(x, m)
        u = L.lpips_input(x.to(device), mask=None if m is None else m.to(device), quantize_u8=True).cpu()
        assert rel_l2(nchw(u), R.input_stage(q)) <= 1e-5
        level = ((u.double() * scale + shift) + 1.0) / 2.0 * 255.0   # the uint8 level the kernel chose
        assert torch.equal(level.round(), (q.double() * 255.0).round())
        assert float((level - level.round()).abs().max()) < 1e-3
    um = L.lpips_input(x.to(device), mask=mask.to(device)).cpu()
    assert rel_l2(nchw(um), R.input_stage(x * mask[..., None])) <= 1e-5
    du = torch.randn(V, H, W, 3, generator=g)
    dx = L.lpips_input_bwd(du.to(device)).cpu()
    assert rel_l2(dx, du.double() * 2.0 / scale) <= 1e-6


# ---- whole network ------------------------------------------------------------------------------------------------------
_CASES = {}


def network_case(shape, net, weights, device):
    """Inputs, GPU results (twice) and the fp64 reference of a shape, computed once."""
    if shape in _CASES:
        return _CASES[shape]
    convs, lins = weights
    V, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W)
    gt = torch.rand(V, H, W, 3, generator=g)
    pred = (gt + 0.1 * torch.randn(V, H, W, 3, generator=g)).clamp(0, 1)
    up = (0.25 + 0.375 * torch.arange(V, dtype=torch.float32))
    p, t = pred.to(device), gt.to(device)
    val = net(p, t)
    val_g, d_pred = net.value_and_grad(p, t, view_scale=up.to(device))
    val_g2, d_pred2 = net.value_and_grad(p, t, view_scale=up.to(device))
    tape = [nchw(a.cpu()) for a in net.forward_with_tape(p)]
    ref = R.lpips(pred, gt, convs, lins)
    c = dict(pred=pred, gt=gt, up=up, val=val.cpu(), val_g=val_g.cpu(), d_pred=d_pred.cpu(), val_g2=val_g2.cpu(),
             d_pred2=d_pred2.cpu(), val2=net(p, t).cpu(), tape=tape, ref=ref)
    _CASES[shape] = c
    return c


@pytest.mark.parametrize("shape", net_shapes())
def test_network_value(device, net, weights, shape):
    c = network_case(shape, net, weights, device)
    err = ((c["val"].double() - c["ref"]).abs() / c["ref"]).tolist()
    print(f"\nLPIPS {shape}: ref {c['ref'].tolist()}, relative error per image {err}")
    assert c["val"].shape == (shape[0],)
    assert max(err) <= 1e-5
    assert torch.equal(c["val"], c["val_g"])  # the metric path and the loss path are the same arithmetic


@pytest.mark.parametrize("shape", net_shapes())
def test_network_two_calls_give_equal_bits(device, net, weights, shape):
    c = network_case(shape, net, weights, device)
    assert torch.equal(c["val"], c["val2"]) and torch.equal(c["val_g"], c["val_g2"])
    assert torch.equal(c["d_pred"], c["d_pred2"])


@pytest.mark.parametrize("shape", net_shapes())
def test_network_gradient_under_the_decisions_taken(device, net, weights, shape):
    convs, lins = weights
    c = network_case(shape, net, weights, device)
    acts, pres = R.features(R.input_stage(c["pred"]), convs)
    masks, idx = R.decisions(c["tape"])
    flips = 0
    for pos in range(13):
        differs = masks[pos] != (pres[pos] > 0)
        flips += int(differs.sum())
        if bool(differs.any()):
            rms = float(pres[pos].square().mean().sqrt())
            worst = float(pres[pos][differs].abs().max())
            assert worst <= 1e-4 * rms, f"conv {R.CONV_IDX[pos]}: a flipped unit has |z_ref| = {worst:.3e}, rms {rms:.3e}"
        assert rel_l2(c["tape"][pos], acts[pos]) <= 1e-5, f"activation of conv {R.CONV_IDX[pos]}"
    x = c["pred"].double().requires_grad_()
    val = R.lpips_frozen(x, c["gt"], convs, lins, masks, idx)
    (val * c["up"].double()).sum().backward()
    err = rel_l2(c["d_pred"], x.grad)
    print(f"\nLPIPS gradient {shape}: {flips} flipped units, d_pred rel-L2 {err:.2e} (|d_pred| {float(x.grad.norm()):.3e})")
    assert c["d_pred"].shape == c["pred"].shape
    assert err <= 1e-4


def test_views_are_chunked(device, net, weights):
    """A chunk bound of one image gives the bits of the unchunked call (images never mix)."""
    c = network_case((2, 35, 52), net, weights, device)
    p, t = c["pred"].to(device), c["gt"].to(device)
    small = L.LPIPS(*weights, device=device)
    small.max_chunk_pixels = 35 * 52
    assert len(small._chunks(2, 35, 52)) == 2
    v, d = small.value_and_grad(p, t, view_scale=c["up"].to(device))
    assert torch.equal(v.cpu(), c["val_g"]) and torch.equal(d.cpu(), c["d_pred"])
    assert torch.equal(small(p, t).cpu(), c["val"])


def test_lpips_loss_autograd_and_refusals(device, net, weights):
    c = network_case((1, 16, 16), net, weights, device)
    p = c["pred"].to(device).requires_grad_()
    loss = L.lpips_loss([p[0]], [c["gt"].to(device)[0]], net)
    (loss * 0.25).sum().backward()
    assert torch.equal(loss.detach().cpu(), c["val_g"])
    assert torch.equal(p.grad.cpu(), c["d_pred"])  # up[0] = 0.25
    with pytest.raises(ValueError, match="at least 16"):
        net(torch.zeros(1, 15, 16, 3, device=device), torch.zeros(1, 15, 16, 3, device=device))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3))


# ---- Trainer ---------------------------------------------------------------------------------------------------------------
PERMS = [[0, 1, 2, 3]] * 5


class _FixedMasks:
    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, name, n, p, device=None):
        if p <= 0.0:
            return None
        keep = 1.0 - p
        return ((torch.rand(n, generator=self.g) < keep).float() / keep).to(device)


@pytest.fixture(scope="module")
def train_setup(device):
    from splatformer_amd.feature_predictor import FeaturePredictor
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    torch.manual_seed(0)
    sd0 = FeaturePredictor(sh_degree=1, zeroinit=False).state_dict()
    s = to_device(make_scene(3000, 1, seed=2), device)
    cams = to_device(make_cameras(64, 64, n_views=2), device)
    gt = [torch.rand(64, 64, 3, generator=torch.Generator().manual_seed(v)).to(device) for v in range(2)]
    return sd0, s, cams, gt


def _trainer(sd0, device, **kw):
    from splatformer_amd import train as strain
    from splatformer_amd.feature_predictor import FeaturePredictor
    model = FeaturePredictor(sh_degree=1, zeroinit=False)
    model.load_state_dict(sd0)
    model = model.to(device)
    return model, strain.Trainer(model, lr=1e-3, **kw)


def _spy_on_the_step(monkeypatch, mode, gt, net, ssim_weight):
    """Wrap the trainer's render call: on the images that very step rendered (two renders of one scene differ in
    their last bits, which is enough to flip a ReLU of the VGG stack and move the gradient by 1e-3), assemble
    image_l1 (or the fused image loss) + lpips_loss through autograd and take its gradient at the step's own leaf,
    through the step's own graph.  -> dict filled during micro_step: loss, lpips, grad; and leaf_grad, what the
    trainer handed to refine_backward."""
    from splatformer_amd import losses
    from splatformer_amd import train as strain
    cap = {}
    real_unpack, real_rb = strain.unpack_leaf, strain.refine_backward
    name = "rasterize_packed_to_multiimgs_batched" if mode == "batched" else "rasterize_gaussians_to_multiimgs"
    real_render = getattr(strain, name)

    def unpack_spy(fp, packed, gs):
        leaf, out = real_unpack(fp, packed, gs)
        cap["leaf"] = leaf
        return leaf, out

    def render_spy(*a, **kw):
        preds, alphas = real_render(*a, **kw)
        leaf = a[0] if mode == "batched" else cap["leaf"]
        base = losses.image_loss(preds, gt, 1.0, ssim_weight).sum() if ssim_weight > 0 else strain.image_l1(preds, gt)
        lp = L.lpips_loss(preds, gt, net)
        loss = (base + lp.sum()) / 2  # / num_images / scenes / accumulate_step
        cap["grad"] = torch.autograd.grad(loss, leaf, retain_graph=True)[0].clone()
        cap["loss"], cap["lpips"] = float(loss.detach()), float(lp.detach().mean())
        return preds, alphas

    monkeypatch.setattr(strain, "unpack_leaf", unpack_spy)
    monkeypatch.setattr(strain, name, render_spy)
    monkeypatch.setattr(strain, "refine_backward",
                        lambda fp, tape, d: (cap.__setitem__("leaf_grad", d.clone()), real_rb(fp, tape, d))[1])
    return cap


@pytest.mark.parametrize("mode", ["per_view", "batched"])
@pytest.mark.parametrize("ssim_weight", [0.0, 0.2])
def test_trainer_step_with_the_lpips_term(device, train_setup, net, monkeypatch, mode, ssim_weight):
    """The step's loss and the gradient that reaches the refined record (leaf.grad) equal image_l1 (or the fused
    L1 + D-SSIM) plus lpips_loss through autograd on the same step's images (_spy_on_the_step).  Bars: 1e-6 relative
    on the loss (the forward has one order); the project's gradient bar, rel-L2 1e-4, on leaf.grad:
    the two sides are two runs of the render backward on image gradients that differ by fp32 association (the fused
    path adds the two derivative maps before it, autograd after).  Measured 4e-9 .. 7e-9."""
    sd0, s, cams, gt = train_setup
    cap = _spy_on_the_step(monkeypatch, mode, gt, net, ssim_weight)
    model, tr = _trainer(sd0, device, render=mode, lpips_loss_weight=1.0, lpips=net, ssim_loss_weight=ssim_weight)
    loss = tr.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert "lpips" in tr.last_metrics and tr.last_metrics["lpips"].is_cuda
    assert ("ssim" in tr.last_metrics) == (ssim_weight > 0)
    err = rel_l2(cap["leaf_grad"], cap["grad"])
    print(f"\n[{mode}, ssim {ssim_weight}] loss {loss:.7f} (assembled {cap['loss']:.7f}), lpips {cap['lpips']:.5f}, "
          f"leaf.grad rel-L2 {err:.2e}")
    assert abs(loss - cap["loss"]) <= 1e-6 * abs(cap["loss"])
    assert abs(float(tr.last_metrics["lpips"]) - cap["lpips"]) <= 1e-6 * cap["lpips"]
    assert err <= 1e-4
    assert bool(torch.isfinite(tr.flat_grad).all()) and float(tr.flat_grad.abs().max()) > 0
    assert not any("lpips" in k for k in tr.state_dict())
    assert all(p.requires_grad is False for p in net.w + net.b + net.lin)


def test_zero_lpips_weight_is_todays_step(device, train_setup, net, monkeypatch):
    """Weight 0 (the default) never touches the LPIPS object and runs the statements the step ran before.  Two runs
    of one step are not bit-equal here (two renders of one scene differ in their last bits: the leaf gradients of
    two such steps measured 2e-5 apart), so the comparison with the default trainer carries the bars two runs of
    one step get: 1e-6 on the loss (tests/test_gpu_train_ssim.py) and the project's gradient bar, rel-L2 1e-4, on
    the flat gradient."""
    sd0, s, cams, gt = train_setup
    calls = []
    for name in ("value_and_grad", "__call__"):
        fn = getattr(L.LPIPS, name)
        monkeypatch.setattr(L.LPIPS, name, lambda *a, _fn=fn, _n=name, **kw: (calls.append(_n), _fn(*a, **kw))[1])
    _, tr = _trainer(sd0, device, lpips_loss_weight=0.0, lpips=net)
    loss = tr.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    _, tr0 = _trainer(sd0, device)
    want = tr0.micro_step([s], [cams], [gt], masks=_FixedMasks(5), perms=PERMS)
    assert calls == [] and tr.last_metrics is None and tr0.lpips_loss_weight == 0.0
    assert abs(loss - want) <= 1e-6 * abs(want)
    assert rel_l2(tr.flat_grad, tr0.flat_grad) <= 1e-4


# ---- evaluate_scenes ------------------------------------------------------------------------------------------------------
def test_evaluate_scenes_with_lpips(device, net):
    from splatformer_amd.evaluate import evaluate_scenes
    from splatformer_amd.feature_predictor import FeaturePredictor
    from splatformer_amd.gs_render import rasterize_gaussians_to_multiimgs
    from splatformer_amd.scenes import make_cameras, make_scene, to_device
    torch.manual_seed(0)
    model = FeaturePredictor(sh_degree=1, zeroinit=False).eval().to(device)
    scenes = [to_device(make_scene(3000, sh_degree=1, seed=s), device) for s in range(2)]
    cams = [to_device(make_cameras(64, 64, n_views=2), device) for _ in range(2)]
    noise = torch.Generator().manual_seed(1)
    renders = []
    for s in range(2):
        with torch.no_grad():
            rgbs, _ = rasterize_gaussians_to_multiimgs(scenes[s], cams[s])
        renders.append(torch.stack(rgbs, 0).cpu())
    noisy = [(r + 0.05 * torch.rand(2, 64, 64, 3, generator=noise)).clamp(0, 1) for r in renders]
    m = (torch.rand(2, 64, 64, generator=noise) > 0.4).float()
    targets = [torch.cat([noisy[0] * m[..., None], m[..., None]], -1), noisy[1]]   # RGBA, RGB
    on_dev = [t.to(device) for t in targets]

    plain, res_plain = evaluate_scenes(model, scenes, cams, lambda i: on_dev[i], device, evaluate_input=True), {}
    evaluate_scenes(model, scenes, cams, lambda i: on_dev[i], device, evaluate_input=True, results=res_plain)
    res, res_in = {}, {}
    got = evaluate_scenes(model, scenes, cams, lambda i: on_dev[i], device, evaluate_input=True, results=res,
                          compare_with_input=True, results_input=res_in, lpips=net)
    assert sorted(plain) == ["num_images", "num_scenes", "psnr", "ssim"]
    assert sorted(got) == ["lpips", "lpips_input", "num_images", "num_scenes", "psnr", "psnr_input", "ssim",
                           "ssim_input"]
    assert all(sorted(res_plain[k]) == ["psnr", "ssim"] and sorted(res[k]) == ["lpips", "psnr", "ssim"] for k in res)
    for k in res:  # today's columns are untouched
        assert res[k]["psnr"] == res_plain[k]["psnr"] and res[k]["ssim"] == res_plain[k]["ssim"]
    assert got["psnr"] == plain["psnr"] and got["ssim"] == plain["ssim"] and got["lpips_input"] == got["lpips"]
    assert res_in == res
    # LPIPS(quantised pred, quantised gt); the RGBA target's mask multiplies the prediction
    q_rgba = net(R.quantize_u8(renders[0], m).to(device), R.quantize_u8(targets[0][..., :3]).to(device)).cpu()
    q_rgb = net(R.quantize_u8(renders[1]).to(device), R.quantize_u8(targets[1]).to(device)).cpu()
    assert res["0"]["lpips"] == q_rgba.double().tolist() and res["1"]["lpips"] == q_rgb.double().tolist()
    assert got["lpips"] == pytest.approx(float(torch.cat([q_rgba, q_rgb]).double().mean()), abs=1e-12)
    assert all(v > 0 for v in res["0"]["lpips"] + res["1"]["lpips"])
