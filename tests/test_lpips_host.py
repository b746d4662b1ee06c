"""Host side of LPIPS (no GPU needed): the weight loader, the argument refusals of every csrc/lpips.hip entry, the
Trainer keyword, and the fp64 restatement's own consistency (tests/lpips_ref.py, shared with
tests/test_gpu_lpips.py).
"""
import inspect

import pytest
import torch

import lpips_ref as R
from splatformer_amd import lpips as L


@pytest.fixture(scope="module")
def weights():
    return R.make_weights(0)


# ---- loader -------------------------------------------------------------------------------------------------------
def test_both_key_layouts_load_equal_tensors(weights, tmp_path):
    convs, lins = weights
    one = R.package_state_dict(convs, lins)
    feats, lin = R.torchvision_state_dicts(convs, lins)
    a = L.parse_state_dict(one)
    b = L.parse_state_dict(feats, lin)
    assert len(a[0]) == len(b[0]) == 13 and len(a[1]) == len(b[1]) == 5
    for (wa, ba), (wb, bb), (w0, b0) in zip(a[0], b[0], convs):
        assert torch.equal(wa, wb) and torch.equal(ba, bb) and torch.equal(wa, w0) and torch.equal(ba, b0)
    for la, lb, l0 in zip(a[1], b[1], lins):
        assert torch.equal(la, lb) and torch.equal(la, l0) and la.dim() == 1
    # through files, loaded with weights_only=True
    torch.save(one, tmp_path / "one.pth")
    sd = torch.load(tmp_path / "one.pth", map_location="cpu", weights_only=True)
    c = L.parse_state_dict(sd)
    assert all(torch.equal(x[0], y[0]) for x, y in zip(a[0], c[0]))
    src = inspect.getsource(L.LPIPS.from_files)
    assert src.count("weights_only=True") == 2


def test_lins_duplicates_are_ignored(weights):
    convs, lins = weights
    with_dup = R.package_state_dict(convs, lins, duplicates=True)
    for l in range(5):  # a duplicate that disagrees must not matter
        with_dup[f"lins.{l}.model.1.weight"] = torch.full_like(with_dup[f"lins.{l}.model.1.weight"], 7.0)
    a = L.parse_state_dict(with_dup)
    b = L.parse_state_dict(R.package_state_dict(convs, lins, duplicates=False, scaling=False))
    assert all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def _package_keys():
    convs, lins = R.make_weights(0)
    return [k for k in R.package_state_dict(convs, lins, duplicates=False, scaling=False)]


@pytest.mark.parametrize("key", _package_keys())
def test_missing_or_misshaped_package_key_is_named(weights, key):
    convs, lins = weights
    sd = R.package_state_dict(convs, lins)
    bad = dict(sd)
    del bad[key]
    with pytest.raises(KeyError, match=key.replace(".", r"\.")):
        L.parse_state_dict(bad)
    bad = dict(sd)
    bad[key] = sd[key].reshape(-1)[:-1].clone()
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        L.parse_state_dict(bad)


def test_missing_or_misshaped_two_file_key_is_named(weights):
    convs, lins = weights
    feats, lin = R.torchvision_state_dicts(convs, lins)
    for key in [k for k in feats if k.startswith("features.")]:
        bad = dict(feats)
        del bad[key]
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            L.parse_state_dict(bad, lin)
        bad = dict(feats)
        bad[key] = feats[key].reshape(-1)[:-1].clone()
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            L.parse_state_dict(bad, lin)
    for key in lin:
        bad = dict(lin)
        del bad[key]
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            L.parse_state_dict(feats, bad)
        bad = dict(lin)
        bad[key] = lin[key].reshape(-1)
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            L.parse_state_dict(feats, bad)


def test_a_scaling_layer_that_disagrees_is_refused(weights):
    convs, lins = weights
    sd = R.package_state_dict(convs, lins)
    sd["scaling_layer.scale"] = torch.tensor([0.5, 0.5, 0.5]).view(1, 3, 1, 1)
    with pytest.raises(ValueError, match=r"scaling_layer\.scale"):
        L.parse_state_dict(sd)


# ---- the C entries validate on the host -------------------------------------------------------------------------------
P = 1 << 20  # a non-null, 16-byte aligned address that is never dereferenced: every call below is refused first
BIG = 1 << 30


def _lib():
    from splatformer_amd import _lib
    return _lib.load()


def _conv(lib, V=1, H=8, W=8, cin=64, cout=64, x=P, packed=2 * P, bias=None, mask=None, relu=1, y=3 * P, ws=4 * P,
          ws_bytes=BIG):
    return lib.sfx_conv3x3(V, H, W, cin, cout, x, packed, bias, mask, relu, y, ws, ws_bytes, None)


CASES = [
    ("sfx_conv3x3", lambda lib: _conv(lib, V=0), b"bad sizes"),
    ("sfx_conv3x3", lambda lib: _conv(lib, H=0), b"bad sizes"),
    ("sfx_conv3x3", lambda lib: _conv(lib, W=-3), b"bad sizes"),
    ("sfx_conv3x3", lambda lib: _conv(lib, cin=0), b"bad sizes"),
    ("sfx_conv3x3", lambda lib: _conv(lib, cout=0), b"bad sizes"),
    ("sfx_conv3x3", lambda lib: _conv(lib, V=14, H=800, W=800), b"2 GiB"),
    ("sfx_conv3x3", lambda lib: _conv(lib, x=None), b"null buffer"),
    ("sfx_conv3x3", lambda lib: _conv(lib, packed=None), b"null buffer"),
    ("sfx_conv3x3", lambda lib: _conv(lib, y=None), b"null buffer"),
    ("sfx_conv3x3", lambda lib: _conv(lib, ws=None), b"null buffer"),
    ("sfx_conv3x3", lambda lib: _conv(lib, ws=4 * P + 4), b"aligned"),
    ("sfx_conv3x3", lambda lib: _conv(lib, x=P + 8), b"aligned"),
    ("sfx_conv3x3", lambda lib: _conv(lib, V=5, ws_bytes=16), b"workspace too small"),
    ("sfx_conv3x3", lambda lib: _conv(lib, y=P), b"aliases"),
    ("sfx_conv3x3_pack", lambda lib: lib.sfx_conv3x3_pack(0, 64, P, 0, 2 * P, None), b"bad channel"),
    ("sfx_conv3x3_pack", lambda lib: lib.sfx_conv3x3_pack(64, -1, P, 0, 2 * P, None), b"bad channel"),
    ("sfx_conv3x3_pack", lambda lib: lib.sfx_conv3x3_pack(64, 64, None, 0, 2 * P, None), b"null buffer"),
    ("sfx_conv3x3_pack", lambda lib: lib.sfx_conv3x3_pack(64, 64, P, 1, None, None), b"null buffer"),
    ("sfx_conv3x3_pack", lambda lib: lib.sfx_conv3x3_pack(64, 64, P, 1, 2 * P + 4, None), b"aligned"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(0, 8, 8, 64, P, 2 * P, None), b"bad sizes"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(1, 1, 8, 64, P, 2 * P, None), b"bad sizes"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(1, 8, 8, 6, P, 2 * P, None), b"bad sizes"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(14, 800, 800, 64, P, 2 * P, None), b"2 GiB"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(1, 8, 8, 64, None, 2 * P, None), b"null buffer"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(1, 8, 8, 64, P, None, None), b"null buffer"),
    ("sfx_maxpool2x2", lambda lib: lib.sfx_maxpool2x2(1, 8, 8, 64, P + 4, 2 * P, None), b"aligned"),
    ("sfx_maxpool2x2_bwd", lambda lib: lib.sfx_maxpool2x2_bwd(1, 8, 0, 64, P, 2 * P, 0, 3 * P, None), b"bad sizes"),
    ("sfx_maxpool2x2_bwd", lambda lib: lib.sfx_maxpool2x2_bwd(14, 800, 800, 64, P, 2 * P, 0, 3 * P, None), b"2 GiB"),
    ("sfx_maxpool2x2_bwd", lambda lib: lib.sfx_maxpool2x2_bwd(1, 8, 8, 64, P, None, 0, 3 * P, None), b"null buffer"),
    ("sfx_maxpool2x2_bwd", lambda lib: lib.sfx_maxpool2x2_bwd(1, 8, 8, 64, P, 2 * P, 0, P, None), b"aliases"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(0, 16, 16, P, None, 0, 2 * P, None), b"bad image count"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(1, 15, 16, P, None, 0, 2 * P, None), b"at least 16"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(1, 16, 15, P, None, 0, 2 * P, None), b"at least 16"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(100, 2048, 2048, P, None, 0, 2 * P, None), b"2 GiB"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(1, 16, 16, None, None, 0, 2 * P, None), b"null buffer"),
    ("sfx_lpips_input", lambda lib: lib.sfx_lpips_input(1, 16, 16, P, None, 1, None, None), b"null buffer"),
    ("sfx_lpips_input_bwd", lambda lib: lib.sfx_lpips_input_bwd(1, 0, 16, P, 2 * P, None), b"bad sizes"),
    ("sfx_lpips_input_bwd", lambda lib: lib.sfx_lpips_input_bwd(100, 2048, 2048, P, 2 * P, None), b"2 GiB"),
    ("sfx_lpips_input_bwd", lambda lib: lib.sfx_lpips_input_bwd(1, 16, 16, None, 2 * P, None), b"null buffer"),
    ("sfx_tap_normalize", lambda lib: lib.sfx_tap_normalize(0, 64, P, 2 * P, None), b"bad sizes"),
    ("sfx_tap_normalize", lambda lib: lib.sfx_tap_normalize(1 << 24, 64, P, 2 * P, None), b"2 GiB"),
    ("sfx_tap_normalize", lambda lib: lib.sfx_tap_normalize(4, 64, P, None, None), b"null buffer"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(0, 4, 64, P, 2 * P, 3 * P, 0, 4 * P, 5 * P, BIG, None), b"bad sizes"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(1, 0, 64, P, 2 * P, 3 * P, 0, 4 * P, 5 * P, BIG, None), b"bad sizes"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(2, 1 << 23, 64, P, 2 * P, 3 * P, 0, 4 * P, 5 * P, BIG, None),
     b"2 GiB"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(1, 4, 64, P, None, 3 * P, 0, 4 * P, 5 * P, BIG, None), b"null buffer"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(1, 4, 64, P, 2 * P, 3 * P, 0, 4 * P, None, BIG, None), b"null buffer"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(1, 4, 64, P, 2 * P, 3 * P, 0, 4 * P, 5 * P + 2, BIG, None),
     b"aligned"),
    ("sfx_tap_dist", lambda lib: lib.sfx_tap_dist(1, 4, 64, P, 2 * P, 3 * P, 0, 4 * P, 5 * P, 15, None),
     b"workspace too small"),
    ("sfx_tap_dist_bwd", lambda lib: lib.sfx_tap_dist_bwd(1, 4, 0, P, 2 * P, 3 * P, 4 * P, 1, 5 * P, None),
     b"bad sizes"),
    ("sfx_tap_dist_bwd", lambda lib: lib.sfx_tap_dist_bwd(2, 1 << 23, 64, P, 2 * P, 3 * P, 4 * P, 1, 5 * P, None),
     b"2 GiB"),
    ("sfx_tap_dist_bwd", lambda lib: lib.sfx_tap_dist_bwd(1, 4, 64, P, 2 * P, 3 * P, None, 1, 5 * P, None),
     b"null buffer"),
    ("sfx_tap_dist_bwd", lambda lib: lib.sfx_tap_dist_bwd(1, 4, 64, P, 2 * P, 3 * P, 4 * P, 1, P, None), b"aliases"),
]


@pytest.mark.parametrize("i", range(len(CASES)))
def test_bad_arguments_are_refused_before_any_launch(i):
    """No GPU is present where this runs: a call that reached a launch (or a memset) could not return a clean
    SFX_ERR_INVALID with the entry's own message."""
    name, fn, word = CASES[i]
    lib = _lib()
    rc = fn(lib)
    msg = lib.sfx_last_error()
    assert rc < 0
    assert name.encode() + b":" in msg and word in msg, msg


def test_entries_declared_sizes_and_abi_unchanged():
    from splatformer_amd import _lib as B
    lib = _lib()
    for name in ("sfx_conv3x3_tile", "sfx_conv3x3_pack_bytes", "sfx_conv3x3_pack", "sfx_conv3x3_workspace_bytes",
                 "sfx_conv3x3", "sfx_maxpool2x2", "sfx_maxpool2x2_bwd", "sfx_lpips_input", "sfx_lpips_input_bwd",
                 "sfx_tap_normalize", "sfx_tap_dist_workspace_bytes", "sfx_tap_dist", "sfx_tap_dist_bwd"):
        assert hasattr(lib, name) and name in B.SIGNATURES
    assert lib.sfx_abi_version() == 17
    assert lib.sfx_conv3x3_pack_bytes(64, 128) == 64 * 128 * 36 + 128 * 4   # fp16 h + l per weight, row scales
    assert lib.sfx_conv3x3_pack_bytes(3, 64) == 3 * 64 * 36                  # fp32, VALU route
    assert lib.sfx_conv3x3_pack_bytes(0, 64) == 0
    assert lib.sfx_conv3x3_workspace_bytes(5) == 32 and lib.sfx_conv3x3_workspace_bytes(0) == 0
    assert lib.sfx_tap_dist_workspace_bytes(2, 10) == 80
    th, tw = L.conv_tile()
    assert th >= 1 and tw >= 1


def test_trainer_needs_an_lpips_object():
    from splatformer_amd.feature_predictor import FeaturePredictor
    from splatformer_amd.train import Trainer
    prm = inspect.signature(Trainer.__init__).parameters
    assert prm["lpips_loss_weight"].default == 0.0 and prm["lpips"].default is None
    model = FeaturePredictor(sh_degree=1, zeroinit=False)
    with pytest.raises(ValueError, match="lpips"):
        Trainer(model, lpips_loss_weight=1.0)
    with pytest.raises(ValueError, match="lpips_loss_weight"):
        Trainer(model, lpips_loss_weight=-1.0)


def test_python_wrappers_refuse_cpu():
    convs, lins = R.make_weights(0)
    with pytest.raises(RuntimeError):
        L.LPIPS(convs, lins, device="cpu")


# ---- the restatement itself ---------------------------------------------------------------------------------------------
def test_ref_of_equal_images_is_zero(weights):
    convs, lins = weights
    x = torch.rand(2, 16, 19, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.lpips(x, x, convs, lins), torch.zeros(2, dtype=torch.float64))


def test_frozen_variant_with_its_own_decisions_equals_the_plain_one(weights):
    convs, lins = weights
    g = torch.Generator().manual_seed(2)
    x, y = torch.rand(2, 17, 21, 3, generator=g), torch.rand(2, 17, 21, 3, generator=g)
    acts, pres = R.features(R.input_stage(x), convs)
    masks, idx = R.decisions(acts)
    assert all(torch.equal(m, z > 0) for m, z in zip(masks, pres))
    plain = R.lpips(x, y, convs, lins)
    frozen = R.lpips_frozen(x, y, convs, lins, masks, idx)
    assert plain.shape == (2,) and float(plain.min()) > 0
    assert float((plain - frozen).abs().max()) <= 1e-14 * float(plain.abs().max())


def test_first_max_index_and_quantiser():
    a = torch.tensor([[[[1., 3., 0., 0., 9.], [3., 2., 0., 0., 9.], [5., 5., 5., 5., 9.]]]])  # [1,1,3,5]
    idx = R.first_max_index(a)
    assert idx.tolist() == [[[[1, 2]]]]  # first 3 in row-major order; the all-zero window -> its first element
    assert torch.equal(R.pool_gather(a, idx), torch.nn.functional.max_pool2d(a, 2))
    x = torch.tensor([0.0, 0.5, 0.999, 1.0, 1.2, -0.1]).view(1, 1, 2, 3)
    q = R.quantize_u8(x)
    want = torch.tensor([0.0, 127.0, 254.0, 255.0, 255.0, 0.0]) / torch.tensor(255.0)  # truncation, saturation
    assert torch.equal(q.flatten(), want)
