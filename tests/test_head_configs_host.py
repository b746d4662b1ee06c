"""Every FeaturePredictor head wiring the reference accepts, on the host: the plain-torch restatement
(tests/heads_ref.py) against a fixture captured from the reference's own module (tests/golden/head_configs.npz,
written by tests/golden/make_golden_head_configs.py), and the product module's structure, argument checks and
epilogue table.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heads_ref  # noqa: E402
from splatformer_amd import ptv3_ops as ops  # noqa: E402
from splatformer_amd.feature_predictor import BASE_FEATURES, FeaturePredictor, load_checkpoint  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_configs.npz")
CASES = sorted(heads_ref.CASES)
WIDTH, NLAYER = 16, 3  # the fixture's small heads


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD)
    assert sorted(z["cases"].tolist()) == CASES
    return z


def _sub(z, prefix):
    return {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}


def _product(case, **more):
    return FeaturePredictor(**heads_ref.product_kwargs(case, output_head_width=WIDTH, output_head_nlayer=NLAYER,
                                                       **more))


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(gold, name):
    case = heads_ref.CASES[name]
    gs = {k: torch.from_numpy(v) for k, v in _sub(gold, f"{name}.in.").items()}
    sd = {k: torch.from_numpy(v) for k, v in _sub(gold, f"{name}.head.").items()}
    feats_in = heads_ref.drop_rest(case["input_features"], case["sh_degree"])
    feat, grid = heads_ref.batchify(gs, feats_in)
    np.testing.assert_array_equal(feat.numpy(), gold[f"{name}.bb_feat"])
    np.testing.assert_array_equal(grid.numpy(), gold[f"{name}.bb_grid_coord"])
    assert grid.dtype == torch.int32 and gold[f"{name}.bb_grid_coord"].dtype == np.int32
    out = heads_ref.forward(sd, torch.from_numpy(gold[f"{name}.bb_out"]), gs, **case)
    assert list(out) == gold[f"{name}.out_keys"].tolist()
    for k, v in out.items():
        ref = gold[f"{name}.out.{k}"]
        assert tuple(v.shape) == ref.shape, k
        np.testing.assert_allclose(v.numpy(), ref, rtol=1e-6, atol=1e-6, err_msg=k)
    same = gold[f"{name}.same_object"].tolist()
    outs = heads_ref.drop_rest(case["output_features"], case["sh_degree"])
    assert same == [k for k in out if k not in outs]
    for k in same:
        assert out[k] is gs[k]


@pytest.mark.parametrize("name", CASES)
def test_product_module_structure(gold, name):
    case = heads_ref.CASES[name]
    fp = _product(case)
    want = {k: v.shape for k, v in _sub(gold, f"{name}.head.").items()}
    got = {k: tuple(v.shape) for k, v in fp.features_outputhead.state_dict().items()}
    assert list(got) == list(want) and got == want
    outs = heads_ref.drop_rest(case["output_features"], case["sh_degree"])
    cols = fp.columns()
    assert list(cols) == outs
    c = 0
    for f in outs:
        w = int(np.prod(gold[f"{name}.out.{f}"].shape[1:]))
        assert cols[f] == (c, w)
        c += w
    assert fp.gs_features_dim == gold[f"{name}.bb_feat"].shape[1]
    assert fp.head_in == 96 + (fp.gs_features_dim if case["input_feat_to_mlp"] else 0)
    # unpack: views of the packed record in output order, features_rest as [N, -1, 3]
    rec = torch.arange(5 * c, dtype=torch.float32).reshape(5, c)
    un = fp.unpack(rec)
    assert list(un) == outs
    for f in outs:
        assert tuple(un[f].shape[1:]) == gold[f"{name}.out.{f}"].shape[1:]
        assert torch.equal(un[f].reshape(5, -1), rec[:, cols[f][0]:cols[f][0] + cols[f][1]])


def test_reference_shaped_checkpoint_loads_strict(gold):
    """A state dict with the reference's head keys and shapes (case c: two heads, 103 inputs) loads with
    strict=True and lands in the heads."""
    fp = _product(heads_ref.CASES["c"])
    sd = {k: v.clone() for k, v in fp.state_dict().items() if not k.startswith("features_outputhead.")}
    heads = {"features_outputhead." + k: torch.from_numpy(v) for k, v in _sub(gold, "c.head.").items()}
    assert sorted(k for k in fp.state_dict() if k.startswith("features_outputhead.")) == sorted(heads)
    sd.update(heads)
    r = load_checkpoint(fp, {"module." + k: v for k, v in sd.items()}, strict=True)
    assert not r.missing_keys and not r.unexpected_keys
    assert torch.equal(fp.features_outputhead["scales"][0].weight, heads["features_outputhead.scales.0.weight"])


@pytest.mark.parametrize("kw,arg", [
    (dict(input_features=["means", "colour"]), "input_features"),
    (dict(output_features=["means", "normals"]), "output_features"),
    (dict(input_features=["means", "scales", "means"]), "input_features"),
    (dict(output_features=["scales", "scales"]), "output_features"),
    (dict(output_features=[]), "output_features"),
    (dict(sh_degree=0, output_features=["features_rest"]), "output_features"),
    (dict(res_feature_activation={"means": torch.nn.ReLU()}), "res_feature_activation"),
    (dict(res_feature_activation={"scales": torch.nn.GELU}), "res_feature_activation"),
    (dict(res_feature_activation={"quats": "softplus"}), "res_feature_activation"),
])
def test_invalid_arguments_raise_value_error(kw, arg):
    with pytest.raises(ValueError, match=arg):
        FeaturePredictor(**kw)


def test_out_of_scope_arguments_still_raise():
    with pytest.raises(NotImplementedError):
        FeaturePredictor(backbone_type="SP")
    with pytest.raises(NotImplementedError):
        FeaturePredictor(output_head_type="mlp-gelu")


@pytest.mark.parametrize("form", ["instance", "class", "name"])
def test_activation_forms(form):
    mods = {"tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid, "identity": torch.nn.Identity}
    make = {"instance": lambda a: mods[a](), "class": lambda a: mods[a], "name": lambda a: mods[a].__name__}[form]
    fp = FeaturePredictor(output_head_width=WIDTH, output_head_nlayer=NLAYER, res_feature_activation={
        "means": make("sigmoid"), "scales": make("tanh"), "opacities": make("identity")})
    assert fp.res_activation == {"means": "sigmoid", "scales": "tanh", "opacities": "identity", "quats": "identity",
                                 "features_dc": "identity", "features_rest": "identity"}
    assert not fp.base_wiring


@pytest.mark.parametrize("sh", [0, 1, 3])
def test_base_arguments_give_todays_table(sh):
    """ptv3_base.gin's arguments: tanh on the three means columns, every residual base in the feat slice behind the
    96 backbone columns, no constant -- sfx_heads' (res_off = 96, n_tanh = 3) -- and the base entry points."""
    fp = FeaturePredictor(sh_degree=sh, output_head_width=WIDTH, output_head_nlayer=NLAYER)
    n = fp.gs_features_dim
    assert fp.base_wiring and fp.output_features == [f for f in BASE_FEATURES if sh or f != "features_rest"]
    assert fp.epilogue_table() == ops.heads_base_table(96, 3, n)
    assert fp.epilogue_table() == ([1, 1, 1] + [0] * (n - 3), list(range(96, 96 + n)), [0.0] * n)
    ld, fcol, rcol = fp.row_layout()
    assert ld == (96 + n + 3) // 4 * 4 and not rcol and fcol["means"] == 96


def test_tables_of_the_other_wirings():
    # c: scales (sigmoid) is no head input: its base sits behind the padded feat; means (tanh) inside feat
    fp = _product(heads_ref.CASES["c"])
    ld, fcol, rcol = fp.row_layout()
    assert fcol == {"features_dc": 96, "means": 99, "opacities": 102} and rcol == {"scales": 104} and ld == 108
    assert fp.head_in == 103
    assert fp.epilogue_table() == ([2, 2, 2, 1, 1, 1], [104, 105, 106, 99, 100, 101], [0.0] * 6)
    # d: direct prediction, clamp on the scales columns with the fp32 log
    fp = _product(heads_ref.CASES["d"])
    act, res, add = fp.epilogue_table()
    k = float(torch.log(torch.tensor(1e-2)))
    assert act == [0] * 3 + [3] * 3 + [0] * 53 and res == [-1] * 59
    assert add == [0.0] * 3 + [k] * 3 + [0.0] * 53
    # e: clamp off; f: base table on the backbone feature alone
    assert _product(heads_ref.CASES["e"]).epilogue_table() == ([0] * 7, [-1] * 7, [0.0] * 7)
    fp = _product(heads_ref.CASES["f"])
    assert fp.head_in == 96 and not fp.base_wiring and fp.epilogue_table() == ops.heads_base_table(96, 3, 23)


def test_new_entry_points_validate_on_the_host():
    """Argument checks of the new C entries run without a GPU and launch nothing."""
    import ctypes
    from splatformer_amd import _lib
    lib = _lib.load()
    assert lib.sfx_abi_version() == 17
    I4, F4 = ctypes.c_int * 4, ctypes.c_float * 4
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    oc = (ctypes.c_int * 2)(0, 4)
    ok = dict(act=I4(0, 1, 2, 3), res=I4(-1, 0, 7, 7), add=F4())
    rc = lib.sfx_heads_cols(5, 1, 8, 4, p, 8, oc, I4(0, 1, 2, 4), ok["res"], ok["add"], p, p, p, None)
    assert rc == -1 and b"epilogue table" in lib.sfx_last_error()
    rc = lib.sfx_heads_cols(5, 1, 8, 4, p, 8, oc, ok["act"], I4(-1, 0, 7, 8), ok["add"], p, p, p, None)
    assert rc == -1 and b"epilogue table" in lib.sfx_last_error()
    rc = lib.sfx_heads_cols(5, 7, 8, 4, p, 8, oc, ok["act"], ok["res"], ok["add"], p, p, p, None)
    assert rc == -1 and b"unsupported head shape" in lib.sfx_last_error()
    srcs, lds = (ctypes.c_void_p * 2)(p, p), (ctypes.c_longlong * 2)(3, 3)
    w2 = (ctypes.c_int * 2)(3, 3)
    rc = lib.sfx_gs_pack_cols(4, 2, srcs, lds, w2, (ctypes.c_int * 2)(0, 2), p, 3, 384.0, p, 8, None, None, None)
    assert rc == -1 and b"overlap" in lib.sfx_last_error()
    rc = lib.sfx_gs_pack_cols(4, 2, srcs, lds, w2, (ctypes.c_int * 2)(0, 6), p, 3, 384.0, p, 8, None, None, None)
    assert rc == -1 and b"outside the row" in lib.sfx_last_error()
    rc = lib.sfx_gs_pack_cols(4, 9, srcs, lds, w2, w2, p, 3, 384.0, p, 8, None, None, None)
    assert rc == -1 and b"1..8 sources" in lib.sfx_last_error()
    rc = lib.sfx_col_epilogue_fwd(4, 3, p, 2, p, p, p, p, 3, p + 64, 3, None)
    assert rc == -1 and b"leading dim" in lib.sfx_last_error()
    rc = lib.sfx_col_epilogue_bwd(4, 3, p, 3, p, 3, p, p, 2, None)
    assert rc == -1 and b"leading dim" in lib.sfx_last_error()
