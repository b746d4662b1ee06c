"""Plain-torch statement of what FeaturePredictor does around its backbone, for every head configuration:
batchify (the backbone's input features and voxel coordinates), the output heads on the backbone feature, the
activation / residual ('res') or direct prediction with the scale clamp ('dc'), and the output dict with the
untouched attributes handed through.  Runs in the dtype of the tensors it is given (fp32 for fixture parity,
fp64 as the yardstick of the device kernels).  No device code, no project import."""
from __future__ import annotations

from collections import OrderedDict

import torch

ALL_FEATURES = ["means", "features_dc", "features_rest", "opacities", "scales", "quats"]
BASE = ["means", "scales", "opacities", "quats", "features_dc", "features_rest"]
_BASE_ACT = {f: "tanh" if f == "means" else "identity" for f in BASE}

# The head wirings the tests and the fixture (tests/golden/head_configs.npz) share: constructor arguments, with
# activations by name.
CASES = {
    "a": dict(sh_degree=1, input_features=BASE, output_features=BASE, output_features_type="res",
              input_feat_to_mlp=True, max_scale_normalized=1e-2,
              activations=dict(_BASE_ACT, scales="sigmoid", opacities="sigmoid")),
    "b": dict(sh_degree=1, input_features=BASE, output_features=["opacities"], output_features_type="res",
              input_feat_to_mlp=True, max_scale_normalized=1e-2, activations=dict(_BASE_ACT)),
    "c": dict(sh_degree=1, input_features=["features_dc", "means", "opacities"], output_features=["scales", "means"],
              output_features_type="res", input_feat_to_mlp=True, max_scale_normalized=1e-2,
              activations=dict(_BASE_ACT, scales="sigmoid", means="tanh")),
    "d": dict(sh_degree=3, input_features=BASE, output_features=BASE, output_features_type="dc",
              input_feat_to_mlp=True, max_scale_normalized=1e-2, activations=dict(_BASE_ACT)),
    "e": dict(sh_degree=1, input_features=BASE, output_features=["scales", "quats"], output_features_type="dc",
              input_feat_to_mlp=True, max_scale_normalized=-1.0, activations=dict(_BASE_ACT)),
    "f": dict(sh_degree=1, input_features=BASE, output_features=BASE, output_features_type="res",
              input_feat_to_mlp=False, max_scale_normalized=1e-2, activations=dict(_BASE_ACT)),
    "g": dict(sh_degree=0, input_features=BASE[:5], output_features=["opacities", "features_dc"],
              output_features_type="dc", input_feat_to_mlp=True, max_scale_normalized=1e-2,
              activations=dict(_BASE_ACT)),
}


def product_kwargs(case, **more):
    """CASES[...] as splatformer_amd.FeaturePredictor keyword arguments."""
    kw = {k: v for k, v in case.items() if k != "activations"}
    kw["res_feature_activation"] = {f: a for f, a in case["activations"].items()}
    kw.update(more)
    return kw
ACTIVATIONS = {"identity": lambda t: t, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


def drop_rest(features, sh_degree):
    """The project's SH degree 0 rule: features_rest is in neither list."""
    return [f for f in features if not (f == "features_rest" and sh_degree == 0)]


def batchify(gs, input_features, grid_resolution=384):
    """(feat [N, Cin] = the input attributes side by side in list order, features_rest flattened;
    grid_coord = floor(means * grid_resolution) as int32, from `means` whether or not it is an input)."""
    n = gs["means"].shape[0]
    feat = torch.cat([gs[f].reshape(n, -1) for f in input_features], 1)
    grid = torch.floor(gs["means"] * grid_resolution).int()
    return feat, grid


def mlp(sd, name, y):
    """features_outputhead[name]: Linear, ReLU, ..., Linear (state-dict keys '<name>.<2 i>.weight' / '.bias')."""
    idx = sorted({int(k.split(".")[1]) for k in sd if k.split(".")[0] == name})
    for i in idx:
        y = y @ sd[f"{name}.{i}.weight"].T + sd[f"{name}.{i}.bias"]
        if i != idx[-1]:
            y = torch.relu(y)
    return y


def log_max_scale(max_scale_normalized):
    """log(max_scale_normalized) the way an fp32 tensor takes it."""
    return float(torch.log(torch.tensor(max_scale_normalized, dtype=torch.float32)))


def predicted(sd, backbone_feat, gs, *, input_features, output_features, output_features_type="res",
              input_feat_to_mlp=True, activations=None, max_scale_normalized=1e-2):
    """name -> the part of each output the heads produce, flat [N, c]: act(head(y)) in 'res' mode, head(y) in 'dc'
    mode, -relu(head(y)) for clamped scales (without the constant)."""
    feat, _ = batchify(gs, input_features)
    y = torch.cat([backbone_feat, feat.to(backbone_feat.dtype)], 1) if input_feat_to_mlp else backbone_feat
    out = OrderedDict()
    for f in output_features:
        z = mlp(sd, f, y)
        if output_features_type == "res":
            z = ACTIVATIONS[(activations or {}).get(f, "tanh" if f == "means" else "identity")](z)
        elif f == "scales" and max_scale_normalized > 0:
            z = -torch.relu(z)
        out[f] = z
    return out


def forward(sd, backbone_feat, gs, *, sh_degree, input_features, output_features, output_features_type="res",
            input_feat_to_mlp=True, activations=None, max_scale_normalized=1e-2):
    """The refined dict: output_features first, in their order, then every other attribute as the input's own
    tensor.  `sd`: the features_outputhead state dict; `activations`: name -> 'identity' | 'tanh' | 'sigmoid'."""
    input_features = drop_rest(input_features, sh_degree)
    output_features = drop_rest(output_features, sh_degree)
    pred = predicted(sd, backbone_feat, gs, input_features=input_features, output_features=output_features,
                     output_features_type=output_features_type, input_feat_to_mlp=input_feat_to_mlp,
                     activations=activations, max_scale_normalized=max_scale_normalized)
    out = OrderedDict()
    for f, z in pred.items():
        if f == "features_rest":
            z = z.reshape(z.shape[0], -1, 3)
        if output_features_type == "res":
            z = gs[f] + z
        elif f == "scales" and max_scale_normalized > 0:
            z = z + log_max_scale(max_scale_normalized)
        out[f] = z
    for f in ALL_FEATURES:
        if f == "features_rest" and sh_degree == 0:
            continue
        if f not in out:
            out[f] = gs[f]
    return out
