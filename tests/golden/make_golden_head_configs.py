"""Capture tests/golden/head_configs.npz from the reference's own FeaturePredictor (run where the reference
tree is present; the fixture holds data only).

For every wiring of tests/heads_ref.py:CASES the reference model is built with a small head (width 16, 3 layers,
zeroinit off), run on a 64-Gaussian scene with make_golden.install_stubs' recording stub backbone, and recorded:
the input dict, the backbone's input `feat` and `grid_coord`, the stub backbone's output, the head state dict, every
output array, the ordered output keys and which outputs were the input's own tensor objects.

The reference keeps the attribute widths in a module-level table it rewrites per construction, so each model is
built and run before the next is constructed.
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import heads_ref  # noqa: E402
import make_golden  # noqa: E402

WIDTH, NLAYER, N = 16, 3, 64


def main():
    rec = {}
    make_golden.install_stubs(rec)
    sys.path.insert(0, make_golden.REF)
    import models  # noqa: F401  (namespace package of the reference)
    fp_mod = importlib.import_module("models.feature_predictor")
    from splatformer_amd.scenes import make_scene
    acts = {"identity": torch.nn.Identity, "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid}
    out = {"cases": np.array(sorted(heads_ref.CASES))}
    for i, (name, case) in enumerate(sorted(heads_ref.CASES.items())):
        deg = case["sh_degree"]
        feats_in = heads_ref.drop_rest(case["input_features"], deg)
        feats_out = heads_ref.drop_rest(case["output_features"], deg)
        torch.manual_seed(100 + i)
        model = fp_mod.FeaturePredictor(
            backbone_type="PT", sh_degree=deg, input_features=feats_in,
            input_feat_to_mlp=case["input_feat_to_mlp"], output_features=feats_out, output_head_nlayer=NLAYER,
            output_head_type="mlp-relu", output_head_width=WIDTH, output_features_type=case["output_features_type"],
            res_feature_activation={f: acts[a]() for f, a in case["activations"].items()},
            max_scale_normalized=case["max_scale_normalized"], grid_resolution=384, resume_ckpt=None,
            input_embed_to_mlp=False, zeroinit=False, additional_info={"tome": "base", "r": 0.0})
        model.eval()
        s = make_scene(N, sh_degree=deg, seed=40 + i)
        if deg == 0:
            s.pop("features_rest", None)
        rec.clear()
        with torch.no_grad():
            outs = model([s], [0])
        p = name + "."
        for k, v in s.items():
            out[p + "in." + k] = v.numpy()
        out[p + "bb_feat"] = rec["backbone_in"]["feat"].numpy()
        out[p + "bb_grid_coord"] = rec["backbone_in"]["grid_coord"].numpy()
        out[p + "bb_out"] = rec["backbone_out"].numpy()
        for k, v in model.features_outputhead.state_dict().items():
            out[p + "head." + k] = v.numpy()
        for k, v in outs[0].items():
            out[p + "out." + k] = v.numpy()
        out[p + "out_keys"] = np.array(list(outs[0]))
        out[p + "same_object"] = np.array([k for k, v in outs[0].items() if v is s.get(k)])
    path = os.path.join(HERE, "head_configs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
