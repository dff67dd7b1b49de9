#!/usr/bin/env python3
"""Generate tests/golden/g14_camera_branch.npz by RUNNING THE REFERENCE'S OWN classes of the vovnet model's TXT branch
(src/model_vovnet_transformer.py: AdaptiveFeaturePyramid, LightweightCameraTransformer, BEVCameraFusion,
UnifiedPredictor; src/modules.py: SceneUnder) on the CPU, after the lines :612-637 of VoVNetBEVTransformer.forward.
Build container only (needs the reference tree).  The fixture holds seeds, shapes and the reference's outputs; weights
and inputs are NOT stored: this script and the tests regenerate them from `oracle.vovnet_oracle.seeded_state` and numpy's
RandomState, with the shape lists read off each side's own modules.

    python tools/gen_golden_camera_branch.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

from _ref_loader import load_reference  # noqa: E402
from oracle import vovnet_oracle as vo  # noqa: E402  (parameter generator only)

OUT = os.path.join(ROOT, "tests", "golden")
N_CAMS = 6
BEV_SHAPE = (1, 256, 4, 4)
# (name, c3 channels, fH, fW, seed): one sample of six cameras each
CASES = (("a", 768, 8, 22, 140), ("b", 64, 3, 5, 150))
MODULES = ("feature_pyramid", "sceneunder", "camera_transformer", "bev_fusion", "unified_predictor")


def randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape).astype(np.float32))


def load_seeded(module, seed):
    shapes = [(k, tuple(v.shape)) for k, v in module.state_dict().items()]
    module.load_state_dict(vo.seeded_state(shapes, seed), strict=True)
    return module.eval()


def main():
    _, rmodules, _ = load_reference()
    import src.model_vovnet_transformer as rv

    torch.set_grad_enabled(False)
    arrs = {"n_cams": N_CAMS, "bev_shape": np.asarray(BEV_SHAPE)}
    for name, cin, fH, fW, seed in CASES:
        mods = [rv.AdaptiveFeaturePyramid(cin, 256), rmodules.SceneUnder(in_channels=256),
                rv.LightweightCameraTransformer(256, 4, 0.1, N_CAMS), rv.BEVCameraFusion(256, 256, 4),
                rv.UnifiedPredictor(256, 4, 8, N_CAMS)]
        fp, su, ct, bf, up = (load_seeded(m, seed + i) for i, m in enumerate(mods))
        c3 = randn(seed + 10, N_CAMS, cin, fH, fW)
        bev_refined = randn(seed + 11, *BEV_SHAPE)
        B, N = 1, N_CAMS
        # the lines :612-637
        scene = su(fp(c3))
        tokens = torch.nn.functional.adaptive_avg_pool2d(scene, (1, 1)).squeeze(-1).squeeze(-1)
        ids = torch.arange(N).unsqueeze(0).expand(B, -1)
        fused = bf(ct(tokens.view(B, N, -1), ids), bev_refined)
        action, description = up(fused)
        arrs.update({name + "_seed": seed, name + "_c3_shape": np.asarray(c3.shape), name + "_tokens": tokens.numpy(),
                     name + "_action": action.numpy(), name + "_description": description.numpy()})
    path = os.path.join(OUT, "g14_camera_branch.npz")
    np.savez_compressed(path, **arrs)
    print("wrote %s %.1f KB" % (path, os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
