"""Generates tests/golden/resnet50_keys.json and tests/golden/resnet50_vectors.npz by IMPORTING THE REFERENCE (only possible in the
build container, where /root/reference exists), on the CPU.  What is committed is data: key lists, sums and the reference's outputs.

    python tests/golden/make_resnet50_golden.py

Contents (recipes in tests/resnet50_scenario.py, so that the tests rebuild weights and inputs without the reference):
  keys      : keys, shapes and dtypes of the reference's resnet50(in_channels=18) and of its PoseMFShapeGaussianNet at
              MODEL.NUM_RESNET_LAYERS = 50
  init_*    : per-tensor float64 sum and sum of squares of both state dicts under torch.manual_seed(0), in key order
  small_*   : the reference's ResNet(Bottleneck, [2, 2, 1, 1], 18) with the scenario's seeded weights on the scenario's (3, 18, 64, 64)
              and (2, 18, 40, 24) inputs: features in float32 and from .double()
  full_*    : the reference's resnet50(18), run the same way on (2, 18, 64, 64)
  net_*     : the whole reference net at 50 (scenario.net_state_dict) on that input, float32
Recipe checks asserted here: max|y64| finite, fewer than half of the features exactly zero, e_cpu32 <= 64 * 2^-23 max|y64|.
"""
import copy
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.modules.setdefault("cv2", types.ModuleType("cv2"))     # utils/rigid_transform_utils.py:1 imports cv2; unused on the path
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from models.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet as RefNet  # noqa: E402
from models.resnet import Bottleneck as RefBottleneck, ResNet as RefResNet, resnet50 as ref_resnet50  # noqa: E402

from hierarchicalprobabilistic3dhuman_amd import configs  # noqa: E402
import resnet50_scenario as S  # noqa: E402


def sums(sd):
    return (np.array([float(v.double().sum()) for v in sd.values()]), np.array([float((v.double() ** 2).sum()) for v in sd.values()]))


def run(model, sd, x, tag, out):
    """Features of the reference ``model`` with weights ``sd``: float32, and from .double(); the recipe checks."""
    model.load_state_dict(sd, strict=True)
    model.eval()
    with torch.no_grad():
        y32 = model(x)
        y64 = copy.deepcopy(model).double()(x.double())
    scale = float(y64.abs().max())
    e = float((y32.double() - y64).abs().max())
    zeros = float((y64 == 0).double().mean())
    print("%-14s max|y64| = %.4e  e_cpu32 = %.3e = %.2f * 2^-23 max|y64|  exact zeros %.3f" % (tag, scale, e, e / (S.EPS32 * scale), zeros))
    assert np.isfinite(scale) and zeros < 0.5 and e <= 64 * S.EPS32 * scale, tag
    out[tag + "_feats32"], out[tag + "_feats64"] = y32.numpy(), y64.numpy()
    return y32


def main():
    parents = configs.SMPL_PARENTS
    cfg = S.net_config()
    torch.manual_seed(0)
    enc = ref_resnet50(in_channels=18)
    torch.manual_seed(0)
    net = RefNet(parents, cfg)
    keys = {"encoder": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in enc.state_dict().items()],
            "net": [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in net.state_dict().items()]}
    with open(os.path.join(HERE, "resnet50_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    assert {k: (tuple(s), d) for k, s, d in keys["encoder"]} == S.encoder_shapes(S.FULL_LAYERS), "the scenario's shape table"
    out = {}
    out["init_encoder_sum"], out["init_encoder_sumsq"] = sums(enc.state_dict())
    out["init_net_sum"], out["init_net_sumsq"] = sums(net.state_dict())

    small = RefResNet(RefBottleneck, list(S.SMALL_LAYERS), 18)
    assert S.shapes_of(small.state_dict()) == S.encoder_shapes(S.SMALL_LAYERS)
    for name in ("small_wino", "small_generic"):
        sd, x = S.case(name)
        run(small, sd, x, name, out)
    sd, x = S.case("full")
    run(enc, sd, x, "full", out)

    nsd = S.net_state_dict(RefNet, parents)
    net.load_state_dict(nsd, strict=True)
    net.eval()
    with torch.no_grad():
        pose_F, pose_U, pose_S, pose_V, mode, shape_dist, glob, cam = net(x)
    for k, v in dict(F=pose_F, S=pose_S, mode=mode, shape_loc=shape_dist.loc, shape_scale=shape_dist.scale, glob=glob, cam=cam).items():
        out["net_" + k] = v.numpy()
        print("net_%-12s %s max| | = %.4e" % (k, tuple(v.shape), float(v.abs().max())))
    path = os.path.join(HERE, "resnet50_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
