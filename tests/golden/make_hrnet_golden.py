"""Generates tests/golden/hrnet_vectors.npz and tests/golden/hrnet_w48_keys.json by IMPORTING THE REFERENCE (only possible where
/root/reference exists): the reference's own models/pose2D_hrnet.PoseHighResolutionNet on the CPU.

    hrnet_w48_keys.json   [key, shape, dtype] of the state dict of the default (W48) network, in the reference's order
    hrnet_vectors.npz     the reference's float64 heat maps of tests/hrnet_scenario.py's SMALL config on a (2, 3, 64, 96) input and of
                          its NARROW config on (1, 3, 32, 64), weights = hrnet_scenario.seeded_state_dict (loaded strict) of the
                          reference module's own shapes, seed 0; inputs = hrnet_scenario.seeded_input

What is committed is data; weights and inputs are regenerated from the seeds.

    python tests/golden/make_hrnet_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import hrnet_scenario as S  # noqa: E402


def reference_class():
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_pose2D_hrnet", os.path.join(REF, "models", "pose2D_hrnet.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.PoseHighResolutionNet


def main():
    Net = reference_class()
    w48 = Net(S.config("W48"))
    keys = [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in w48.state_dict().items()]
    with open(os.path.join(HERE, "hrnet_w48_keys.json"), "w") as f:
        json.dump(keys, f)
    print("W48: %d entries, %d parameters" % (len(keys), sum(p.numel() for p in w48.parameters())))
    out = {}
    for name, shape in S.GOLDEN_INPUTS.items():
        net = Net(S.config(name)).eval()
        sd = S.seeded_state_dict(S.shapes_of(net.state_dict()), 0)
        net.load_state_dict(sd, strict=True)
        net = net.double()
        with torch.no_grad():
            y = net(S.seeded_input(shape, 0).double())
        out[name] = y.numpy()
        print(name, tuple(y.shape), "max|y| = %.4f" % float(y.abs().max()))
    np.savez_compressed(os.path.join(HERE, "hrnet_vectors.npz"), **out)


if __name__ == "__main__":
    main()
