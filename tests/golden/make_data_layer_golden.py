"""Generates tests/golden/data_layer_vectors.npz by IMPORTING THE REFERENCE (only possible where a checkout of it exists; its
directory comes from HPS_REFERENCE_DIR, default /root/reference): the reference's own data/on_the_fly_smpl_train_dataset.py class, run
on the CPU, tells which texture and which background it picks after torch.manual_seed(seed).  What is committed is data: the indices.

    python tests/golden/make_data_layer_golden.py

draws_seed<S>_B<B>: (B, 3) int64 = (is_grey, texture index, background index) of items 0 .. B-1 taken in order after
torch.manual_seed(S), on the files tests/data_layer_scenario.write_train_files writes with marker textures; grey_tex_prob and the bank
sizes are recorded beside them.

The reference imports cv2, which is absent here.  For the draws a stand-in module of our own is enough: its imread returns the
background's index as a pixel value and its resize keeps that value, so that the picked index can be read back from the item.

Where the real OpenCV IS installed, the script also records its outputs on the scenario's resize and crop cases (cv2_resize_* /
cv2_crop_* / cv2_seg_*); tests/test_data_layer_host.py compares the NumPy restatements against them and skips while they are absent.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("HPS_REFERENCE_DIR", "/root/reference")

try:
    import cv2 as real_cv2
except ImportError:
    real_cv2 = None

stand_in = types.ModuleType("cv2")
stand_in.COLOR_BGR2RGB, stand_in.INTER_LINEAR = 4, 1
stand_in.imread = lambda path, *flags: np.full((2, 2, 3), int(os.path.basename(path)[3:-4]), np.uint8)
stand_in.cvtColor = lambda image, code: image[..., ::-1]
stand_in.resize = lambda image, dsize, interpolation=None: np.full((dsize[1], dsize[0], 3), image[0, 0, 0], np.uint8)
sys.modules["cv2"] = stand_in
sys.path.insert(0, REF)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from data.on_the_fly_smpl_train_dataset import OnTheFlySMPLTrainDataset  # noqa: E402

import data_layer_scenario as S  # noqa: E402


def draws(out):
    with tempfile.TemporaryDirectory() as root:
        files = S.write_train_files(root, marker_textures=True)
        ds = OnTheFlySMPLTrainDataset(grey_tex_prob=S.DRAW_GREY_PROB, img_wh=4, **files)
        for seed in S.DRAW_SEEDS:
            for B in S.DRAW_BATCHES:
                torch.manual_seed(seed)
                rows = []
                for i in range(B):
                    item = ds[i % len(ds)]
                    tex = int(round(float(item["texture"][0, 0, 0]) * 255))
                    rows.append((int(tex < 100), tex % 100, int(round(float(item["background"][0, 0, 0]) * 255))))
                out["draws_seed%d_B%d" % (seed, B)] = np.array(rows, dtype=np.int64)
    out["grey_tex_prob"] = np.float64(S.DRAW_GREY_PROB)
    out["bank_sizes"] = np.array([S.DRAW_N_GREY, S.DRAW_N_NONGREY, S.DRAW_N_BACKGROUNDS], dtype=np.int64)


def opencv(out):
    cv2 = real_cv2
    for H, W in S.RESIZE_SOURCES:
        for T in S.RESIZE_TARGETS:
            out["cv2_resize_%dx%d_to%d" % (H, W, T)] = cv2.resize(S.noise_image(H * 1000 + W, H, W), (T, T), interpolation=cv2.INTER_LINEAR)
    for H, W in S.CROP_IMAGES:
        rgb, seg = S.noise_image(H * 1000 + W, H, W), S.noise_image(H * 1000 + W + 1, H, W, channels=0)
        for name, (centre, side) in S.crop_boxes(H, W).items():
            M = S.crop_matrix(centre, side, 1.2, 16)
            kw = dict(borderMode=cv2.BORDER_CONSTANT, borderValue=0)
            out["cv2_crop_%dx%d_%s" % (H, W, name)] = cv2.warpAffine(rgb, M, (16, 16), flags=cv2.INTER_LINEAR, **kw)
            out["cv2_seg_%dx%d_%s" % (H, W, name)] = cv2.warpAffine(seg, M, (16, 16), flags=cv2.INTER_NEAREST, **kw)


if __name__ == "__main__":
    out = {}
    draws(out)
    if real_cv2 is not None:
        opencv(out)
    else:
        print("OpenCV is not installed: the cv2_* arrays are not recorded (their test skips)")
    path = os.path.join(HERE, "data_layer_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", len(out), "arrays")
