"""Generates tests/golden/train_frontend_vectors.npz by IMPORTING THE REFERENCE (only possible where /root/reference exists): the
reference's own functions for the training step between the renderer and the Canny detector
(train/train_poseMF_shapeGaussian_net.py:181-183 and :199-244), run on the CPU on tests/train_frontend_scenario.py's seeded inputs
after np.random.seed(s); torch.manual_seed(s).  What is committed is data: the reference's outputs only.

    python tests/golden/make_train_frontend_golden.py

Per golden case <c>: <c>_seg_crop, <c>_seg_aug (int8: the values are whole numbers -1..24), <c>_rgb_in, <c>_joints2D,
<c>_joints2D_input, <c>_vis, <c>_counts (pixels of the 14-part labels 3, 5, 7, 9, 11, 12, 13, 14), and <c>_next_np / <c>_next_torch, one
further draw from each global generator after the step (the state the reference leaves them in).

cv2 and torchgeometry are absent here and are not called on this path: both are stubbed as empty modules.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
for name in ("torchgeometry", "torchgeometry.image", "torchgeometry.image.gaussian"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchgeometry.image.gaussian"].gaussian_blur = None          # rgb_augmentation.py:3; random_gaussian_blur is not on the path
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from utils.augmentation.proxy_rep_augmentation import augment_proxy_representation, random_extreme_crop  # noqa: E402
from utils.augmentation.rgb_augmentation import augment_rgb  # noqa: E402
from utils.image_utils import batch_add_rgb_background, batch_crop_pytorch_affine  # noqa: E402
from utils.joints2d_utils import check_joints2d_occluded_torch, check_joints2d_visibility_torch  # noqa: E402
from utils.label_conversions import convert_densepose_seg_to_14part_labels  # noqa: E402

import train_frontend_scenario as S  # noqa: E402


def step(inputs, cfg, D, W, H):
    """train/train_poseMF_shapeGaussian_net.py:181-183, :199-244 with device = 'cpu', the renderer's outputs given."""
    iuv_in, rgb_in, background, joints2d = (inputs[k].clone() for k in ("iuv", "rgb", "background", "joints2d"))
    B = iuv_in.shape[0]
    vis = check_joints2d_visibility_torch(joints2d, D)
    seg_extreme_crop = random_extreme_crop(seg=iuv_in[:, 0, :, :], extreme_crop_probability=cfg.PROXY_REP.EXTREME_CROP_PROB)
    crop = batch_crop_pytorch_affine(input_wh=(W, H), output_wh=(D, D), num_to_crop=B, device="cpu", rgb=rgb_in, iuv=iuv_in,
                                     joints2D=joints2d, bbox_determiner=seg_extreme_crop, orig_scale_factor=S.BBOX_SCALE_FACTOR,
                                     delta_scale_range=cfg.BBOX.DELTA_SCALE_RANGE, delta_centre_range=cfg.BBOX.DELTA_CENTRE_RANGE,
                                     out_of_frame_pad_val=-1)
    iuv_in, joints, rgb_in = crop["iuv"], crop["joints2D"], crop["rgb"]
    vis = check_joints2d_visibility_torch(joints, D, visibility=vis)
    seg14 = convert_densepose_seg_to_14part_labels(iuv_in[:, 0, :, :])
    vis = check_joints2d_occluded_torch(seg14, vis, pixel_count_threshold=S.COUNT_THRESHOLD)
    seg_aug, joints_input, vis = augment_proxy_representation(seg=iuv_in[:, 0, :, :], joints2D=joints, joints2D_visib=vis,
                                                              proxy_rep_augment_config=cfg.PROXY_REP)
    rgb_in = batch_add_rgb_background(backgrounds=background, rgb=rgb_in, seg=seg_aug)
    rgb_in, joints_input, vis = augment_rgb(rgb=rgb_in, joints2D=joints_input, joints2D_visib=vis, rgb_augment_config=cfg.RGB)
    counts = torch.stack([(seg14 == part).sum(dim=(1, 2)) for part in S.COUNTED_PARTS], dim=1)
    return dict(seg_crop=iuv_in[:, 0], seg_aug=seg_aug, rgb_in=rgb_in, joints2D=joints, joints2D_input=joints_input, vis=vis,
                counts=counts)


def main():
    out = {}
    for name in S.GOLDEN_CASES:
        case = S.CASES[name]
        inputs = S.make_inputs(case)
        np.random.seed(case.seed)
        torch.manual_seed(case.seed)
        r = step(inputs, S.augment_cfg(case.cfg), case.D, case.W, case.H)
        out[name + "_next_np"] = np.float64(np.random.rand())
        out[name + "_next_torch"] = torch.rand(1).numpy()
        for k in S.GOLDEN_KEYS:
            v = r[k].numpy()
            if k in ("seg_crop", "seg_aug"):
                assert (v == np.round(v)).all() and v.min() >= -1 and v.max() <= 24
                v = v.astype(np.int8)
            out["%s_%s" % (name, k)] = v
    path = os.path.join(HERE, "train_frontend_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
