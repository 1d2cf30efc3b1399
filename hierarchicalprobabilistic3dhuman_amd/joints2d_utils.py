"""2D-joint visibility checks of the training step, with the names of the reference's utils/joints2d_utils.py, over
hps_train_joints2d (csrc/train_frontend.hip).  COCO joints (K = 17) on the device; there is no CPU path."""
import torch

from . import _capi
from . import train_augmentation as ta


def undo_keypoint_normalisation(normalised_keypoints, img_wh):
    """utils/joints2d_utils.py:5-10: [-1, 1] -> pixels."""
    return (normalised_keypoints + 1) * (img_wh / 2.0)


def check_joints2d_visibility_torch(joints2d, img_wh, visibility=None):
    """utils/joints2d_utils.py:13-26: (B,17) bool, False where a coordinate is > img_wh or < 0 (and where ``visibility`` already
    is).  Returns a new tensor; the reference writes into ``visibility``."""
    _capi.require_device(joints2d, "joints2d")
    out = torch.empty(joints2d.shape[0], ta.NUM_JOINTS, device=joints2d.device, dtype=torch.uint8)
    ta.joints2d(joints2d, visibility, None, None, None, img_wh, ta.J_PRE_VIS, vis_u8=out)
    return out.view(torch.bool)


def check_joints2d_occluded_torch(seg14part, vis, pixel_count_threshold=50):
    """utils/joints2d_utils.py:29-45: joints 7-10 and 13-16 stay visible only while their body part has more than
    ``pixel_count_threshold`` pixels in ``seg14part`` (B,D,D), a 14-part segmentation."""
    _capi.require_device(seg14part, "seg14part")
    s = _capi.f32c(seg14part)
    B, D = s.shape[0], s.shape[-1]
    counts = torch.zeros(B, ta.NUM_PART_COUNTS, device=s.device, dtype=torch.int32)
    ta.crop_augment(s, None, None, None, None, D, ta.COUNT14, part_counts=counts)
    out = torch.empty(B, ta.NUM_JOINTS, device=s.device, dtype=torch.uint8)
    ta.joints2d(torch.zeros(B, ta.NUM_JOINTS, 2, device=s.device), vis, None, counts, None, D, ta.J_OCCLUDED, pixel_count_threshold,
                vis_u8=out)
    return out.view(torch.bool)
