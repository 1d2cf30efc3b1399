"""Generates tests/golden/predict_frontend_vectors.npz by IMPORTING THE REFERENCE (only possible where /root/reference exists): the
reference's own predict/predict_hrnet.predict_hrnet and the second utils/image_utils.batch_crop_pytorch_affine of
predict/predict_poseMF_shapeGaussian_net.py:73-89, run on the CPU on tests/predict_frontend_scenario.py's seeded cases.  The heat maps
are given data (the injected ``hrnet_model`` returns them), so no network is involved.  What is committed is data: the inputs and the
reference's outputs only.

    python tests/golden/make_predict_frontend_golden.py

Per case <c>: <c>_image (H,W,3) uint8, <c>_heatmaps (1,17,16,8), and the reference's <c>_joints2D, <c>_joints2Dconfs, <c>_cropped_image,
<c>_bbox_centre, <c>_bbox_height, <c>_bbox_width (predict_hrnet's dict) and <c>_proxy_rgb, <c>_proxy_joints2D (the second crop).

cv2 and torchvision are absent here; neither is called for anything but transforms.Normalize, which this script's own minimal
module supplies.
"""
import os
import sys
import types
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=t.dtype, device=t.device)[:, None, None]
        std = torch.as_tensor(self.std, dtype=t.dtype, device=t.device)[:, None, None]
        return (t - mean) / std


sys.modules.setdefault("cv2", types.ModuleType("cv2"))
_tv, _tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
_tr.Normalize = _Normalize
_tv.transforms = _tr
sys.modules.setdefault("torchvision", _tv)
sys.modules.setdefault("torchvision.transforms", _tr)
sys.path.insert(0, REF)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from predict.predict_hrnet import predict_hrnet  # noqa: E402
from utils.image_utils import batch_crop_pytorch_affine  # noqa: E402

import predict_frontend_scenario as S  # noqa: E402


def run(case):
    cfg = NS(MODEL=NS(IMAGE_SIZE=list(S.GOLDEN_IMAGE_SIZE), HEATMAP_SIZE=list(S.GOLDEN_HEATMAP_SIZE)))
    u8 = S.case_image(case)
    heat = S.special_heatmaps(17, S.GOLDEN_HEATMAP_SIZE[1], S.GOLDEN_HEATMAP_SIZE[0], case.seed)
    image = torch.from_numpy(u8.transpose(2, 0, 1)).float() / 255.0                          # predict/...:63
    det = S.case_det(case)
    detector = None
    if det is not None:
        detector = lambda batch: [{"boxes": det[0].clone(), "labels": det[1].clone(), "scores": det[2].clone()}]
    with torch.no_grad():
        hr = predict_hrnet(hrnet_model=lambda x: heat.clone(), hrnet_config=cfg, object_detect_model=detector, image=image,
                           object_detect_threshold=S.GOLDEN_THRESHOLD, bbox_scale_factor=S.GOLDEN_SCALE_FACTOR)
        crop = hr["cropped_image"]
        centre = torch.tensor([[crop.shape[1], crop.shape[2]]], dtype=torch.float32) * 0.5     # :73-79
        height = torch.tensor([crop.shape[1]], dtype=torch.float32)
        D = S.GOLDEN_PROXY
        second = batch_crop_pytorch_affine(input_wh=(cfg.MODEL.IMAGE_SIZE[0], cfg.MODEL.IMAGE_SIZE[1]), output_wh=(D, D), num_to_crop=1,
                                           device="cpu", joints2D=hr["joints2D"][None], rgb=crop[None], bbox_centres=centre,
                                           bbox_heights=height, bbox_widths=height, orig_scale_factor=1.0)     # :80-89
    out = {"image": u8, "heatmaps": heat.numpy()}
    for k in ("joints2D", "joints2Dconfs", "cropped_image", "bbox_centre", "bbox_height", "bbox_width"):
        out[k] = hr[k].numpy().astype(np.float32)
    out["proxy_rgb"], out["proxy_joints2D"] = second["rgb"][0].numpy(), second["joints2D"][0].numpy()
    return out


def main():
    out = {}
    for name, case in S.GOLDEN_CASES.items():
        for k, v in run(case).items():
            out["%s_%s" % (name, k)] = v
    path = os.path.join(HERE, "predict_frontend_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
