"""Silhouette masks, targets and counts for hps_silhouette_iou (tests/test_silhouette_host.py, tests/test_gpu_silhouette.py,
tests/dev/silhouette_time.py), derived from tests/render_scenario.py's restatement of the rasteriser.

The yardstick is the float64 ``render``: a pixel is set where round(iuv[..., 0]) != 0 (np.rint rounds half to even, as torch.round
and the device do).  The target of a case is the float64 mask rolled by (2, 3) pixels unless a test states another one; counts are
rows of [tp, fp, tn, fn] as metrics/eval_metrics_tracker.py:297-304 forms them.

On every case below the float32 restatement's mask equals the float64 one in every pixel and both equal (pix_to_face >= 0)
(tests/test_silhouette_host.py asserts it), so exact equality with the float64 mask is what the device is held to.
"""
import functools

import numpy as np

import render_scenario as S

ROLL = (2, 3)
CLOSED_FORM_TOTALS = {"shared_edge": 56, "coincident": 28, "behind": 28, "zero_area": 28, "whole_image_exact": 64, "whole_image": 1600}
# counts [tp, fp, tn, fn] per image against the rolled float64 mask
ROLLED_COUNTS = {
    "w16_f13_b1": [[6, 20, 210, 20]],
    "w16_f2400_b1": [[10, 23, 200, 23]],
    "w40_f257_b3": [[234, 79, 1208, 79], [141, 63, 1333, 63], [0, 0, 1600, 0]],
    "w36_f257_b2": [[236, 80, 900, 80], [138, 61, 1036, 61]],
    "w64_f2400_b3_ortho": [[567, 110, 3309, 110], [497, 130, 3339, 130], [692, 134, 3136, 134]],
}
CASES = sorted(CLOSED_FORM_TOTALS) + sorted(ROLLED_COUNTS)


def mask_of(iuv):
    """convert_multiclass_to_binary_labels(iuv[..., 0].round()): (B,W,W) bool."""
    return np.rint(np.asarray(iuv)[..., 0]) != 0


def counts_of(mask, target):
    """(B,W,W) masks against (B,W,W) targets, nonzero = foreground -> (B,4) int64 [tp, fp, tn, fn]."""
    m, t = np.asarray(mask) != 0, np.asarray(target) != 0
    return np.stack([(m & t).sum(axis=(1, 2)), (m & ~t).sum(axis=(1, 2)), (~m & ~t).sum(axis=(1, 2)), (~m & t).sum(axis=(1, 2))],
                    axis=1).astype(np.int64)


def iou_of(counts):
    """tp / (tp + fp + fn) per row in float64; 0 / 0 is nan."""
    c = np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return c[:, 0] / (c[:, 0] + c[:, 1] + c[:, 3])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(scene, float32 mask, float64 mask, target uint8, float64 counts against it) of a case, computed once and shared: callers must
    not modify them."""
    scene, r32, r64 = S.reference(name)
    m32, m64 = mask_of(r32["iuv"]), mask_of(r64["iuv"])
    target = np.roll(m64, ROLL, axis=(1, 2)).astype(np.uint8)
    return scene, m32, m64, target, counts_of(m64, target)


def flipped(scene):
    """The scene with every vertex rotated by pi about x, (x, -y, -z): what flip_x_pi does inside the kernel."""
    from types import SimpleNamespace
    d = dict(vars(scene))
    d["vertices"] = scene.vertices * np.array([1.0, -1.0, -1.0], dtype=np.float32)
    return SimpleNamespace(**d)
