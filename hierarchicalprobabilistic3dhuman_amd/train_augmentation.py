"""The synthetic-data training front end: everything the reference's training step does between the renderer's output and
``proxy_rep_input`` (train/train_poseMF_shapeGaussian_net.py:199-256) -- extreme-crop selection, bounding box from the part
segmentation, augmented affine crop of IUV / RGB / 2D joints, the visibility and body-part occlusion checks, the
proxy-representation augmentations, the background composite and the RGB augmentations (utils/augmentation/proxy_rep_augmentation.py,
utils/augmentation/rgb_augmentation.py, utils/image_utils.py:234-372 with a bbox_determiner, utils/joints2d_utils.py).

Two halves:

* ``draw_augment_plan`` draws EVERY random number of a step on the host, from numpy's and torch's CPU generators, in exactly the
  order in which the reference draws them with device='cpu', and turns them into decisions: class masks, half-open ranges,
  thresholds, factors -- one record of ``PLAN_WORDS`` 32-bit words per image (layout: include/hps.h), page-locked, uploaded with one
  asynchronous copy.
* three launches (csrc/train_frontend.hip: hps_seg_bbox_affine, hps_train_crop_augment, hps_train_joints2d) apply a plan on the
  device; ``SyntheticTrainFrontEnd`` chains them with the Canny and heat-map kernels.  The reference-named functions below are thin
  wrappers over the same kernels with some stages switched off.  There is no CPU path.
"""
import numpy as np
import torch

from . import _capi
from .label_conversions import TWENTYFOUR_PART_SEG_TO_COCO_JOINTS_MAP, make_proxy_representation

PLAN_WORDS = 84
NUM_JOINTS = 17
NUM_PART_COUNTS = 8
# word offsets (include/hps.h)
_CROP_MASK, _SEG_MASK, _DSCALE, _DCENTRE, _BOX, _SEG_OCC, _RGB_OCC, _SEG_JT, _RGB_JT, _INVIS, _CHAN, _SWAP, _DEV = (
    0, 1, 2, 3, 5, 9, 15, 21, 25, 29, 30, 33, 50)

# stages of hps_train_crop_augment / hps_train_joints2d (include/hps.h)
RESAMPLE, CLASS_MASK, CROP_CLASS_MASK, SEG_OCCLUDE, BACKGROUND, RGB_OCCLUDE, RGB_NOISE, COUNT, COUNT14 = 1, 2, 4, 8, 16, 32, 64, 128, 256
J_PRE_VIS, J_AFFINE, J_POST_VIS, J_OCCLUDED, J_SEG_AUG, J_RGB_AUG = 1, 2, 4, 8, 16, 32
FUSED_STAGES = RESAMPLE | COUNT | CLASS_MASK | SEG_OCCLUDE | BACKGROUND | RGB_OCCLUDE | RGB_NOISE
FUSED_J_STAGES = J_PRE_VIS | J_AFFINE | J_POST_VIS | J_OCCLUDED | J_SEG_AUG | J_RGB_AUG

# utils/augmentation/proxy_rep_augmentation.py:246-251
REMOVE_LEGS_CLASSES = (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)
REMOVE_LEGS_ARMS_CLASSES = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 19, 20, 21, 22)
# :11-12
_HIP_JOINTS = (11, 12)
_OTHER_JOINTS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16)


def _class_bits(classes):
    bits = 0
    for c in classes:
        c = int(c)
        if not 0 < c < 32:
            raise ValueError("part class %d cannot be held in a plan's class mask (1..31)" % c)
        bits |= 1 << c
    return bits


def _range(start, stop, size):
    """A Python slice of the reference, ``[start:stop]`` over ``size`` elements, as the half-open range the kernels see."""
    lo, hi, _ = slice(None if start is None else int(start), None if stop is None else int(stop)).indices(int(size))
    return (lo, hi) if lo < hi else (0, 0)


class AugmentPlan:
    """The decisions of one training step for ``batch_size`` images of side ``img_wh``: ``words`` (B, PLAN_WORDS) int32 on the host
    (page-locked when a device is present), ``floats`` the same memory seen as float32.  A fresh plan changes nothing (no class
    masked, empty ranges, tests off, identity swaps, zero deviations, unit factors)."""

    def __init__(self, batch_size, img_wh):
        self.batch_size, self.img_wh = int(batch_size), int(img_wh)
        self.tensor = torch.zeros(self.batch_size, PLAN_WORDS, dtype=torch.int32)
        if torch.cuda.is_available():
            self.tensor = self.tensor.pin_memory()
        self.words = self.tensor.numpy()
        self.floats = self.words.view(np.float32)
        inf = np.float32(np.inf)
        for base in (_SEG_JT, _RGB_JT):
            self.floats[:, base:base + 4] = (inf, -inf, -inf, inf)
        self.floats[:, _CHAN:_CHAN + 3] = 1.0
        self.words[:, _SWAP:_SWAP + NUM_JOINTS] = np.arange(NUM_JOINTS, dtype=np.int32)

    def upload(self, out=None):
        """One asynchronous copy of the whole block to the current device (into ``out`` (B, PLAN_WORDS) int32 when given)."""
        if out is None:
            out = torch.empty(self.batch_size, PLAN_WORDS, device="cuda", dtype=torch.int32)
        out.copy_(self.tensor, non_blocking=True)
        return out


def _rand(generator, *shape):
    return torch.rand(*shape, generator=generator, dtype=torch.float32)


def _np_random(np_random):
    return np.random if np_random is None else np_random


def draw_extreme_crop(plan, extreme_crop_probability, generator=None):
    """random_extreme_crop's draw (proxy_rep_augmentation.py:259-262): legs below p/2, legs and arms between p/2 and p."""
    r = _rand(generator, plan.batch_size)
    legs = (r < extreme_crop_probability * 0.5).numpy()
    legs_arms = torch.logical_and(r > extreme_crop_probability * 0.5, r < extreme_crop_probability).numpy()
    plan.words[:, _CROP_MASK] = np.where(legs, _class_bits(REMOVE_LEGS_CLASSES), 0) | np.where(legs_arms, _class_bits(REMOVE_LEGS_ARMS_CLASSES), 0)


def draw_bbox(plan, delta_scale_range, delta_centre_range, generator=None):
    """utils/image_utils.py:315-326: the scale draw, then the centre draw, each only when its range is given."""
    if delta_scale_range is not None:
        l, h = delta_scale_range
        plan.floats[:, _DSCALE] = ((h - l) * _rand(generator, plan.batch_size) + l).numpy()
    if delta_centre_range is not None:
        l, h = delta_centre_range
        plan.floats[:, _DCENTRE:_DCENTRE + 2] = ((h - l) * _rand(generator, plan.batch_size, 2) + l).numpy()


def _draw_half_occlusions(plan, cfg, occ, jt, np_random):
    """random_occlude_bottom_half / _top_half / _vertical_half (proxy_rep_augmentation.py:121-183 and rgb_augmentation.py:6-68 draw
    alike): rand(B), per hit image randint, for the vertical one a further rand()."""
    B, wh = plan.batch_size, plan.img_wh
    rv = np_random.rand(B)
    for i in range(B):
        if rv[i] < cfg.OCCLUDE_BOTTOM_PROB:
            occlude_from = int(wh / 2.0) + np_random.randint(low=-int(wh / 5.), high=int(wh / 5.))
            plan.words[i, occ:occ + 2] = _range(occlude_from, None, wh)
            plan.floats[i, jt] = occlude_from
    rv = np_random.rand(B)
    for i in range(B):
        if rv[i] < cfg.OCCLUDE_TOP_PROB:
            occlude_up_to = int(wh / 2.0) + np_random.randint(low=-int(wh / 5.), high=int(wh / 5.))
            plan.words[i, occ + 2:occ + 4] = _range(None, occlude_up_to, wh)
            plan.floats[i, jt + 1] = occlude_up_to
    rv = np_random.rand(B)
    for i in range(B):
        if rv[i] < cfg.OCCLUDE_VERTICAL_PROB:
            occlude_up_to = int(wh / 2.0) + np_random.randint(low=-int(wh / 30.), high=int(wh / 30.))
            if np_random.rand() > 0.5:
                plan.words[i, occ + 4:occ + 6] = _range(None, occlude_up_to, wh)
                plan.floats[i, jt + 2] = occlude_up_to
            else:
                plan.words[i, occ + 4:occ + 6] = _range(occlude_up_to, None, wh)
                plan.floats[i, jt + 3] = occlude_up_to


def draw_proxy_rep(plan, cfg, np_random=None, generator=None):
    """augment_proxy_representation's draws, function by function (proxy_rep_augmentation.py:186-235)."""
    rs = _np_random(np_random)
    B, wh = plan.batch_size, plan.img_wh
    assert len(cfg.REMOVE_PARTS_CLASSES) == len(cfg.REMOVE_PARTS_PROBS)
    seg_mask = np.zeros(B, dtype=np.int64)
    invis = np.zeros(B, dtype=np.int64)
    for cls, prob in zip(cfg.REMOVE_PARTS_CLASSES, cfg.REMOVE_PARTS_PROBS):                       # :27-59
        rv = rs.rand(B) < prob
        seg_mask |= np.where(rv, _class_bits([cls]), 0)
        if cls in TWENTYFOUR_PART_SEG_TO_COCO_JOINTS_MAP:
            rvj = np.logical_and(rv, rs.rand(B) < cfg.REMOVE_APPENDAGE_JOINTS_PROB)
            invis |= np.where(rvj, 1 << TWENTYFOUR_PART_SEG_TO_COCO_JOINTS_MAP[cls], 0)
    plan.words[:, _SEG_MASK] = seg_mask.astype(np.int32)
    centre, dim = wh / 2, cfg.OCCLUDE_BOX_DIM                                                     # :94-118 (x_h < x_l, as there)
    x_h, x_l = centre - 0.3 * wh / 2, centre + 0.3 * wh / 2
    y_h, y_l = centre - 0.3 * wh / 2, centre + 0.3 * wh / 2
    x = (x_h - x_l) * rs.rand(B) + x_l
    y = (y_h - y_l) * rs.rand(B) + y_l
    x1, x2 = (x - dim / 2).astype(np.int16), (x + dim / 2).astype(np.int16)
    y1, y2 = (y - dim / 2).astype(np.int16), (y + dim / 2).astype(np.int16)
    rv = rs.rand(B)
    for i in range(B):
        if rv[i] < cfg.OCCLUDE_BOX_PROB:
            rows, cols = _range(x1[i], x2[i], wh), _range(y1[i], y2[i], wh)                      # the first index is the row
            if rows != (0, 0) and cols != (0, 0):
                plan.words[i, _BOX:_BOX + 4] = rows + cols
    for a, b in cfg.JOINTS_TO_SWAP:                                                               # :73-91
        rv = rs.rand(B) < cfg.JOINTS_SWAP_PROB
        src = plan.words[:, _SWAP:_SWAP + NUM_JOINTS]
        sa, sb = src[rv, a].copy(), src[rv, b].copy()
        src[rv, a], src[rv, b] = sb, sa
    l, h = cfg.DELTA_J2D_DEV_RANGE                                                                # :7-24, both with this range (:212-214)
    dev = plan.floats[:, _DEV:_DEV + 2 * NUM_JOINTS].reshape(B, NUM_JOINTS, 2)
    dev[:, _OTHER_JOINTS, :] = ((h - l) * _rand(generator, B, len(_OTHER_JOINTS), 2) + l).numpy()
    dev[:, _HIP_JOINTS, :] = ((h - l) * _rand(generator, B, len(_HIP_JOINTS), 2) + l).numpy()
    for joint in cfg.REMOVE_JOINTS_INDICES:                                                       # :62-70
        invis |= np.where(rs.rand(B) < cfg.REMOVE_JOINTS_PROB, 1 << joint, 0)
    plan.words[:, _INVIS] = invis.astype(np.int32)
    _draw_half_occlusions(plan, cfg, _SEG_OCC, _SEG_JT, rs)


def draw_rgb(plan, cfg, np_random=None, generator=None):
    """augment_rgb's draws (rgb_augmentation.py:92-115)."""
    _draw_half_occlusions(plan, cfg, _RGB_OCC, _RGB_JT, _np_random(np_random))
    l, h = 1 - cfg.PIXEL_CHANNEL_NOISE, 1 + cfg.PIXEL_CHANNEL_NOISE
    plan.floats[:, _CHAN:_CHAN + 3] = ((h - l) * _rand(generator, plan.batch_size, 3) + l).numpy()


def draw_augment_plan(cfg, batch_size, img_wh, np_random=None, generator=None):
    """Every random number of one training step (train/train_poseMF_shapeGaussian_net.py:199-244), drawn in the reference's order
    from ``np_random`` (default: numpy's global state) and ``generator`` (default: torch's CPU generator), as decisions.  ``cfg``:
    anything with the attributes of TRAIN.SYNTH_DATA.AUGMENT (PROXY_REP, RGB, BBOX).  After ``np.random.seed(s);
    torch.manual_seed(s)`` the plan holds the very numbers the reference uses after the same two calls, and leaves both generators
    where the reference leaves them."""
    plan = AugmentPlan(batch_size, img_wh)
    draw_extreme_crop(plan, cfg.PROXY_REP.EXTREME_CROP_PROB, generator)
    draw_bbox(plan, cfg.BBOX.DELTA_SCALE_RANGE, cfg.BBOX.DELTA_CENTRE_RANGE, generator)
    draw_proxy_rep(plan, cfg.PROXY_REP, np_random, generator)
    draw_rgb(plan, cfg.RGB, np_random, generator)
    return plan


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
def _part_plane(t, what):
    """(pointer tensor, batch stride, B, H, W) of a part plane given as (B,H,W) or as a whole (B,3,H,W) IUV batch (channel 0)."""
    _capi.require_device(t, what)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _capi.HpsError("%s must be contiguous float32" % what)
    if t.dim() == 4:
        return t, t.shape[1] * t.shape[2] * t.shape[3], t.shape[0], t.shape[2], t.shape[3]
    if t.dim() != 3:
        raise _capi.HpsError("%s must be (B,H,W) or (B,C,H,W)" % what)
    return t, t.shape[1] * t.shape[2], t.shape[0], t.shape[1], t.shape[2]


def _plan_dev(plan, B):
    if plan is None:
        return None
    if isinstance(plan, AugmentPlan):
        if plan.batch_size != B:
            raise _capi.HpsError("plan drawn for %d images, batch has %d" % (plan.batch_size, B))
        return plan.upload()
    _capi.require_device(plan, "plan")
    assert plan.shape == (B, PLAN_WORDS)
    return plan


def seg_bbox_affine(part, plan_dev, out_wh, orig_scale_factor, ws=None, affine=None, theta=None, status=None, part_counts=None):
    """hps_seg_bbox_affine on a (B,H,W) plane or a (B,3,H,W) IUV batch -> (affine (B,2,3), theta (B,4), status (B,) int32)."""
    t, stride, B, H, W = _part_plane(part, "part")
    dev = t.device
    if ws is None:
        ws = torch.empty(_capi.query_workspace(_capi.WS_SEG_BBOX, B) // 4, device=dev, dtype=torch.int32)
    affine = torch.empty(B, 2, 3, device=dev) if affine is None else affine
    theta = torch.empty(B, 4, device=dev) if theta is None else theta
    status = torch.empty(B, device=dev, dtype=torch.int32) if status is None else status
    I = _capi.iptr
    _capi.call("hps_seg_bbox_affine", _capi.ptr(t), stride, I(plan_dev), B, H, W, int(out_wh), float(orig_scale_factor), I(ws),
               _capi.ptr(affine), _capi.ptr(theta), I(status), I(part_counts), _capi.stream())
    return affine, theta, status


def crop_augment(part, rgb, background, theta, plan_dev, out_wh, stages, rgb_out=None, part_counts=None, part_crop=None,
                 part_aug=None):
    """hps_train_crop_augment; ``part`` as for seg_bbox_affine (or None), ``rgb`` (B,3,H,W) or None.  Outputs are out_wh x out_wh
    with the RESAMPLE stage, else H x W (``out_wh`` is then ignored)."""
    P, I = _capi.ptr, _capi.iptr
    if part is not None:
        t, stride, B, H, W = _part_plane(part, "part")
    else:
        t, stride = None, 0
        _capi.require_device(rgb, "rgb")
        B, _, H, W = rgb.shape
    if rgb is not None and tuple(rgb.shape) != (B, 3, H, W):
        raise _capi.HpsError("rgb must be (B,3,H,W) with the part plane's B, H, W")
    D = int(out_wh)
    oh, ow = (D, D) if stages & RESAMPLE else (H, W)
    if background is not None and tuple(background.shape) != (B, 3, oh, ow):
        raise _capi.HpsError("background must be (B,3,%d,%d)" % (oh, ow))
    for o, shape in ((rgb_out, (B, 3, oh, ow)), (part_crop, (B, oh, ow)), (part_aug, (B, oh, ow)), (part_counts, (B, NUM_PART_COUNTS))):
        assert o is None or (tuple(o.shape) == shape and o.is_contiguous())
    _capi.call("hps_train_crop_augment", P(t), stride, P(rgb), P(background), P(theta), I(plan_dev), B, H, W, D, int(stages),
               P(rgb_out), I(part_counts), P(part_crop), P(part_aug), _capi.stream())


def _u8(vis, what="visibility"):
    if vis is None:
        return None
    _capi.require_device(vis, what)
    if vis.dtype == torch.bool:
        vis = vis.contiguous().view(torch.uint8)
    if vis.dtype != torch.uint8:
        raise _capi.HpsError("%s must be a bool (or uint8) tensor" % what)
    return vis.contiguous()


def joints2d(joints, vis_in, affine, part_counts, plan_dev, img_wh, stages, pixel_count_threshold=50, joints_target=None,
             joints_input=None, vis=None, vis_u8=None):
    """hps_train_joints2d on (B,17,2) joints."""
    _capi.require_device(joints, "joints2D")
    j = _capi.f32c(joints)
    if j.dim() != 3 or j.shape[1:] != (NUM_JOINTS, 2):
        raise _capi.HpsError("joints2D must be (B,17,2) COCO joints")
    P, I = _capi.ptr, _capi.iptr
    U = lambda t: _capi.ptr(t, torch.uint8)
    _capi.call("hps_train_joints2d", P(j), U(_u8(vis_in)), P(affine), I(part_counts), I(plan_dev), j.shape[0], NUM_JOINTS,
               float(img_wh), int(pixel_count_threshold), int(stages), P(joints_target), P(joints_input), P(vis), U(vis_u8),
               _capi.stream())


class SyntheticTrainFrontEnd:
    """train/train_poseMF_shapeGaussian_net.py:199-256 minus the renderer, on the device: from the renderer's ``iuv`` (B,3,H,W; the
    part index in channel 0) and ``rgb`` (B,3,H,W), a ``background`` (B,3,D,D) and the projected COCO ``joints2d`` (B,17,2) to the
    network's input.  Five launches and one asynchronous upload per call, no torch kernel and no host round trip in steady state:
    hps_seg_bbox_affine, hps_train_crop_augment, hps_train_joints2d, then CannyEdgeDetector.edge_map_into and
    make_proxy_representation(out=...).  ``cfg``: TRAIN.SYNTH_DATA.AUGMENT (PROXY_REP, RGB, BBOX).  Output buffers are owned per
    (B, H, W) and overwritten by the next call of the same shape.

    An image whose (extreme-cropped) segmentation is empty is where the reference raises; here its box is the whole frame and a
    status word is set: ``check()`` reads the words of the last call and raises (one synchronisation, at the caller's request)."""

    def __init__(self, cfg, img_wh, edge_detector, heatmap_std, edge_nms, bbox_scale_factor=1.2, pixel_count_threshold=50):
        self.cfg, self.img_wh, self.edge_detector = cfg, int(img_wh), edge_detector
        self.heatmap_std, self.edge_nms = float(heatmap_std), bool(edge_nms)
        self.bbox_scale_factor, self.pixel_count_threshold = float(bbox_scale_factor), int(pixel_count_threshold)
        self._bufs = {}
        self._last = None

    def _buffers(self, B, H, W, dev):
        key = (B, H, W, dev.index)
        bufs = self._bufs.get(key)
        if bufs is None:
            D = self.img_wh
            f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            i = lambda *s: torch.empty(*s, device=dev, dtype=torch.int32)
            bufs = dict(plan=i(B, PLAN_WORDS), ws=i(_capi.query_workspace(_capi.WS_SEG_BBOX, B) // 4), affine=f(B, 2, 3),
                        theta=f(B, 4), status=i(B), counts=i(B, NUM_PART_COUNTS), rgb_in=f(B, 3, D, D), proxy=f(B, NUM_JOINTS + 1, D, D),
                        joints_target=f(B, NUM_JOINTS, 2), joints_input=f(B, NUM_JOINTS, 2), vis=f(B, NUM_JOINTS),
                        vis_u8=torch.empty(B, NUM_JOINTS, device=dev, dtype=torch.uint8), seg_crop=None, seg_aug=None)
            self._bufs[key] = bufs
        return bufs

    def __call__(self, iuv, rgb, background, joints2d_in, plan=None, return_seg_aug=False, return_seg_crop=False):
        for t, what in ((iuv, "iuv"), (rgb, "rgb"), (background, "background"), (joints2d_in, "joints2d")):
            _capi.require_device(t, what)
        part, _, B, H, W = _part_plane(iuv, "iuv")
        D = self.img_wh
        bufs = self._buffers(B, H, W, part.device)
        if plan is None:
            plan = draw_augment_plan(self.cfg, B, D)
        if plan.batch_size != B or plan.img_wh != D:
            raise _capi.HpsError("plan drawn for (%d, %d), called with (%d, %d)" % (plan.batch_size, plan.img_wh, B, D))
        plan.upload(bufs["plan"])
        for name, want in (("seg_aug", return_seg_aug), ("seg_crop", return_seg_crop)):
            if want and bufs[name] is None:
                bufs[name] = torch.empty(B, D, D, device=part.device, dtype=torch.float32)
        seg_bbox_affine(part, bufs["plan"], D, self.bbox_scale_factor, bufs["ws"], bufs["affine"], bufs["theta"], bufs["status"],
                        bufs["counts"])
        crop_augment(part, _capi.f32c(rgb), _capi.f32c(background), bufs["theta"], bufs["plan"], D, FUSED_STAGES, bufs["rgb_in"],
                     bufs["counts"], bufs["seg_crop"] if return_seg_crop else None, bufs["seg_aug"] if return_seg_aug else None)
        joints2d(joints2d_in, None, bufs["affine"], bufs["counts"], bufs["plan"], D, FUSED_J_STAGES, self.pixel_count_threshold,
                 bufs["joints_target"], bufs["joints_input"], bufs["vis"], bufs["vis_u8"])
        self.edge_detector.edge_map_into(bufs["rgb_in"], bufs["proxy"], nms=self.edge_nms)
        make_proxy_representation(None, bufs["joints_input"], bufs["vis"], D, self.heatmap_std, out=bufs["proxy"])
        self._last = bufs
        out = {"proxy_rep_input": bufs["proxy"], "rgb_in": bufs["rgb_in"], "joints2D": bufs["joints_target"],
               "joints2D_input": bufs["joints_input"], "joints2D_vis": bufs["vis_u8"].view(torch.bool)}
        if return_seg_aug:
            out["seg_aug"] = bufs["seg_aug"]
        if return_seg_crop:
            out["seg_crop"] = bufs["seg_crop"]
        return out

    def part_counts(self):
        """(B, 8) int32 pixel counts of the 14-part labels 3, 5, 7, 9, 11, 12, 13, 14 in the last call's cropped segmentation."""
        return self._last["counts"]

    def status(self):
        """(B,) int32 of the last call: 1 where the image had no body pixel to take its box from."""
        return self._last["status"]

    def check(self):
        """Raise if an image of the last call had no body pixel to take its box from (synchronises)."""
        if self._last is None:
            return
        bad = torch.nonzero(self._last["status"]).flatten().tolist()
        if bad:
            raise _capi.HpsError("no body pixel left to determine the bounding box of image(s) %s (the reference raises at "
                                 "utils/image_utils.py:304); their crop is the whole frame" % bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference's names, over the same kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def random_extreme_crop(seg, extreme_crop_probability=0.05, plan=None, generator=None):
    """proxy_rep_augmentation.py:238-275: ``seg`` (B,H,W) with the legs (or legs and arms) of the chosen images set to 0 -- the plane
    the bounding box is then taken from.  ``plan``: use its decision instead of drawing one."""
    t, _, B, H, W = _part_plane(seg, "seg")
    if plan is None:
        plan = AugmentPlan(B, W)
        draw_extreme_crop(plan, extreme_crop_probability, generator)
    out = torch.empty_like(t)
    crop_augment(t, None, None, None, _plan_dev(plan, B), W, CROP_CLASS_MASK, part_aug=out)
    return out


def batch_crop_pytorch_affine_train(input_wh, output_wh, num_to_crop, device=None, iuv=None, joints2D=None, rgb=None,
                                    bbox_determiner=None, orig_scale_factor=1.2, delta_scale_range=None, delta_centre_range=None,
                                    out_of_frame_pad_val=-1, plan=None, generator=None):
    """utils/image_utils.py:234-372 as the training step calls it (train/train_poseMF_shapeGaussian_net.py:203-214): the box from
    ``bbox_determiner`` (B,H,W) (else from channel 0 of ``iuv``), augmented by the delta ranges (or by ``plan``), the crop of ``iuv``,
    ``rgb`` and ``joints2D`` to a square ``output_wh``.  Returns {'iuv': (B,1,D,D), 'rgb', 'joints2D'}: ONLY CHANNEL 0 of iuv is
    cropped -- the part index, the one channel training reads (:224, :231); out-of-frame pixels are -1."""
    if out_of_frame_pad_val != -1:
        raise NotImplementedError("batch_crop_pytorch_affine_train: out_of_frame_pad_val must be -1, as training passes it")
    if output_wh[0] != output_wh[1]:
        raise NotImplementedError("batch_crop_pytorch_affine_train: square outputs only")
    if iuv is None:
        raise NotImplementedError("batch_crop_pytorch_affine_train: iuv is needed (boxes from joints or seg are not a training path)")
    part, _, B, H, W = _part_plane(iuv, "iuv")
    assert B == num_to_crop and (W, H) == tuple(int(v) for v in input_wh)
    D = int(output_wh[0])
    if plan is None:
        plan = AugmentPlan(B, D)
        draw_bbox(plan, delta_scale_range, delta_centre_range, generator)
        plan_dev = plan.upload()
        plan_dev[:, _CROP_MASK] = 0
    else:
        plan_dev = _plan_dev(plan, B).clone()
        plan_dev[:, _CROP_MASK] = 0                       # the determiner already has the extreme-crop classes removed
    affine, theta, status = seg_bbox_affine(part if bbox_determiner is None else bbox_determiner, plan_dev, D, orig_scale_factor)
    out = {"iuv": torch.empty(B, 1, D, D, device=part.device), "status": status}
    if rgb is not None:
        out["rgb"] = torch.empty(B, 3, D, D, device=part.device)
    crop_augment(part, None if rgb is None else _capi.f32c(rgb), None, theta, None, D, RESAMPLE, out.get("rgb"),
                 part_crop=out["iuv"].view(B, D, D))
    if joints2D is not None:
        out["joints2D"] = torch.empty(B, NUM_JOINTS, 2, device=part.device)
        joints2d(joints2D, None, affine, None, None, D, J_AFFINE, joints_target=out["joints2D"])
    return out


def augment_proxy_representation(seg, joints2D, joints2D_visib, proxy_rep_augment_config=None, plan=None, np_random=None,
                                 generator=None):
    """proxy_rep_augmentation.py:186-235 -> (new seg, new joints2D, new visibility (bool)); inputs are left as they are."""
    t, _, B, H, W = _part_plane(seg, "seg")
    if H != W:
        raise _capi.HpsError("seg must be square")
    if plan is None:
        plan = AugmentPlan(B, W)
        draw_proxy_rep(plan, proxy_rep_augment_config, np_random, generator)
    plan_dev = _plan_dev(plan, B)
    new_seg = torch.empty_like(t)
    crop_augment(t, None, None, None, plan_dev, W, CLASS_MASK | SEG_OCCLUDE, part_aug=new_seg)
    new_j = torch.empty(B, NUM_JOINTS, 2, device=t.device)
    new_vis = torch.empty(B, NUM_JOINTS, device=t.device, dtype=torch.uint8)
    joints2d(joints2D, joints2D_visib, None, None, plan_dev, W, J_SEG_AUG, joints_input=new_j, vis_u8=new_vis)
    return new_seg, new_j, new_vis.view(torch.bool)


def augment_rgb(rgb, joints2D, joints2D_visib, rgb_augment_config=None, plan=None, np_random=None, generator=None):
    """rgb_augmentation.py:92-115 -> (new rgb, joints2D, new visibility (bool)); ``rgb`` (B,3,D,D) is left as it is (the reference
    writes into it)."""
    _capi.require_device(rgb, "rgb")
    x = _capi.f32c(rgb)
    B, _, H, W = x.shape
    if H != W:
        raise _capi.HpsError("rgb must be square")
    if plan is None:
        plan = AugmentPlan(B, W)
        draw_rgb(plan, rgb_augment_config, np_random, generator)
    plan_dev = _plan_dev(plan, B)
    out = torch.empty_like(x)
    crop_augment(None, x, None, None, plan_dev, W, RGB_OCCLUDE | RGB_NOISE, rgb_out=out)
    new_vis = torch.empty(B, NUM_JOINTS, device=x.device, dtype=torch.uint8)
    joints2d(joints2D, joints2D_visib, None, None, plan_dev, W, J_RGB_AUG, vis_u8=new_vis)
    return out, joints2D, new_vis.view(torch.bool)
