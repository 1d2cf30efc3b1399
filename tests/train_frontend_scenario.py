"""The synthetic-data training front end's references (tests/test_train_frontend_host.py, tests/test_gpu_train_frontend.py,
tests/dev/train_frontend_time.py).

``restate`` is a torch restatement of the reference's training step between the renderer's output and the Canny detector
(train/train_poseMF_shapeGaussian_net.py:199-244 with utils/augmentation/proxy_rep_augmentation.py, rgb_augmentation.py,
utils/image_utils.py:234-372, utils/joints2d_utils.py, utils/label_conversions.py:38-72), operation by operation, in a chosen dtype,
drawing its random numbers from a numpy RandomState and a torch CPU generator in the reference's order.  In float32 on the CPU it
reproduces tests/golden/train_frontend_vectors.npz (the reference's own functions, tests/golden/make_train_frontend_golden.py) bit for
bit; in float64 it is the truth the device is measured against.  Random DRAWS are made in float32, as the reference makes them, and
cast: the two dtypes see the same deltas, deviations and factors.

Inputs are generated from the case's seed, never stored: a figure of 24 labelled blobs of seeded sizes on a background of zeros (so
that some 14-part counts fall on each side of the 50-pixel threshold), random RGB and background, 17 joints spread over 1.4 frame
widths so that some lie outside the frame before the crop and more after it.

``apply_plan`` is the other direction: what a plan's record means, applied on the host to the restatement's intermediate results --
the check that draw_augment_plan's DECISIONS are the reference's.

The bound for float outputs is the project's standing rule:
    bound = 4 * max(e_cpu32, 2**-23 * max|y64|)        e_cpu32 = max|restate(float32) - restate(float64)|
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
TIE_MARGIN = 2.0 ** -13          # pixels: no float64 source coordinate may be this close to x.5 (the nearest sample's rounding tie)
JOINT_MARGIN = 1e-3              # pixels: no compared joint coordinate may be this close to the threshold it is compared with
COUNT_THRESHOLD = 50
BBOX_SCALE_FACTOR = 1.2
LEGS = (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)
LEGS_ARMS = (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 19, 20, 21, 22)
PART_TO_JOINT = {19: 7, 21: 7, 20: 8, 22: 8, 4: 9, 3: 10, 12: 13, 14: 13, 11: 14, 13: 14, 5: 15, 6: 16}
DP24_TO_14 = [0, 1, 1, 11, 12, 14, 13, 8, 6, 8, 6, 9, 7, 9, 7, 2, 4, 2, 4, 3, 5, 3, 5, 10, 10]
COUNTED_PARTS = (3, 5, 7, 9, 11, 12, 13, 14)                                 # the device's part_counts columns
JOINT_TO_PART = {7: 3, 8: 5, 9: 12, 10: 11, 13: 7, 14: 9, 15: 14, 16: 13}    # utils/joints2d_utils.py:37
OTHER_JOINTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 15, 16]
HIP_JOINTS = [11, 12]


def augment_cfg(kind):
    """'default': the reference's TRAIN.SYNTH_DATA.AUGMENT values.  'raised': every probability well above them, so that a dozen
    images exercise every branch on both sides."""
    from hierarchicalprobabilistic3dhuman_amd import configs
    cfg = configs.get_cfg_defaults().TRAIN.SYNTH_DATA.AUGMENT
    if kind == "default":
        return cfg
    assert kind == "raised"
    p, r = cfg.PROXY_REP, cfg.RGB
    p.REMOVE_PARTS_PROBS = [0.15] * 24
    p.REMOVE_APPENDAGE_JOINTS_PROB, p.REMOVE_JOINTS_PROB, p.JOINTS_SWAP_PROB = 0.5, 0.2, 0.4
    p.OCCLUDE_BOX_PROB, p.OCCLUDE_BOTTOM_PROB, p.OCCLUDE_TOP_PROB, p.OCCLUDE_VERTICAL_PROB = 0.5, 0.3, 0.3, 0.5
    p.EXTREME_CROP_PROB = 0.6
    r.OCCLUDE_BOTTOM_PROB, r.OCCLUDE_TOP_PROB, r.OCCLUDE_VERTICAL_PROB = 0.3, 0.3, 0.5
    return cfg


# name -> B, D (output side), H, W (input), cfg kind, seed (of the inputs and of both generators).  The first four are in the golden
# file; seeds were searched until tests/test_train_frontend_host.py's conditions on the inputs hold (branch coverage, margins).
SEEDS = {'d64_b1': 5, 'd64_b3': 3, 'd64_b6': 20, 'd46_b3': 3, 'd256_b2': 1}
CASES = {
    "d64_b1": SimpleNamespace(B=1, D=64, H=64, W=64, cfg="raised", seed=SEEDS['d64_b1']),
    "d64_b3": SimpleNamespace(B=3, D=64, H=64, W=64, cfg="raised", seed=SEEDS['d64_b3']),
    "d64_b6": SimpleNamespace(B=6, D=64, H=64, W=64, cfg="raised", seed=SEEDS['d64_b6']),
    "d46_b3": SimpleNamespace(B=3, D=46, H=80, W=64, cfg="raised", seed=SEEDS['d46_b3']),
    "d256_b2": SimpleNamespace(B=2, D=256, H=256, W=256, cfg="default", seed=SEEDS['d256_b2']),
}
GOLDEN_CASES = ("d64_b1", "d64_b3", "d64_b6", "d46_b3")
GOLDEN_KEYS = ("seg_crop", "seg_aug", "rgb_in", "joints2D", "joints2D_input", "vis", "counts")


def make_inputs(case, image_seeds=None):
    """iuv (B,3,H,W), rgb (B,3,H,W), background (B,3,D,D), joints2d (B,17,2), all float32 on the CPU.  Image i is generated from
    ``image_seeds[i]`` (default: 1000 * case.seed + i) alone, so that an image can be put into another batch."""
    B, D, H, W = case.B, case.D, case.H, case.W
    seeds = [1000 * case.seed + i for i in range(B)] if image_seeds is None else list(image_seeds)
    iuv, rgb, bg, j2d = (torch.zeros(B, 3, H, W), torch.zeros(B, 3, H, W), torch.zeros(B, 3, D, D), torch.zeros(B, 17, 2))
    rows, cols = torch.arange(H, dtype=torch.float32)[:, None], torch.arange(W, dtype=torch.float32)[None, :]
    for i, s in enumerate(seeds):
        g = torch.Generator().manual_seed(int(s))
        # the figure: 6 x 4 blob centres over the middle of the frame, jittered, radii of 4 to 11 % of the frame
        top, left = (0.18 + 0.1 * torch.rand(2, generator=g)).tolist()
        fh, fw = (0.5 + 0.12 * torch.rand(2, generator=g)).tolist()
        part = torch.zeros(H, W)
        order = torch.randperm(24, generator=g).tolist()
        for n, cls in enumerate(order):
            gr, gc = divmod(n, 4)
            cy = (top + fh * (gr + 0.5) / 6 + 0.02 * float(torch.rand(1, generator=g))) * H
            cx = (left + fw * (gc + 0.5) / 4 + 0.02 * float(torch.rand(1, generator=g))) * W
            ry = (0.04 + 0.07 * float(torch.rand(1, generator=g))) * H
            rx = (0.04 + 0.07 * float(torch.rand(1, generator=g))) * W
            part[((rows - cy) / ry) ** 2 + ((cols - cx) / rx) ** 2 <= 1.0] = cls + 1
        iuv[i, 0] = part
        iuv[i, 1:] = torch.randint(0, 256, (2, H, W), generator=g).float() * (part != 0)
        rgb[i] = torch.rand(3, H, W, generator=g)
        bg[i] = torch.rand(3, D, D, generator=g)
        j2d[i] = (torch.rand(17, 2, generator=g) * 1.4 - 0.2) * torch.tensor([W, H], dtype=torch.float32)
    return dict(iuv=iuv, rgb=rgb, background=bg, joints2d=j2d)


def generators(seed):
    """numpy RandomState and torch CPU generator in the state np.random.seed(seed); torch.manual_seed(seed) leave the global ones."""
    return np.random.RandomState(seed), torch.Generator().manual_seed(seed)


def _visibility(j, img_wh, vis=None):
    """utils/joints2d_utils.py:13-26."""
    if vis is None:
        vis = torch.ones(j.shape[:2], device=j.device, dtype=torch.bool)
    vis[j[:, :, 0] > img_wh] = 0
    vis[j[:, :, 1] > img_wh] = 0
    vis[j[:, :, 0] < 0] = 0
    vis[j[:, :, 1] < 0] = 0
    return vis


def _to14(seg):
    out = torch.zeros_like(seg)
    for c in range(1, 25):
        out[seg == c] = DP24_TO_14[c]
    return out


def _half_occlusions(cfg, wh, rs, B, zero_rows, zero_cols, joints, vis, tag, log):
    """random_occlude_bottom_half / _top_half / _vertical_half of either augmentation module (they differ only in the image they
    write to): ``zero_rows(i, slice)`` / ``zero_cols(i, slice)`` do the writing."""
    rv = rs.rand(B)
    for i in range(B):
        hit = rv[i] < cfg.OCCLUDE_BOTTOM_PROB
        log[tag + "_bottom"].append(bool(hit))
        if hit:
            occlude_from = int(wh / 2.0) + rs.randint(low=-int(wh / 5.), high=int(wh / 5.))
            zero_rows(i, slice(occlude_from, None))
            log["joint_tests"].append((joints[i, :, 1], occlude_from))
            vis[i, joints[i, :, 1] > occlude_from] = False
    rv = rs.rand(B)
    for i in range(B):
        hit = rv[i] < cfg.OCCLUDE_TOP_PROB
        log[tag + "_top"].append(bool(hit))
        if hit:
            occlude_up_to = int(wh / 2.0) + rs.randint(low=-int(wh / 5.), high=int(wh / 5.))
            zero_rows(i, slice(None, occlude_up_to))
            log["joint_tests"].append((joints[i, :, 1], occlude_up_to))
            vis[i, joints[i, :, 1] < occlude_up_to] = False
    rv = rs.rand(B)
    for i in range(B):
        hit = rv[i] < cfg.OCCLUDE_VERTICAL_PROB
        left = False
        if hit:
            occlude_up_to = int(wh / 2.0) + rs.randint(low=-int(wh / 30.), high=int(wh / 30.))
            log["joint_tests"].append((joints[i, :, 0], occlude_up_to))
            if rs.rand() > 0.5:
                left = True
                zero_cols(i, slice(None, occlude_up_to))
                vis[i, joints[i, :, 0] < occlude_up_to] = False
            else:
                zero_cols(i, slice(occlude_up_to, None))
                vis[i, joints[i, :, 0] > occlude_up_to] = False
        log[tag + "_vertical_left"].append(bool(hit and left))
        log[tag + "_vertical_right"].append(bool(hit and not left))


def restate(inputs, cfg, D, np_random, generator, dtype=torch.float32, device="cpu", record=True):
    """The training step's lines :199-244 on ``inputs`` (make_inputs) -> dict of seg_crop, seg_aug (B,D,D), rgb_in (B,3,D,D), joints2D,
    joints2D_input (B,17,2), vis (B,17) bool, counts (B,8) int64, plus what the host tests ask of the inputs: ``source_xy`` (the
    source coordinates of the output columns and rows, (B,D) each), ``joint_tests`` ((coordinates, threshold) of every comparison made)
    and ``branches`` (name -> bools per image -- ``record=False`` leaves out those that would read device results back, for timing; per (image, joint) or (image, part) for the three checks of the joints)."""
    from collections import defaultdict
    rs, log = np_random, defaultdict(list)
    iuv, rgb, background, joints2d = (inputs[k].to(device=device, dtype=dtype) for k in ("iuv", "rgb", "background", "joints2d"))
    B, _, H, W = iuv.shape
    T = lambda x: x.to(device=device, dtype=dtype)                    # a float32 draw, as the reference draws it, in the working dtype
    pr, rg, bb = cfg.PROXY_REP, cfg.RGB, cfg.BBOX
    img_wh = D

    # ---- :181-183 visibility before the crop
    log["joint_tests"] += [(joints2d.reshape(-1), 0), (joints2d.reshape(-1), img_wh)]
    vis = _visibility(joints2d, img_wh)
    if record:
        log["pre_crop_out_of_frame"] = (~vis).flatten().tolist()                # per (image, joint)
    vis_pre = vis.clone()

    # ---- :199-200 random_extreme_crop
    seg = iuv[:, 0]
    rv = torch.rand(B, generator=generator)
    p = pr.EXTREME_CROP_PROB
    legs, legs_arms = rv < p * 0.5, torch.logical_and(rv > p * 0.5, rv < p)
    log["extreme_crop_legs"], log["extreme_crop_legs_arms"] = legs.tolist(), legs_arms.tolist()
    determiner = seg.clone()
    for chosen, classes in ((legs, LEGS), (legs_arms, LEGS_ARMS)):
        sub = determiner[chosen.to(device)]
        sub[(sub[..., None] == torch.tensor(classes, device=device, dtype=dtype)).any(-1)] = 0
        determiner[chosen.to(device)] = sub

    # ---- :203-217 batch_crop_pytorch_affine with a bbox_determiner
    input_wh = torch.tensor((W, H), device=device, dtype=dtype)
    output_wh = torch.tensor((D, D), device=device, dtype=dtype)
    corners = torch.zeros(B, 4, dtype=dtype, device=device)
    for i in range(B):
        body = torch.nonzero(determiner[i] != 0, as_tuple=False)
        corners[i, :2], _ = torch.min(body, dim=0)
        corners[i, 2:], _ = torch.max(body, dim=0)
    centres = torch.zeros(B, 2, dtype=dtype, device=device)
    centres[:, 0] = (corners[:, 0] + corners[:, 2]) / 2.0
    centres[:, 1] = (corners[:, 1] + corners[:, 3]) / 2.0
    heights, widths = corners[:, 2] - corners[:, 0], corners[:, 3] - corners[:, 1]
    aspect = (output_wh[1] / output_wh[0]).item()
    widths[heights > widths * aspect] = heights[heights > widths * aspect] / aspect
    heights[heights < widths * aspect] = widths[heights < widths * aspect] * aspect
    l, h = bb.DELTA_SCALE_RANGE
    scale = BBOX_SCALE_FACTOR + T((h - l) * torch.rand(B, generator=generator, dtype=torch.float32) + l)
    heights, widths = heights * scale, widths * scale
    l, h = bb.DELTA_CENTRE_RANGE
    centres = centres + T((h - l) * torch.rand(B, 2, generator=generator, dtype=torch.float32) + l)
    output_centre = output_wh * 0.5
    affine = torch.zeros(B, 2, 3, dtype=dtype, device=device)
    affine[:, 0, 0] = output_wh[0] / widths
    affine[:, 1, 1] = output_wh[1] / heights
    whs = torch.stack([widths, heights], dim=-1)
    affine[:, :, 2] = output_centre - (output_wh / whs) * centres[:, [1, 0]]
    theta = torch.zeros(B, 2, 3, dtype=dtype, device=device)
    theta[:, 0, 0] = widths / input_wh[0]
    theta[:, 1, 1] = heights / input_wh[1]
    theta[:, :, 2] = -affine[:, :, 2] / (output_wh / whs)
    theta[:, :, 2] = theta[:, :, 2] / (input_wh * 0.5) + (whs / input_wh) - 1
    grid = F.affine_grid(theta=theta, size=[B, 1, D, D], align_corners=False)
    seg_crop = (F.grid_sample(iuv[:, :1] + 1, grid, mode="nearest", padding_mode="zeros", align_corners=False) - 1)[:, 0]
    homo = torch.cat([joints2d, torch.ones(B, 17, 1, device=device, dtype=dtype)], dim=-1)
    joints = torch.einsum("bij,bkj->bki", affine, homo)
    rgb_crop = F.grid_sample(rgb, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    source_xy = (((grid[:, 0, :, 0] + 1) * W - 1) / 2, ((grid[:, :, 0, 1] + 1) * H - 1) / 2)

    # ---- :220-227 visibility after the crop, body-part occlusion
    log["joint_tests"] += [(joints.reshape(-1), 0), (joints.reshape(-1), img_wh)]
    vis = _visibility(joints, img_wh, vis)
    if record:
        log["post_crop_out_of_frame"] = (vis_pre & ~vis).flatten().tolist()
    seg14 = _to14(seg_crop)
    counts = torch.stack([(seg14 == part).sum(dim=(1, 2)) for part in COUNTED_PARTS], dim=1)
    new_vis = vis.clone()
    for joint, part in JOINT_TO_PART.items():
        new_vis[:, joint] = vis[:, joint] & ((seg14 == part).sum(dim=(1, 2)) > COUNT_THRESHOLD)
    vis = new_vis
    if record:
        log["part_count_below"] = (counts <= COUNT_THRESHOLD).flatten().tolist()     # per (image, counted part)
    vis_occlusion = vis.clone()

    # ---- :230-234 augment_proxy_representation
    seg_aug, j_in, vis = seg_crop.clone(), joints.clone(), vis.clone()
    with_joint, without_joint = [False] * B, [False] * B
    for cls, prob in zip(pr.REMOVE_PARTS_CLASSES, pr.REMOVE_PARTS_PROBS):
        rvec = rs.rand(B) < prob
        sub = seg_aug[rvec].clone()
        sub[sub == cls] = 0
        seg_aug[rvec] = sub
        if cls in PART_TO_JOINT:
            rvj = np.logical_and(rvec, rs.rand(B) < pr.REMOVE_APPENDAGE_JOINTS_PROB)
            vis[rvj, PART_TO_JOINT[cls]] = 0
            for i in range(B):
                with_joint[i] |= bool(rvj[i])
                without_joint[i] |= bool(rvec[i] and not rvj[i])
    log["part_removed_with_joint"], log["part_removed_without_joint"] = with_joint, without_joint
    wh = seg_aug.shape[-1]
    centre, dim = wh / 2, pr.OCCLUDE_BOX_DIM
    x_h, x_l = centre - 0.3 * wh / 2, centre + 0.3 * wh / 2
    y_h, y_l = centre - 0.3 * wh / 2, centre + 0.3 * wh / 2
    x = (x_h - x_l) * rs.rand(B) + x_l
    y = (y_h - y_l) * rs.rand(B) + y_l
    x1, x2 = (x - dim / 2).astype(np.int16), (x + dim / 2).astype(np.int16)
    y1, y2 = (y - dim / 2).astype(np.int16), (y + dim / 2).astype(np.int16)
    rvec = rs.rand(B)
    for i in range(B):
        hit = rvec[i] < pr.OCCLUDE_BOX_PROB
        log["box"].append(bool(hit))
        log["box_negative_start"].append(bool(hit and (x1[i] < 0 or y1[i] < 0)))
        if hit:
            seg_aug[i, x1[i]:x2[i], y1[i]:y2[i]] = 0
    swapped = [False] * B
    for pair in pr.JOINTS_TO_SWAP:
        rvec = rs.rand(B) < pr.JOINTS_SWAP_PROB
        sub, tmp = j_in[rvec].clone(), j_in[rvec].clone()
        sub[:, pair[0], :] = tmp[:, pair[1], :]
        sub[:, pair[1], :] = tmp[:, pair[0], :]
        j_in[rvec] = sub
        swapped = [a or bool(b) for a, b in zip(swapped, rvec)]
    log["swap"] = swapped
    l, h = pr.DELTA_J2D_DEV_RANGE
    j_in[:, OTHER_JOINTS, :] = j_in[:, OTHER_JOINTS, :] + T((h - l) * torch.rand(B, 15, 2, generator=generator, dtype=torch.float32) + l)
    j_in[:, HIP_JOINTS, :] = j_in[:, HIP_JOINTS, :] + T((h - l) * torch.rand(B, 2, 2, generator=generator, dtype=torch.float32) + l)
    removed = [False] * B
    for joint in pr.REMOVE_JOINTS_INDICES:
        rvec = rs.rand(B) < pr.REMOVE_JOINTS_PROB
        vis[rvec, joint] = 0
        removed = [a or bool(b) for a, b in zip(removed, rvec)]
    log["joint_removed"] = removed

    def seg_rows(i, s):
        seg_aug[i, s, :] = 0

    def seg_cols(i, s):
        seg_aug[i, :, s] = 0

    _half_occlusions(pr, wh, rs, B, seg_rows, seg_cols, j_in, vis, "seg", log)

    # ---- :237-239 batch_add_rgb_background
    is_bg = seg_aug[:, None, :, :] == 0
    rgb_bg = rgb_crop * torch.logical_not(is_bg) + background * is_bg

    # ---- :241-244 augment_rgb
    rgb_in = rgb_bg.clone()

    def rgb_rows(i, s):
        rgb_in[i, :, s, :] = 0

    def rgb_cols(i, s):
        rgb_in[i, :, :, s] = 0

    _half_occlusions(rg, rgb_in.shape[-1], rs, B, rgb_rows, rgb_cols, j_in, vis, "rgb", log)
    l, h = 1 - rg.PIXEL_CHANNEL_NOISE, 1 + rg.PIXEL_CHANNEL_NOISE
    noise = T((h - l) * torch.rand(B, 3, generator=generator, dtype=torch.float32) + l)
    rgb_in = torch.clamp(rgb_in * noise[:, :, None, None], max=1.0)

    joint_tests = log.pop("joint_tests")
    return dict(seg_crop=seg_crop, seg_aug=seg_aug, rgb_in=rgb_in, joints2D=joints, joints2D_input=j_in, vis=vis, counts=counts,
                rgb_crop=rgb_crop, rgb_bg=rgb_bg, background=background, vis_occlusion=vis_occlusion, determiner=determiner, affine=affine,
                source_xy=source_xy, joint_tests=joint_tests, branches=dict(log))


BRANCHES = ("extreme_crop_legs", "extreme_crop_legs_arms", "part_removed_with_joint", "part_removed_without_joint", "box", "swap",
            "joint_removed", "seg_bottom", "seg_top", "seg_vertical_left", "seg_vertical_right", "rgb_bottom", "rgb_top",
            "rgb_vertical_left", "rgb_vertical_right", "pre_crop_out_of_frame", "post_crop_out_of_frame", "part_count_below",
            "box_negative_start")


def tie_distance(ref64):
    """Smallest distance, in pixels, of a float64 source coordinate to a rounding tie of the nearest sample."""
    return min(float(((c - torch.floor(c)) - 0.5).abs().min()) for c in ref64["source_xy"])


def joint_distance(ref64):
    """Smallest distance, in pixels, of a compared float64 joint coordinate to the threshold it is compared with."""
    return min(float((c - t).abs().min()) for c, t in ref64["joint_tests"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, float32 restatement, float64 restatement) of a case, computed once and shared: callers must not modify them."""
    case = CASES[name]
    inputs = make_inputs(case)
    return inputs, restate(inputs, augment_cfg(case.cfg), case.D, *generators(case.seed)), restate(
        inputs, augment_cfg(case.cfg), case.D, *generators(case.seed), dtype=torch.float64)


def plan(name):
    """draw_augment_plan under the case's seeds."""
    from hierarchicalprobabilistic3dhuman_amd import train_augmentation as ta
    case = CASES[name]
    return ta.draw_augment_plan(augment_cfg(case.cfg), case.B, case.D, *generators(case.seed))


def bound(name, key):
    _, r32, r64 = reference(name)
    return 4.0 * max(float((r32[key].double() - r64[key]).abs().max()), EPS32 * float(r64[key].abs().max()))


def apply_plan(plan, ref):
    """What a plan's record means (include/hps.h), applied on the host to the restatement's cropped plane, cropped RGB, background-free
    joints and post-occlusion visibility -> (seg_aug, rgb_in, joints2D_input, vis) in the restatement's dtype."""
    from hierarchicalprobabilistic3dhuman_amd import train_augmentation as ta
    w, f = plan.words, plan.floats
    seg, rgb, joints, vis = ref["seg_crop"].clone(), ref["rgb_crop"].clone(), ref["joints2D"], ref["vis_occlusion"].clone()
    B, D = seg.shape[0], seg.shape[-1]
    j_in = torch.zeros_like(joints)
    for i in range(B):
        for c in range(1, 25):
            if (int(w[i, ta._SEG_MASK]) >> c) & 1:
                seg[i][seg[i] == c] = 0
        r0, r1, c0, c1 = w[i, ta._BOX:ta._BOX + 4]
        seg[i, r0:r1, c0:c1] = 0
        o = w[i, ta._SEG_OCC:ta._SEG_OCC + 6]
        seg[i, o[0]:o[1], :] = 0
        seg[i, o[2]:o[3], :] = 0
        seg[i, :, o[4]:o[5]] = 0
        j_in[i] = joints[i, w[i, ta._SWAP:ta._SWAP + 17].tolist()] + torch.from_numpy(f[i, ta._DEV:ta._DEV + 34].reshape(17, 2)).to(joints.dtype)
        for k in range(17):
            if (int(w[i, ta._INVIS]) >> k) & 1:
                vis[i, k] = False
        for base in (ta._SEG_JT, ta._RGB_JT):
            t = f[i, base:base + 4].astype(np.float64)
            u, v = j_in[i, :, 0], j_in[i, :, 1]
            vis[i, (v > t[0]) | (v < t[1]) | (u < t[2]) | (u > t[3])] = False
    is_bg = seg[:, None] == 0
    rgb = torch.where(is_bg, ref["background"], rgb)
    for i in range(B):
        o = w[i, ta._RGB_OCC:ta._RGB_OCC + 6]
        rgb[i, :, o[0]:o[1], :] = 0
        rgb[i, :, o[2]:o[3], :] = 0
        rgb[i, :, :, o[4]:o[5]] = 0
    chan = torch.from_numpy(f[:, ta._CHAN:ta._CHAN + 3].copy()).to(rgb.dtype)
    rgb = torch.clamp(rgb * chan[:, :, None, None], max=1.0)
    return seg, rgb, j_in, vis
