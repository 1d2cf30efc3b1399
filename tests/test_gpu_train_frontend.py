"""GPU: the synthetic-data training front end (csrc/train_frontend.hip through train_augmentation.SyntheticTrainFrontEnd and the
reference-named wrappers) against the reference's own outputs (tests/golden/train_frontend_vectors.npz) and the float64 restatement
of tests/train_frontend_scenario.py.

Cropped and augmented part planes, part counts and visibility are decisions: they EQUAL the reference everywhere (the host tests show
that no source coordinate is near a rounding tie and no joint near a threshold, so nothing is excluded).  rgb_in, both joint sets and
the heat-map channels hold the standing rule  |device - float64| <= 4 max(|float32 restatement - float64|, 2^-23 max|float64|).  The
edge channel is pinned to the Canny kernel run on the front end's own rgb_in: the threshold is a discontinuity and that kernel has
tests of its own.

Cases: D = 64 with B = 1, 3, 6; D = 46 with B = 3 from an 80 x 64 input (scalar tail, unaligned rows, non-square source); D = 256,
B = 2 at the default configuration.  Every case runs once (module cache) and is shared by the tests.
"""
import functools
import os

import numpy as np
import pytest
import torch

import train_frontend_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, image_utils, joints2d_utils, label_conversions, train_augmentation as ta
from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEATMAP_STD = 4.0
NAMES = list(S.CASES)


@functools.lru_cache(maxsize=None)
def vectors():
    z = np.load(os.path.join(ROOT, "tests", "golden", "train_frontend_vectors.npz"))
    return {k: z[k] for k in z.files}


def make_front_end(case):
    data = configs.get_cfg_defaults().DATA
    edge = CannyEdgeDetector(non_max_suppression=data.EDGE_NMS, gaussian_filter_std=data.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=data.EDGE_GAUSSIAN_SIZE, threshold=data.EDGE_THRESHOLD).to("cuda")
    return ta.SyntheticTrainFrontEnd(S.augment_cfg(case.cfg), case.D, edge, HEATMAP_STD, data.EDGE_NMS,
                                     bbox_scale_factor=S.BBOX_SCALE_FACTOR, pixel_count_threshold=S.COUNT_THRESHOLD)


def on_device(inputs):
    return {k: v.cuda() for k, v in inputs.items()}


def run(fe, inputs, plan):
    d = on_device(inputs)
    out = fe(d["iuv"], d["rgb"], d["background"], d["joints2d"], plan=plan, return_seg_aug=True, return_seg_crop=True)
    got = {k: v.clone() for k, v in out.items()}
    got["counts"] = fe.part_counts().clone()
    fe.check()
    return got


@functools.lru_cache(maxsize=None)
def device_run(name):
    """The fused front end on a case, once: (front end, outputs on the device)."""
    case = S.CASES[name]
    fe = make_front_end(case)
    return fe, run(fe, S.reference(name)[0], S.plan(name))


def expected(name, key):
    """The reference's own output where the golden file has the case, else the float32 restatement's (decisions only)."""
    if name in S.GOLDEN_CASES:
        return torch.from_numpy(vectors()["%s_%s" % (name, key)].astype(np.float64))
    return S.reference(name)[1][key].double()


@pytest.mark.parametrize("name", NAMES)
def test_planes_counts_and_visibility_equal_the_reference(dev, name):
    got = device_run(name)[1]
    for key, mine in (("seg_crop", "seg_crop"), ("seg_aug", "seg_aug"), ("counts", "counts"), ("vis", "joints2D_vis")):
        want, have = expected(name, key), got[mine].cpu().double()
        differ = int((want != have).sum())
        print("%s %s: %d of %d entries differ" % (name, key, differ, want.numel()))
        assert want.shape == have.shape and differ == 0, (name, key)


@pytest.mark.parametrize("name", NAMES)
def test_rgb_and_joints_hold_the_rule(dev, name):
    got = device_run(name)[1]
    r64 = S.reference(name)[2]
    for key in ("rgb_in", "joints2D", "joints2D_input"):
        err, bound = float((got[key].cpu().double() - r64[key]).abs().max()), S.bound(name, key)
        print("%s %s: max error %.3e, bound %.3e (ratio %.3f)" % (name, key, err, bound, err / bound))
        assert err <= bound, (name, key)


def heatmaps(joints, vis, D):
    """utils/label_conversions.py:105-124 times the visibility (train_poseMF_shapeGaussian_net.py:250-253), in the joints' dtype."""
    xx = torch.arange(D, dtype=joints.dtype)[None, None, None, :]
    yy = torch.arange(D, dtype=joints.dtype)[None, None, :, None]
    u, v = joints[:, :, 0, None, None], joints[:, :, 1, None, None]
    return torch.exp(-(((xx - u) / HEATMAP_STD) ** 2) / 2 - (((yy - v) / HEATMAP_STD) ** 2) / 2) * vis[:, :, None, None].to(joints.dtype)


@pytest.mark.parametrize("name", NAMES)
def test_proxy_representation(dev, name):
    fe, got = device_run(name)
    case = S.CASES[name]
    proxy = got["proxy_rep_input"]
    assert proxy.shape == (case.B, 18, case.D, case.D)
    # bit for bit the Canny and heat-map kernels on the front end's own rgb_in, joints and visibility
    again = torch.empty_like(proxy)
    fe.edge_detector.edge_map_into(got["rgb_in"], again, nms=fe.edge_nms)
    label_conversions.make_proxy_representation(None, got["joints2D_input"], got["joints2D_vis"].float(), case.D, HEATMAP_STD, out=again)
    assert torch.equal(proxy, again)
    # the heat-map channels against the restatement
    _, r32, r64 = S.reference(name)
    h64 = heatmaps(r64["joints2D_input"], r64["vis"], case.D)
    e32 = float((heatmaps(r32["joints2D_input"], r32["vis"], case.D).double() - h64).abs().max())
    bound = 4.0 * max(e32, S.EPS32 * float(h64.abs().max()))
    err = float((proxy[:, 1:].cpu().double() - h64).abs().max())
    print("%s heat-maps: max error %.3e, bound %.3e (ratio %.3f)" % (name, err, bound, err / bound))
    assert err <= bound


@pytest.mark.parametrize("name", ["d64_b6", "d46_b3"])
def test_each_wrapper_alone_agrees_with_the_fused_path_bit_for_bit(dev, name):
    """The training script's own sequence of calls (train/train_poseMF_shapeGaussian_net.py:181-244), one wrapper per line, on the same
    plan."""
    case, plan = S.CASES[name], S.plan(name)
    fused = device_run(name)[1]
    d = on_device(S.reference(name)[0])
    cfg = S.augment_cfg(case.cfg)
    vis = joints2d_utils.check_joints2d_visibility_torch(d["joints2d"], case.D)
    determiner = ta.random_extreme_crop(d["iuv"][:, 0].contiguous(), cfg.PROXY_REP.EXTREME_CROP_PROB, plan=plan)
    crop = ta.batch_crop_pytorch_affine_train((case.W, case.H), (case.D, case.D), case.B, "cuda", iuv=d["iuv"], joints2D=d["joints2d"],
                                              rgb=d["rgb"], bbox_determiner=determiner, orig_scale_factor=S.BBOX_SCALE_FACTOR, plan=plan)
    assert int(crop["status"].sum()) == 0
    seg = crop["iuv"][:, 0].contiguous()
    assert torch.equal(seg, fused["seg_crop"]) and torch.equal(crop["joints2D"], fused["joints2D"])
    vis = joints2d_utils.check_joints2d_visibility_torch(crop["joints2D"], case.D, visibility=vis)
    seg14 = label_conversions.convert_densepose_seg_to_14part_labels(seg)
    assert torch.equal(seg14.cpu(), S._to14(fused["seg_crop"].cpu()))
    vis = joints2d_utils.check_joints2d_occluded_torch(seg14, vis, pixel_count_threshold=S.COUNT_THRESHOLD)
    assert torch.equal(vis.cpu(), S.reference(name)[1]["vis_occlusion"])
    seg_aug, j_in, vis = ta.augment_proxy_representation(seg, crop["joints2D"], vis, cfg.PROXY_REP, plan=plan)
    assert torch.equal(seg_aug, fused["seg_aug"])
    rgb = image_utils.batch_add_rgb_background(d["background"], crop["rgb"], seg_aug)
    rgb, j_in, vis = ta.augment_rgb(rgb, j_in, vis, cfg.RGB, plan=plan)
    assert torch.equal(rgb, fused["rgb_in"])
    assert torch.equal(j_in, fused["joints2D_input"])
    assert torch.equal(vis, fused["joints2D_vis"])


def test_wrappers_draw_their_own_plan_in_the_reference_order(dev):
    """Without ``plan=`` a wrapper draws what its reference function draws: the three of them, called in the training script's order
    under the case's seeds, end where the fused path's plan ends."""
    name = "d64_b3"
    case, fused = S.CASES[name], device_run(name)[1]
    cfg = S.augment_cfg(case.cfg)
    d = on_device(S.reference(name)[0])
    rs, gen = S.generators(case.seed)
    determiner = ta.random_extreme_crop(d["iuv"][:, 0].contiguous(), cfg.PROXY_REP.EXTREME_CROP_PROB, generator=gen)
    crop = ta.batch_crop_pytorch_affine_train((case.W, case.H), (case.D, case.D), case.B, "cuda", iuv=d["iuv"], joints2D=d["joints2d"],
                                              rgb=d["rgb"], bbox_determiner=determiner, orig_scale_factor=S.BBOX_SCALE_FACTOR,
                                              delta_scale_range=cfg.BBOX.DELTA_SCALE_RANGE, delta_centre_range=cfg.BBOX.DELTA_CENTRE_RANGE,
                                              generator=gen)
    seg = crop["iuv"][:, 0].contiguous()
    assert torch.equal(seg, fused["seg_crop"])
    vis = torch.from_numpy(np.ascontiguousarray(S.reference(name)[1]["vis_occlusion"].numpy())).cuda()
    seg_aug, j_in, vis = ta.augment_proxy_representation(seg, crop["joints2D"], vis, cfg.PROXY_REP, np_random=rs, generator=gen)
    rgb = image_utils.batch_add_rgb_background(d["background"], crop["rgb"], seg_aug)
    rgb, j_in, vis = ta.augment_rgb(rgb, j_in, vis, cfg.RGB, np_random=rs, generator=gen)
    assert torch.equal(seg_aug, fused["seg_aug"]) and torch.equal(rgb, fused["rgb_in"])
    assert torch.equal(j_in, fused["joints2D_input"]) and torch.equal(vis, fused["joints2D_vis"])


def test_empty_mask_sets_the_status_word_and_check_raises(dev):
    name = "d64_b3"
    case = S.CASES[name]
    inputs = {k: v.clone() for k, v in S.reference(name)[0].items()}
    inputs["iuv"][1] = 0.0                                            # image 1: no body pixel at all
    fe = make_front_end(case)
    d = on_device(inputs)
    out = fe(d["iuv"], d["rgb"], d["background"], d["joints2d"], plan=S.plan(name), return_seg_crop=True)
    assert fe.status().tolist() == [0, 1, 0]
    with pytest.raises(_capi.HpsError, match=r"image\(s\) \[1\]"):
        fe.check()
    # its box is the whole frame: background inside it, -1 outside
    assert float(out["seg_crop"][1].max()) == 0.0 and float(out["seg_crop"][1].min()) >= -1.0
    good = device_run(name)[1]
    for i in (0, 2):                                                  # the other images are untouched
        assert torch.equal(out["rgb_in"][i], good["rgb_in"][i]) and torch.equal(out["joints2D_vis"][i], good["joints2D_vis"][i])


@pytest.mark.parametrize("name", ["d64_b6", "d46_b3"])
def test_two_runs_give_equal_bits(dev, name):
    fe, first = device_run(name)
    second = run(fe, S.reference(name)[0], S.plan(name))
    for key in first:
        assert torch.equal(first[key], second[key]), key
    other = run(make_front_end(S.CASES[name]), S.reference(name)[0], S.plan(name))        # and from freshly allocated buffers
    for key in first:
        assert torch.equal(first[key], other[key]), key


def test_an_image_gives_the_same_bits_alone_and_inside_a_batch(dev):
    name, i = "d64_b6", 3
    case6, plan6 = S.CASES[name], S.plan(name)
    case1 = S.CASES["d64_b1"]
    inputs1 = S.make_inputs(case1, image_seeds=[1000 * case6.seed + i])
    for k, v in S.reference(name)[0].items():
        assert torch.equal(inputs1[k][0], v[i])
    plan1 = ta.AugmentPlan(1, case6.D)
    plan1.words[0] = plan6.words[i]
    alone = run(make_front_end(case1), inputs1, plan1)
    batch = device_run(name)[1]
    for key in batch:
        assert torch.equal(alone[key][0], batch[key][i]), key


def test_cpu_tensors_are_refused(dev):
    name = "d64_b1"
    case = S.CASES[name]
    fe, inputs = make_front_end(case), S.reference(name)[0]
    d = on_device(inputs)
    for key in ("iuv", "rgb", "background", "joints2d"):
        args = dict(d, **{key: inputs[key]})
        with pytest.raises(_capi.HpsError):
            fe(args["iuv"], args["rgb"], args["background"], args["joints2d"], plan=S.plan(name))
    with pytest.raises(_capi.HpsError):
        ta.random_extreme_crop(inputs["iuv"][:, 0].contiguous())
    with pytest.raises(_capi.HpsError):
        image_utils.batch_add_rgb_background(inputs["background"], d["rgb"], d["iuv"][:, 0].contiguous())
    with pytest.raises(_capi.HpsError):
        joints2d_utils.check_joints2d_visibility_torch(inputs["joints2d"], case.D)


def test_perspective_projection(dev):
    """utils/cam_utils.py:30-61 against its definition in float64."""
    from hierarchicalprobabilistic3dhuman_amd import cam_utils
    g = torch.Generator().manual_seed(3)
    pts = torch.randn(4, 17, 3, generator=g) * 0.4
    t = torch.tensor(configs.get_cfg_defaults().TRAIN.SYNTH_DATA.MEAN_CAM_T)[None].repeat(4, 1) + 0.05 * torch.randn(4, 3, generator=g)
    got = cam_utils.perspective_project_torch(pts.cuda(), None, t.cuda(), focal_length=300.0, img_wh=256)
    p = pts.double() + t.double()[:, None]
    want = 300.0 * p[:, :, :2] / p[:, :, 2:] + 128.0
    assert got.shape == (4, 17, 2)
    # five roundings (translate, divide, times f, times 1 for the centre, add), each at most half an ulp of a value no larger than the
    # result's maximum: 2.5 * 2^-23 max|.|; 8 leaves room for the sum order of the intrinsics product
    assert float((got.cpu().double() - want).abs().max()) <= 8 * S.EPS32 * float(want.abs().max())
