"""hps_silhouette_iou (csrc/render.hip through TexturedIUVRenderer.silhouette_counts) against the float64 restatement
(tests/silhouette_scenario.py), the tracker's two input forms on the device, and the evaluation harness with the four SSP-3D
metrics.

The device's condition is exact equality: on every case the float32 restatement's mask equals the float64 one in every pixel
(tests/test_silhouette_host.py).  Should the device differ in a pixel all the same, that pixel must be one of the near-ties
tests/test_gpu_render.py allows (the device's face differs from the float64 one there, within the same cap and the same two bounds), and
the count is printed; 0 is expected.  Whatever the yardstick says, the mask must be the one the device's own hps_render image gives,
bit for bit, and the counts must be numpy's counts of that mask.

Shapes: the five 8 x 8 closed-form scenes and the whole-image triangle; 13 faces in one chunk; 2400 faces on 16 x 16 pixels (record
lists that overflow in every tile); a 36-pixel image (partial tiles) with a mesh partly off the screen; a 40-pixel batch whose last image
is wholly off the screen (every tile takes the empty path and still counts its target pixels; IOU 0 / 0); the orthographic 64-pixel
batch with a scale per image, which also serves the group, flip and repeatability tests."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render_scenario as S
import silhouette_scenario as Q
from hierarchicalprobabilistic3dhuman_amd import _capi, cam_utils, configs, smpl_data, textured_renderer as tr
from hierarchicalprobabilistic3dhuman_amd.eval_metrics_tracker import EvalMetricsTracker
from hierarchicalprobabilistic3dhuman_amd.label_conversions import ALL_JOINTS_TO_COCO_MAP
from test_gpu_evaluate import _SyntheticEvalDataset
from test_gpu_render import device, make_renderer

pytestmark = pytest.mark.gpu
ORTHO = "w64_f2400_b3_ortho"


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def camera(scene):
    kw = dict(cam_t=cuda(scene.cam_t))
    if scene.projection == "orthographic" and scene.scale.shape[0] > 1:
        kw["orthographic_scale"] = cuda(scene.scale)
    return kw


@functools.lru_cache(maxsize=None)
def counted(name):
    """(counts (B,4), masks (B,W,W)) of a case against its rolled target, as numpy arrays, from one call."""
    scene, _, _, target, _ = Q.reference(name)
    counts, masks = device(name)[0].silhouette_counts(cuda(scene.vertices), cuda(target), return_silhouettes=True, **camera(scene))
    assert counts.dtype == torch.int32 and masks.dtype == torch.uint8 and counts.is_cuda and masks.is_cuda
    return counts.cpu().numpy(), masks.cpu().numpy()


@pytest.mark.parametrize("name", Q.CASES)
def test_counts_and_masks_match_the_float64_yardstick(name):
    scene, _, m64, target, want = Q.reference(name)
    _, r32, r64 = S.reference(name)
    rendered = device(name)[2]
    counts, masks = counted(name)
    assert masks.shape == (scene.B, scene.W, scene.W) and set(np.unique(masks).tolist()) <= {0, 1}
    # the mask hps_render's own image gives, bit for bit; numpy's counts of it; every pixel counted once
    assert np.array_equal(masks != 0, Q.mask_of(rendered["iuv"]))
    assert np.array_equal(counts, Q.counts_of(masks, target))
    assert (counts.sum(axis=1) == scene.W * scene.W).all()
    differing = int(((masks != 0) != m64).sum())
    print("%-28s set %6d differing from float64 %d" % (name, int(m64.sum()), differing))
    if differing:                                                                     # the near-tie rule of tests/test_gpu_render.py
        dev = S.deviations(scene, r32, r64)
        agree, n, covered, w_min, excess = S.agreement(scene, rendered, r64)
        assert not (agree & ((masks != 0) != m64)).any()
        assert n <= S.NEAR_TIE_CAP * covered and w_min > -S.FACTOR * dev["bary"] and excess < S.FACTOR * dev["zbuf"]
    else:
        assert np.array_equal(counts, want)
    if name in Q.CLOSED_FORM_TOTALS:                                                  # exact arithmetic: no near-tie to allow
        assert differing == 0 and int(masks.sum()) == Q.CLOSED_FORM_TOTALS[name]


def test_a_wholly_empty_image_still_counts_its_target_pixels():
    counts, masks = counted("w40_f257_b3")
    target = Q.reference("w40_f257_b3")[3]
    assert not masks[2].any() and counts[2].tolist() == [0, 0, 1600 - int(target[2].sum()), int(target[2].sum())] == [0, 0, 1600, 0]
    # ... and with a target that has foreground there: all of it false negatives
    scene = Q.reference("w40_f257_b3")[0]
    ones = np.zeros_like(target)
    ones[:, 3:30, 5:39] = 1
    got = device("w40_f257_b3")[0].silhouette_counts(cuda(scene.vertices), cuda(ones), **camera(scene)).cpu().numpy()
    assert got[2].tolist() == [0, 0, 1600 - 27 * 34, 27 * 34]


def test_targets_all_zero_all_ones_and_none():
    name = "w36_f257_b2"
    scene, _, m64, _, _ = Q.reference(name)
    renderer, masks = device(name)[0], counted(name)[1]
    n_set = masks.reshape(scene.B, -1).sum(axis=1).astype(np.int64)
    rest = scene.W * scene.W - n_set
    zero = np.zeros(scene.B, dtype=np.int64)
    v = cuda(scene.vertices)
    for target, want in ((torch.zeros(scene.B, 36, 36, dtype=torch.uint8, device="cuda"), [zero, n_set, rest, zero]),
                         (None, [zero, n_set, rest, zero]),
                         (torch.ones(scene.B, 36, 36, dtype=torch.bool, device="cuda"), [n_set, zero, zero, rest]),
                         (torch.full((scene.B, 36, 36), 255, dtype=torch.uint8, device="cuda"), [n_set, zero, zero, rest])):
        got = renderer.silhouette_counts(v, target, **camera(scene)).cpu().numpy()
        assert np.array_equal(got, np.stack(want, axis=1))
    with pytest.raises(_capi.HpsError):
        renderer.silhouette_counts(v.cpu(), None, **camera(scene))
    with pytest.raises(_capi.HpsError):
        renderer.silhouette_counts(v, torch.zeros(scene.B, 36, 36, dtype=torch.uint8), **camera(scene))
    with pytest.raises(_capi.HpsError):
        renderer.silhouette_counts(v, torch.zeros(scene.B, 36, 36, device="cuda"), **camera(scene))       # float targets


def test_a_group_of_meshes_shares_its_target_and_camera():
    scene, _, m64, target, want = Q.reference(ORTHO)
    renderer = device(ORTHO)[0]
    v = cuda(scene.vertices).repeat_interleave(2, dim=0)                              # M = 6: meshes 2 g and 2 g + 1 are image g
    counts, masks = renderer.silhouette_counts(v, cuda(target), group=2, return_silhouettes=True, **camera(scene))
    counts, masks = counts.cpu().numpy(), masks.cpu().numpy()
    assert np.array_equal(masks, np.repeat(counted(ORTHO)[1], 2, axis=0))             # camera m // 2
    assert np.array_equal(counts, np.repeat(counted(ORTHO)[0], 2, axis=0))            # target m // 2
    perm = [1, 2, 0]
    moved = renderer.silhouette_counts(v, cuda(target[perm]), group=2, **camera(scene)).cpu().numpy()
    assert np.array_equal(moved, Q.counts_of(masks, np.repeat(target[perm], 2, axis=0))) and not np.array_equal(moved, counts)
    with pytest.raises(_capi.HpsError):
        renderer.silhouette_counts(v, cuda(target), group=4, **camera(scene))


def test_flip_is_the_rotation_by_pi_about_x():
    scene, _, _, target, _ = Q.reference(ORTHO)
    renderer = device(ORTHO)[0]
    v, t = cuda(scene.vertices), cuda(target)
    inside = renderer.silhouette_counts(v, t, flip=True, **camera(scene)).cpu().numpy()
    before = renderer.silhouette_counts(cuda(Q.flipped(scene).vertices), t, flip=False, **camera(scene)).cpu().numpy()
    assert np.array_equal(inside, before)
    assert not np.array_equal(inside, counted(ORTHO)[0])
    assert ((inside[:, 0] + inside[:, 1]) != (counted(ORTHO)[0][:, 0] + counted(ORTHO)[0][:, 1])).all()      # another image in each


def test_two_calls_are_bit_identical_and_the_outputs_do_not_depend_on_each_other():
    scene, _, _, target, _ = Q.reference(ORTHO)
    renderer, (counts, masks) = device(ORTHO)[0], counted(ORTHO)
    v, t, kw = cuda(scene.vertices), cuda(target), camera(scene)
    again = renderer.silhouette_counts(v, t, return_silhouettes=True, **kw)
    assert np.array_equal(again[0].cpu().numpy(), counts) and np.array_equal(again[1].cpu().numpy(), masks)
    other = make_renderer(scene, render_rgb=False)                                    # another workspace, other buffers, no RGB
    only_counts = other._silhouette(v, t, kw["cam_t"], kw.get("orthographic_scale"), 1, False, True, False)
    assert only_counts[1] is None and np.array_equal(only_counts[0].cpu().numpy(), counts)
    other._silhouette_bufs[(scene.B, 1)]["counts"].fill_(-1)
    only_masks = other._silhouette(v, t, kw["cam_t"], kw.get("orthographic_scale"), 1, False, False, True)
    assert only_masks[0] is None and np.array_equal(only_masks[1].cpu().numpy(), masks)
    assert bool((other._silhouette_bufs[(scene.B, 1)]["counts"] == -1).all())         # not written when not wanted


def test_tracker_takes_counts_and_masks_alike_on_the_device():
    scene, _, m64, target, want = Q.reference(ORTHO)
    renderer = device(ORTHO)[0]
    v, t, kw = cuda(scene.vertices), cuda(target), camera(scene)
    metrics = ["silhouette-IOU", "silhouettesamples-IOU"]
    v2 = v.repeat_interleave(2, dim=0)
    results = []
    for fused in (True, False):
        tracker = EvalMetricsTracker(metrics, silhouette_renderer=renderer)
        tracker.initialise_metric_sums()
        tracker.initialise_per_frame_metric_lists()
        counts, masks = renderer.silhouette_counts(v, t, return_silhouettes=True, **kw)
        counts, masks = counts.clone(), masks.clone()
        counts2, masks2 = renderer.silhouette_counts(v2, t, group=2, return_silhouettes=True, **kw)
        if fused:
            pred, tgt = {"silhouette_counts": counts, "silhouettesamples_counts": counts2}, {}
        else:
            pred, tgt = {"silhouettes": masks, "silhouettessamples": masks2.view(3, 2, 64, 64)}, {"silhouettes": t}
        _, per_frame = tracker.update_per_batch(pred, tgt, 3, return_per_frame_metrics=True)
        assert all(torch.is_tensor(s) and s.is_cuda and s.dtype == torch.float64 for s in tracker.metric_sums.values())
        sums = {k: float(s) for k, s in tracker.metric_sums.items()}
        tracker.reduce_across_ranks()                                                 # no process group: a no-op on the new keys
        assert {k: float(s) for k, s in tracker.metric_sums.items()} == sums and tracker.total_samples == 3
        results.append((sums, per_frame["silhouette-IOU"].cpu().numpy(), tracker.compute_final_metrics(verbose=False)))
    assert results[0][0] == results[1][0] and np.array_equal(results[0][1], results[1][1]) and results[0][2] == results[1][2]
    sums, per_frame, final = results[0]
    got = counted(ORTHO)[0]                                                           # equal to the yardstick's unless a near-tie was printed
    tp, fp, tn, fn = got.sum(axis=0).astype(np.float64)
    assert [sums["num_true_positives"], sums["num_false_positives"], sums["num_true_negatives"], sums["num_false_negatives"]] == [tp, fp, tn, fn]
    assert sums["num_samples_true_positives"] == 2 * tp and sums["num_samples_false_negatives"] == 2 * fn
    assert np.array_equal(per_frame, Q.iou_of(got))
    assert final["silhouette-IOU"] == tp / (tp + fp + fn) == final["silhouettesamples-IOU"]
    if np.array_equal(got, want):
        wtp, wfp, _, wfn = want.sum(axis=0).astype(np.float64)
        assert final["silhouette-IOU"] == wtp / (wtp + wfp + wfn)


def test_per_frame_iou_of_an_empty_frame_is_nan():
    counts = cuda(counted("w40_f257_b3")[0])
    tracker = EvalMetricsTracker(["silhouette-IOU"], silhouette_renderer=device("w40_f257_b3")[0])
    tracker.initialise_metric_sums()
    tracker.initialise_per_frame_metric_lists()
    _, per_frame = tracker.update_per_batch({"silhouette_counts": counts}, {}, 3, return_per_frame_metrics=True)
    iou = per_frame["silhouette-IOU"].cpu().numpy()
    assert np.isnan(iou[2]) and np.array_equal(iou, Q.iou_of(counted("w40_f257_b3")[0]), equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# the evaluation harness
# ---------------------------------------------------------------------------------------------------------------------------------
NEW_METRICS = ["silhouette-IOU", "joints2D-L2E", "joints2Dsamples-L2E", "silhouettesamples-IOU"]
SSP3D_METRICS = ["PVE-PA", "PVE-T-SC"] + NEW_METRICS                                  # run_evaluate.py:67-68


class _SyntheticSSP3DDataset(_SyntheticEvalDataset):
    """The items of tests/test_gpu_evaluate.py with the two keys data/ssp3d_eval_dataset.py:87-94 adds, as numpy arrays like there."""

    def __init__(self, n, wh):
        super().__init__(n, wh=wh)
        rs = np.random.RandomState(17)
        rr, cc = np.indices((wh, wh))
        for it in self.items:
            cy, cx, ry, rx = rs.uniform(0.4 * wh, 0.6 * wh, 2).tolist() + rs.uniform(0.15 * wh, 0.4 * wh, 2).tolist()
            it["silhouette"] = ((((rr - cy) / ry) ** 2 + ((cc - cx) / rx) ** 2) <= 1).astype(np.uint8)
            it["keypoints"] = rs.uniform(0.2 * wh, 0.8 * wh, (17, 2)).astype(np.float32)


def _densepose(num_verts, seed=23, num_faces=300):
    """A DensePose tuple from a seed: every SMPL vertex once and about 5 % of them a second time, ``num_faces`` faces over those,
    part labels 1 + i % 24."""
    rs = np.random.RandomState(seed)
    verts_map = np.concatenate([np.arange(num_verts), rs.randint(0, num_verts, num_verts // 20)])
    Nd = len(verts_map)
    faces = np.stack([rs.choice(Nd, 3, replace=False) for _ in range(num_faces)]).astype(np.int64)
    iuv = np.stack([1 + np.arange(Nd) % 24, rs.rand(Nd), rs.rand(Nd)], axis=1).astype(np.float32)
    return (torch.from_numpy(rs.rand(1, Nd, 2).astype(np.float32)), torch.from_numpy(iuv)[None], torch.from_numpy(verts_map),
            torch.from_numpy(faces)[None])


@pytest.fixture(scope="module")
def harness(dev, net_gpu, smpl_gpu):
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd.evaluate_poseMF_shapeGaussian_net import evaluate_pose_MF_shapeGaussian_net
    from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL
    cfg = configs.get_cfg_defaults()
    wh = cfg.DATA.PROXY_REP_SIZE
    gendered = {k: SMPL(smpl_data.synthetic_smpl_model(s), gender=g).to(dev) for k, s, g in (("m", 1, "male"), ("f", 2, "female"))}
    det = CannyEdgeDetector(cfg.DATA.EDGE_NMS, cfg.DATA.EDGE_GAUSSIAN_STD, cfg.DATA.EDGE_GAUSSIAN_SIZE, cfg.DATA.EDGE_THRESHOLD).to(dev)
    renderer = tr.TexturedIUVRenderer(dev, 1, img_wh=wh, projection_type="orthographic", render_rgb=False, bin_size=32,
                                      densepose_uv=_densepose(smpl_gpu.num_verts))
    ds = _SyntheticSSP3DDataset(3, wh)

    def run(metrics, N, batch_size):
        return evaluate_pose_MF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, gendered["m"], gendered["f"], det, dev, ds, metrics, None,
                                                  num_workers=0, pin_memory=False, save_per_frame_metrics=False,
                                                  num_samples_for_metrics=N, batch_size=batch_size, seed=77,
                                                  silhouette_renderer=renderer)
    return SimpleNamespace(cfg=cfg, wh=wh, det=det, renderer=renderer, ds=ds, run=run, net=net_gpu, smpl=smpl_gpu)


@functools.lru_cache(maxsize=None)
def _evaluated(run, N, batch_size):
    return run(tuple(SSP3D_METRICS) if N > 1 else tuple(NEW_METRICS), N, batch_size)


def test_harness_mode_metrics_equal_a_recomputation(harness):
    """silhouette-IOU from forward()'s image of the flipped mode mesh plus numpy, exactly; joints2D-L2E from the model's joints in
    float64, within 16 x the deviation of the same recomputation in float32 from it (S.FACTOR, as the other scenario files do)."""
    h = harness
    got = _evaluated(h.run, 4, 1)
    from hierarchicalprobabilistic3dhuman_amd.rigid_transform_utils import batch_rodrigues, rot6d_to_rotmat
    counts, err = np.zeros(4), {np.float32: [], np.float64: []}
    with torch.no_grad():
        for it in h.ds.items:
            edges = h.det(it["image"][None].cuda())
            edge = edges["thresholded_thin_edges"] if h.cfg.DATA.EDGE_NMS else edges["thresholded_grad_magnitude"]
            _, _, _, _, mode, shape_dist, glob, cam = h.net(torch.cat([edge, it["heatmaps"][None].cuda()], dim=1))
            glob_R = batch_rodrigues(glob) if glob.shape[-1] == 3 else rot6d_to_rotmat(glob)
            out = h.smpl(body_pose=mode, global_orient=glob_R.unsqueeze(1), betas=shape_dist.loc, pose2rot=False)
            cam_t = torch.cat([cam[:, 1:], torch.full_like(cam[:, :1], 2.5)], dim=-1)
            iuv = h.renderer(vertices=cam_utils.flip_about_x(out.vertices), cam_t=cam_t,
                             orthographic_scale=cam[:, [0, 0]].contiguous())["iuv_images"].cpu().numpy()
            counts += Q.counts_of(Q.mask_of(iuv), it["silhouette"][None])[0]
            for dt in err:
                j = out.joints[0, ALL_JOINTS_TO_COCO_MAP].cpu().numpy().astype(dt) * np.array([1, -1, -1], dtype=dt)
                c = cam[0].cpu().numpy().astype(dt)
                j2d = (c[0] * (j[:, :2] + c[1:]) + dt(1)) * dt(h.wh / 2.0)
                err[dt].append(np.linalg.norm(j2d.astype(np.float64) - it["keypoints"].astype(np.float64), axis=-1))
    tp, fp, tn, fn = counts
    assert tp > 0 and fp > 0 and fn > 0                                               # the meshes and the targets overlap in part
    assert got["silhouette-IOU"] == tp / (tp + fp + fn)
    want64, want32 = float(np.mean(err[np.float64])), float(np.mean(err[np.float32]))
    print("joints2D-L2E %.9f float64 %.9f float32 deviation %.3e" % (got["joints2D-L2E"], want64, abs(want32 - want64)))
    assert abs(got["joints2D-L2E"] - want64) <= S.FACTOR * abs(want32 - want64)
    assert all(np.isfinite(got[m]) for m in SSP3D_METRICS) and 0 < got["silhouettesamples-IOU"] < 1


def test_harness_one_sample_is_the_mode_mesh(harness):
    got = _evaluated(harness.run, 1, 1)
    assert got["silhouettesamples-IOU"] == got["silhouette-IOU"]


def test_harness_values_do_not_depend_on_the_batch_size(harness):
    one, three = _evaluated(harness.run, 4, 1), _evaluated(harness.run, 4, 3)
    for m in NEW_METRICS:
        assert one[m] == three[m], (m, one[m], three[m])
