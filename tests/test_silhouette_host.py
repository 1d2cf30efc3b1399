"""The silhouette metrics without a GPU: the scenario's masks and counts (tests/silhouette_scenario.py) on the closed-form and seeded
scenes, the C ABI's new entry points (exported, prototyped, refusing bad arguments before any launch), the workspace formula, and the
tracker's device-free parts.

The counts asserted here are the float64 restatement's; the float32 restatement gives the same mask in every pixel of every case, which
is why tests/test_gpu_silhouette.py holds the device to exact equality."""
import ctypes

import numpy as np
import pytest
import torch

import render_scenario as S
import silhouette_scenario as Q
from hierarchicalprobabilistic3dhuman_amd import _capi
from hierarchicalprobabilistic3dhuman_amd.eval_metrics_tracker import EvalMetricsTracker, silhouette_counts_from_masks

NEW_SYMBOLS = ("hps_silhouette_iou", "hps_sizeof_silhouette_args")


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenario
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(Q.CLOSED_FORM_TOTALS))
def test_closed_form_totals(name):
    scene, m32, m64, target, counts = Q.reference(name)
    assert int(m64.sum()) == Q.CLOSED_FORM_TOTALS[name]
    assert np.array_equal(m32, m64) and np.array_equal(m64, S.reference(name)[2]["pix_to_face"] >= 0)
    assert (counts.sum(axis=1) == scene.W * scene.W).all()


@pytest.mark.parametrize("name", sorted(Q.ROLLED_COUNTS))
def test_rolled_target_counts(name):
    scene, m32, m64, target, counts = Q.reference(name)
    assert counts.tolist() == Q.ROLLED_COUNTS[name]
    assert np.array_equal(target, np.roll(m64, (2, 3), axis=(1, 2)))
    # float32 and float64 agree on every pixel, and every winner's part label rounds to a part: the mask is the coverage
    assert np.array_equal(m32, m64) and np.array_equal(m64, S.reference(name)[2]["pix_to_face"] >= 0)
    assert (counts.sum(axis=1) == scene.W * scene.W).all()


def test_scenes_cover_what_they_are_for():
    counts = Q.reference("w40_f257_b3")[4]
    assert counts[2].tolist() == [0, 0, 1600, 0] and np.isnan(Q.iou_of(counts)[2]) and not np.isnan(Q.iou_of(counts)[:2]).any()
    m = Q.reference("w36_f257_b2")[2]
    assert m[0][32:, :].any() and m[1][:, 32:].any()                                  # the partial tiles hold set pixels
    # the flipped orthographic scene is another image, every vertex in front of the camera
    scene = S.reference("w64_f2400_b3_ortho")[0]
    fl = Q.flipped(scene)
    assert (S.project(fl, np.float64)[3] > 0).all()
    m_fl = Q.mask_of(S.render(fl, np.float64)["iuv"])
    assert np.array_equal(m_fl, Q.mask_of(S.render(fl, np.float32)["iuv"]))
    assert m_fl.sum(axis=(1, 2)).tolist() == [673, 629, 828] and Q.reference("w64_f2400_b3_ortho")[2].sum(axis=(1, 2)).tolist() == [677, 627, 826]


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def test_silhouette_entry_points_are_exported_and_prototyped():
    """Fails without the feature."""
    lib = ctypes.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), "libhps.so does not export %s" % name
        assert name in _capi.EXPORTED_SYMBOLS
    lib = _capi.load()
    assert lib.hps_version() == 502
    assert lib.hps_sizeof_silhouette_args() == ctypes.sizeof(_capi.SilhouetteArgs)


def test_silhouette_workspace_formula():
    """NDC as a 16-byte record per (mesh, vertex), 16 bytes of counts per (mesh, 8 x 8 tile), a box of two words per face and per chunk
    of 64 faces; the image side travels in d2 above the face count."""
    q = lambda M, Nd, F, W: _capi.query_workspace(_capi.WS_SILHOUETTE, M, Nd, _capi.silhouette_d2(F, W))
    assert _capi.WS_SILHOUETTE == 15 and _capi.silhouette_d2(13774, 256) == 13774 + 256 * 2 ** 32
    assert q(320, 7829, 13774, 256) == 320 * (7829 * 16 + 32 * 32 * 16 + 13774 * 8 + 216 * 8)
    assert q(1, 4, 257, 36) == 4 * 16 + 5 * 5 * 16 + 257 * 8 + 5 * 8
    assert q(2, 4, 1, 4096) == 2 * (4 * 16 + 512 * 512 * 16 + 8 + 8)
    lib = _capi.load()
    for d2 in (13774, _capi.silhouette_d2(13774, 4097), _capi.silhouette_d2(2 ** 24 + 1, 64)):      # no W, W too large, too many faces
        assert lib.hps_query_workspace(_capi.WS_SILHOUETTE, 1, 4, d2) == -1 and b"HPS_WS_SILHOUETTE" in lib.hps_last_error()


def _args(**over):
    fake = ctypes.c_void_p(64)
    a = _capi.SilhouetteArgs()
    a.struct_bytes = ctypes.sizeof(_capi.SilhouetteArgs)
    a.M, a.W, a.group, a.num_verts, a.num_dp_verts, a.num_faces = 4, 16, 2, 4, 4, 2
    a.projection, a.flip_x_pi, a.cam_t_stride, a.scale_stride = _capi.RENDER_ORTHOGRAPHIC, 1, 3, 0
    for name in ("vertices", "verts_map", "faces", "verts_iuv", "cam_t", "scale", "target", "workspace", "counts", "mask_out"):
        setattr(a, name, fake)
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("over,message", [
    (dict(struct_bytes=8), b"struct_bytes"),
    (dict(vertices=None), b"null pointer"),
    (dict(verts_map=None), b"null pointer"),
    (dict(faces=None), b"null pointer"),
    (dict(verts_iuv=None), b"null pointer"),
    (dict(cam_t=None), b"null pointer"),
    (dict(scale=None), b"null pointer"),
    (dict(workspace=None), b"null pointer"),
    (dict(counts=None, mask_out=None), b"no output"),
    (dict(M=0), b"M in"),
    (dict(M=65536, group=1), b"M in"),
    (dict(W=0), b"W in"),
    (dict(W=4097), b"W in"),
    (dict(group=0), b"group"),
    (dict(group=3), b"group"),
    (dict(num_faces=0), b"num_faces"),
    (dict(projection=2), b"projection"),
    (dict(scale_stride=3), b"scale_stride"),
    (dict(workspace=ctypes.c_void_p(72)), b"16-byte"),
    (dict(counts=ctypes.c_void_p(72)), b"16-byte"),
])
def test_silhouette_refuses_bad_arguments_before_any_launch(over, message):
    """Every pointer here is a fake: a call that got as far as a launch would not return -1."""
    lib = _capi.load()
    assert lib.hps_silhouette_iou(None, None) == -1 and b"null pointer" in lib.hps_last_error()
    a = _args(**over)
    assert lib.hps_silhouette_iou(ctypes.addressof(a), None) == -1
    assert message in lib.hps_last_error(), lib.hps_last_error()


# ---------------------------------------------------------------------------------------------------------------------------------
# the tracker
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_tracker_still_refuses_without_a_renderer():
    for m in ("silhouette-IOU", "silhouettesamples-IOU"):
        with pytest.raises(NotImplementedError):
            EvalMetricsTracker(["PVE", m])
        with pytest.raises(NotImplementedError):
            EvalMetricsTracker([m], silhouette_renderer=None)


def test_the_tracker_sums_counts_and_masks_alike():
    """The tracker's own arithmetic is plain tensor operations, so its two input forms can be compared on host tensors: the sums carry
    the reference's names and the final value is tp / (tp + fn + fp) of the yardstick counts."""
    _, _, m64, target, counts = Q.reference("w40_f257_b3")
    metrics = ["silhouette-IOU", "silhouettesamples-IOU"]
    samples = np.stack([m64, np.roll(m64, 1, axis=2)], axis=1)                        # (B,2,W,W)
    sample_counts = np.stack([Q.counts_of(samples[:, k], target) for k in range(2)], axis=1).reshape(-1, 4)
    assert np.array_equal(silhouette_counts_from_masks(torch.from_numpy(samples), torch.from_numpy(target)).numpy(), sample_counts)
    finals = []
    for fused in (False, True):
        t = EvalMetricsTracker(metrics, silhouette_renderer=object())
        t.initialise_metric_sums()
        t.initialise_per_frame_metric_lists()
        assert sorted(t.metric_sums) == sorted("num_%s%s_%s" % (s, a, b) for s in ("", "samples_") for a in ("true", "false")
                                               for b in ("positives", "negatives"))
        if fused:
            pred = {"silhouette_counts": torch.from_numpy(counts).int(), "silhouettesamples_counts": torch.from_numpy(sample_counts).int()}
            tgt = {}
        else:
            pred = {"silhouettes": torch.from_numpy(m64), "silhouettessamples": torch.from_numpy(samples)}
            tgt = {"silhouettes": torch.from_numpy(target)}
        _, per_frame = t.update_per_batch(pred, tgt, 3, return_per_frame_metrics=True)
        assert [float(t.metric_sums[k]) for k in ("num_true_positives", "num_false_positives", "num_true_negatives",
                                                  "num_false_negatives")] == counts.sum(axis=0).tolist()
        assert float(t.metric_sums["num_samples_true_negatives"]) == sample_counts[:, 2].sum()
        assert np.array_equal(per_frame["silhouette-IOU"].numpy(), Q.iou_of(counts), equal_nan=True)
        before = {k: float(v) for k, v in t.metric_sums.items()}
        t.reduce_across_ranks()                                                       # no process group: nothing changes
        assert {k: float(v) for k, v in t.metric_sums.items()} == before and t.total_samples == 3
        finals.append(t.compute_final_metrics(verbose=False))
    tp, fp, _, fn = counts.sum(axis=0).astype(np.float64)
    assert finals[0] == finals[1] and finals[0]["silhouette-IOU"] == tp / (tp + fp + fn)
    tp, fp, _, fn = sample_counts.sum(axis=0).astype(np.float64)
    assert finals[0]["silhouettesamples-IOU"] == tp / (tp + fp + fn)
