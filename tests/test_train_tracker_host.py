"""CPU: the training loss-and-metrics tracker without a device -- the float64 restatement of tests/train_tracker_scenario.py held to the
reference's own class (tests/golden/train_tracker_golden.json), the structure of update_per_batch with the library call recorded,
history / pickle / load_history, the best-weights rule, checkpoint_utils, and the host-side argument refusals of
hps_train_metrics_update."""
import copy
import ctypes
import json
import os
import pickle

import numpy as np
import pytest
import torch

import encoder_call_trace as T
import train_tracker_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, checkpoint_utils, train_loss_and_metrics_tracker as tlm
from hierarchicalprobabilistic3dhuman_amd.train_loss_and_metrics_tracker import TrainingLossesAndMetricsTracker

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the restatement against the reference itself ----
def test_restatement_matches_the_reference_tracker():
    """|reference - r64| <= 4 max(|r32 - r64|, 2^-23 |r64|) for every key of epochs_history: the reference's float32 sums stay inside
    the project's rule (worst measured ratio 0.21), so the float64 restatement is a fair truth for the device."""
    with open(os.path.join(HERE, "golden", "train_tracker_golden.json")) as f:
        golden = json.load(f)
    assert golden["case"] == json.loads(json.dumps(S.GOLDEN))
    updates = S.golden_updates()
    h64, _ = S.run_restated(updates, S.METRICS, S.GOLDEN["img_wh"], np.float64)
    h32, _ = S.run_restated(updates, S.METRICS, S.GOLDEN["img_wh"], np.float32)
    assert set(golden["epochs_history"]) == set(h64)
    worst = 0.0
    for key in sorted(h64):
        (ref,), (r64,), (r32,) = golden["epochs_history"][key], h64[key], h32[key]
        bound = S.history_bound(r64, r32)
        print("%-28s reference %.9g  r64 %.9g  r32 %.9g  err %.3e  bound %.3e  ratio %.3f" % (key, ref, r64, r32, abs(ref - r64), bound,
                                                                                           abs(ref - r64) / bound))
        assert abs(ref - r64) <= bound, key
        worst = max(worst, abs(ref - r64) / bound)
    print("worst ratio %.3f" % worst)
    # the visibility of the golden case hides some joints, and not all
    assert all(0 < c["vis"].sum() < c["vis"].size for _, c in updates)


def test_restatement_notices_a_wrong_tracker():
    """The rule is tight enough to tell: the SC scale in the PA slot, invisible joints counted, a dropped batch."""
    updates = S.golden_updates()
    h64, r = S.run_restated(updates, S.METRICS, 256, np.float64)
    h32, _ = S.run_restated(updates, S.METRICS, 256, np.float32)
    bound = lambda k: S.history_bound(h64[k][0], h32[k][0])
    assert abs(h64["train_PVE-SC"][0] - h64["train_PVE-PA"][0]) > 1e3 * bound("train_PVE-PA")
    c = updates[0][1]
    everything = float(S.j2d_errors(c, np.float64, True).sum() / (c["B"] * c["N"] * c["K"]))
    visible, _, n = S.j2d_truth(c, True)
    assert abs(everything - visible / n) > 1e3 * bound("train_joints2Dsamples-L2E")
    h_short, _ = S.run_restated(updates[:3], S.METRICS, 256, np.float64)
    assert abs(h_short["val_PVE"][0] - h64["val_PVE"][0]) > 1e3 * bound("val_PVE")


# ---- structure, with the library call recorded ----
FIELDS = [name for name, _ in _capi.TrainMetricsArgs._fields_]


def dicts_of(c, device="cpu"):
    t = lambda a: torch.from_numpy(np.array(a)).to(device)
    pred = {"verts": t(c["pred_verts"]), "joints3D": t(c["pred_joints3d"]), "joints2D": t(c["pred_joints2d"]),
            "joints2Dsamples": t(c["pred_joints2d_samples"])}
    target = {"verts": t(c["target_verts"]), "joints3D": t(c["target_joints3d"]), "joints2D": t(c["target_joints2d"]),
              "joints2D_vis": t(c["vis"])}
    return pred, target, t(c["pred_reposed"]), t(c["target_reposed"]), torch.tensor(float(c["loss"]), dtype=torch.float32, device=device)


@pytest.fixture
def recorded(monkeypatch):
    """(calls, tracker factory): inside, _capi.call records (entry, the argument block's fields) instead of calling."""
    calls = []
    with T.recording(monkeypatch):
        def call(entry, *args):
            block = ctypes.cast(args[0], ctypes.POINTER(_capi.TrainMetricsArgs)).contents
            calls.append((entry, {f: getattr(block, f) for f in FIELDS}))
        monkeypatch.setattr(_capi, "call", call)
        yield calls


def test_one_update_is_one_library_call(recorded):
    c = S.case(1, 2, 40, 14, 17, 3)
    metrics = list(S.METRICS[:9])
    tracker = TrainingLossesAndMetricsTracker(metrics, 256, None)
    tracker.initialise_loss_metric_sums()
    pred, target, pr, tr, loss = dicts_of(c)
    before = (dict(pred), dict(target))
    tracker.update_per_batch("train", loss, pred, target, 2, pred_reposed_vertices=pr, target_reposed_vertices=tr)
    assert [e for e, _ in recorded] == ["hps_train_metrics_update"]
    a = recorded[0][1]
    assert (a["B"], a["P"], a["J"], a["K"], a["N"], a["batch_size"], a["split"], a["mask"]) == (2, 40, 14, 17, 0, 2, 0, 0x1ff)
    assert a["pred_joints2d_samples"] is None and a["vis"] is None and a["status"] is None and a["num_status"] == 0
    assert a["pred_verts"] == pred["verts"].data_ptr() and a["target_joints2d"] == target["joints2D"].data_ptr()      # no copy of fp32 inputs
    assert a["struct_bytes"] == ctypes.sizeof(_capi.TrainMetricsArgs) == _capi.load().hps_sizeof_train_metrics_args()
    # the caller's dicts are untouched: the same keys, the same tensor objects (the reference replaces them by numpy arrays)
    assert pred.keys() == before[0].keys() and all(pred[k] is before[0][k] for k in pred)
    assert target.keys() == before[1].keys() and all(target[k] is before[1][k] for k in target)
    # metrics_to_track is read at each call: the loop's append at the stage change
    metrics.append("joints2Dsamples-L2E")
    status = torch.zeros(2, dtype=torch.int32)
    tracker.update_per_batch("val", loss, pred, target, 2, pred_reposed_vertices=pr, target_reposed_vertices=tr, status=status)
    tracker.update_per_batch("val", loss, pred, target, 2, pred_reposed_vertices=pr, target_reposed_vertices=tr, status=status)
    assert len(recorded) == 3
    b, c3 = recorded[1][1], recorded[2][1]
    assert (b["mask"], b["split"], b["N"], b["num_status"]) == (0x3ff, 1, 3, 2) and b["status"] == status.data_ptr()
    assert b["vis"] == target["joints2D_vis"].data_ptr()
    # buffer addresses do not change between calls
    for f in ("workspace", "sums"):
        assert a[f] == b[f] == c3[f] and a[f]
    assert b == c3


def test_leading_dimensions_are_flattened_and_bad_shapes_refused(recorded):
    c = S.case(2, 6, 10, 14, 17, 2)
    tracker = TrainingLossesAndMetricsTracker(["PVE", "MPJPE-PA"], 256, None)
    tracker.initialise_loss_metric_sums()
    pred, target, pr, tr, loss = dicts_of(c)
    views = lambda d: {k: (v.reshape(2, 3, *v.shape[1:]) if k in ("verts", "joints3D") else v) for k, v in d.items()}
    tracker.update_per_batch("train", loss, views(pred), views(target), 2)
    a = recorded[0][1]
    assert (a["B"], a["P"], a["J"], a["batch_size"], a["mask"]) == (6, 10, 14, 2, 0x81)
    with pytest.raises(_capi.HpsError):
        tracker.update_per_batch("train", loss, dict(pred, verts=pred["verts"][:, :9]), target, 2)
    with pytest.raises(_capi.HpsError):
        tracker.update_per_batch("train", loss, dict(pred, joints3D=pred["joints3D"][:5]), target, 2)
    with pytest.raises(AssertionError):
        tracker.update_per_batch("test", loss, pred, target, 2)
    tracker.metrics_to_track.append("PVE-T")
    with pytest.raises(AssertionError):
        tracker.update_per_batch("train", loss, pred, target, 2)          # reposed vertices missing, as in the reference


def test_cpu_tensors_are_refused():
    c = S.case(1, 2, 40)
    tracker = TrainingLossesAndMetricsTracker(list(S.METRICS), 256, None)
    tracker.initialise_loss_metric_sums()
    pred, target, pr, tr, loss = dicts_of(c)
    with pytest.raises(_capi.HpsError):
        tracker.update_per_batch("train", loss, pred, target, 2, pred_reposed_vertices=pr, target_reposed_vertices=tr)
    fresh = TrainingLossesAndMetricsTracker(["PVE"], 256, None)
    with pytest.raises(_capi.HpsError):
        fresh.update_per_epoch()


# ---- epochs: history, pickle, load_history ----
def with_sums(tracker, rows):
    """Put ``rows`` (2, NSLOT) where update_per_batch leaves the device sums (a CPU tensor reads back the same way)."""
    tracker._sums = torch.tensor(rows, dtype=torch.float64)


def test_history_pickle_and_load_history_round_trip(tmp_path, capsys):
    path = str(tmp_path / "log.pkl")
    metrics = ["PVE", "MPJPE-PA", "joints2D-L2E", "joints2Dsamples-L2E"]
    tracker = TrainingLossesAndMetricsTracker(metrics, 256, path)
    assert list(tracker.epochs_history) == ["train_losses", "val_losses"] + tracker.all_metrics_types
    assert tracker.all_metrics_types[:4] == ["train_PVE", "val_PVE", "train_PVE-SC", "val_PVE-SC"] and len(tracker.all_metrics_types) == 20
    for epoch in range(3):
        tracker.initialise_loss_metric_sums()
        assert tracker.loss_metric_sums["train_num_samples"] == 0 and "val_num_visib_joints2Dsamples" in tracker.loss_metric_sums
        rows = np.zeros((2, tlm.NSLOT))
        rows[:, tlm.SLOT_LOSS], rows[:, tlm.SLOT_SAMPLES] = [12.0 + epoch, 6.0], [4, 2]
        rows[0, tlm.SLOT_METRIC0 + 0], rows[1, tlm.SLOT_METRIC0 + 7] = 6890.0 * 4 * 0.5, 14.0 * 2 * 0.25
        rows[:, tlm.SLOT_METRIC0 + 8], rows[:, tlm.SLOT_METRIC0 + 9], rows[:, tlm.SLOT_VISIBLE] = [17.0 * 4 * 3.0, 0.0], [90.0, 0.0], [30, 0]
        rows[0, tlm.SLOT_METRIC0 + 1] = 123.0                                        # PVE-SC is not tracked: 0 in the history
        with_sums(tracker, rows)
        tracker.update_per_epoch()
    out = capsys.readouterr().out
    assert "Finished epoch." in out and "Train Loss: 3.50000, Val Loss: 3.00000" in out and "Train PVE: 0.50000" in out
    h = tracker.epochs_history
    assert h["train_losses"] == [3.0, 3.25, 3.5] and h["val_losses"] == [3.0] * 3
    assert h["train_PVE"] == [0.5] * 3 and h["val_MPJPE-PA"] == [0.25] * 3 and h["train_PVE-SC"] == [0.0] * 3
    assert h["train_joints2D-L2E"] == [3.0] * 3 and h["train_joints2Dsamples-L2E"] == [3.0] * 3
    assert all(np.isnan(v) for v in h["val_joints2Dsamples-L2E"])                   # no visible joint all epoch: the reference's 0 / 0
    assert all(type(v) is float for values in h.values() for v in values)           # plain Python floats in the pickle
    assert tracker.loss_metric_sums["train_PVE"] == 6890.0 * 2 and tracker.loss_metric_sums["train_num_samples"] == 4
    with open(path, "rb") as f:
        np.testing.assert_equal(pickle.load(f), h)
    resumed = TrainingLossesAndMetricsTracker(metrics, 256, path, load_logs=True, current_epoch=2)
    assert all(len(v) == 2 for v in resumed.epochs_history.values()) and resumed.epochs_history["train_losses"] == [3.0, 3.25]
    # a metric the log lacks is filled with zeros; a list that is too short is refused
    with open(path, "rb") as f:
        log = pickle.load(f)
    del log["val_PVE-T"]
    with open(path, "wb") as f:
        pickle.dump(log, f)
    assert TrainingLossesAndMetricsTracker(metrics, 256, path, load_logs=True, current_epoch=3).epochs_history["val_PVE-T"] == [0.0] * 3
    with pytest.raises(AssertionError):
        TrainingLossesAndMetricsTracker(metrics, 256, path, load_logs=True, current_epoch=4)


def test_divisors_come_from_the_shapes_and_status_raises_at_the_epoch(recorded):
    c = S.case(3, 2, 40, 9, 5, 2)
    tracker = TrainingLossesAndMetricsTracker(["PVE", "MPJPE", "joints2D-L2E"], 64, None)
    tracker.initialise_loss_metric_sums()
    pred, target, pr, tr, loss = dicts_of(c)
    tracker.update_per_batch("train", loss, pred, target, 2)
    rows = np.zeros((2, tlm.NSLOT))
    rows[:, tlm.SLOT_SAMPLES] = 2
    rows[0, tlm.SLOT_METRIC0 + 0], rows[0, tlm.SLOT_METRIC0 + 5], rows[0, tlm.SLOT_METRIC0 + 8] = 40 * 2 * 1.5, 9 * 2 * 2.5, 5 * 2 * 3.5
    with_sums(tracker, rows)
    tracker.update_per_epoch()
    h = tracker.epochs_history
    assert (h["train_PVE"], h["train_MPJPE"], h["train_joints2D-L2E"]) == ([1.5], [2.5], [3.5])
    rows[1, tlm.SLOT_STATUS] = 2.0
    tracker.initialise_loss_metric_sums()
    assert float(tracker.device_sums().abs().sum()) == 0.0                       # zeroed in place
    with_sums(tracker, rows)
    with pytest.raises(_capi.HpsError, match="2 image"):
        tracker.update_per_epoch()


def test_determine_save_model_weights_this_epoch():
    tracker = TrainingLossesAndMetricsTracker(["PVE-SC", "MPJPE-PA"], 256, None)
    tracker.epochs_history["val_PVE-SC"] += [0.10, 0.08]
    tracker.epochs_history["val_MPJPE-PA"] += [0.20, 0.21]
    best = {"PVE-SC": 0.09, "MPJPE-PA": 0.21}
    assert tracker.determine_save_model_weights_this_epoch(["PVE-SC", "MPJPE-PA"], best) is True           # equal is not worse
    assert tracker.determine_save_model_weights_this_epoch(["PVE-SC", "MPJPE-PA"], dict(best, **{"MPJPE-PA": 0.2})) is False
    assert tracker.determine_save_model_weights_this_epoch(["PVE-SC"], {"PVE-SC": np.inf}) is True
    assert tracker.determine_save_model_weights_this_epoch([], {}) is True


def test_load_training_info_from_checkpoint(capsys):
    wts = {"w": torch.ones(2)}
    ckpt = {"epoch": 4, "best_epoch": 3, "best_model_state_dict": wts, "best_epoch_val_metrics": {"PVE-SC": 0.1, "MPJPE-PA": 0.2}}
    cur, best, got_wts, metrics = checkpoint_utils.load_training_info_from_checkpoint(copy.deepcopy(ckpt), ["PVE-SC", "MPJPE-PA"])
    assert (cur, best) == (5, 3) and metrics == {"PVE-SC": 0.1, "MPJPE-PA": 0.2} and torch.equal(got_wts["w"], wts["w"])
    # an added metric starts at infinity, a dropped one leaves; the checkpoint's own dict is the one edited and returned
    mine = copy.deepcopy(ckpt)
    cur, best, got_wts, metrics = checkpoint_utils.load_training_info_from_checkpoint(mine, ["PVE-SC", "PVE-PA"])
    assert metrics == {"PVE-SC": 0.1, "PVE-PA": np.inf} and metrics is mine["best_epoch_val_metrics"] and got_wts is mine["best_model_state_dict"]
    assert "Current epoch: 5" in capsys.readouterr().out


# ---- the library's host side ----
def args_for(**kw):
    p = ctypes.c_void_p(64)
    a = _capi.TrainMetricsArgs(struct_bytes=ctypes.sizeof(_capi.TrainMetricsArgs), B=2, P=10, J=14, K=17, N=3, batch_size=2, mask=0x3ff, split=0,
                               num_status=0, img_wh=256.0)
    for f in ("pred_verts", "target_verts", "pred_reposed", "target_reposed", "pred_joints3d", "target_joints3d", "pred_joints2d",
              "target_joints2d", "pred_joints2d_samples", "vis", "loss", "workspace", "sums"):
        setattr(a, f, p)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,text", [
    (dict(struct_bytes=8), b"struct_bytes"), (dict(B=0), b"at least 1"), (dict(batch_size=0), b"at least 1"), (dict(split=2), b"split"),
    (dict(split=-1), b"split"), (dict(mask=0x400), b"mask"), (dict(mask=-1), b"mask"), (dict(loss=None), b"null pointer"),
    (dict(workspace=None), b"null pointer"), (dict(sums=None), b"null pointer"), (dict(sums=ctypes.c_void_p(68)), b"aligned"),
    (dict(pred_verts=None), b"point-set"), (dict(target_reposed=None, mask=0x10), b"point-set"), (dict(pred_joints3d=None, mask=0x80), b"point-set"),
    (dict(P=0), b"P / J"), (dict(J=0, mask=0x20), b"P / J"), (dict(target_joints2d=None, mask=0x100), b"2-D"), (dict(K=0), b"2-D"),
    (dict(img_wh=0.0), b"2-D"), (dict(pred_joints2d=None), b"pred_joints2d"), (dict(vis=None), b"joints2Dsamples"),
    (dict(pred_joints2d_samples=None, mask=0x200), b"joints2Dsamples"), (dict(N=0), b"joints2Dsamples"),
    (dict(status=ctypes.c_void_p(64), num_status=0), b"num_status"), (dict(num_status=3), b"num_status")])
def test_bad_arguments_are_refused_before_any_launch(kw, text):
    """As test_argument_validation_needs_no_gpu: -1 and a message, no device needed (the pointers are never followed)."""
    lib = _capi.load()
    assert lib.hps_train_metrics_update(ctypes.byref(args_for(**kw)), None) == -1
    assert text in lib.hps_last_error(), lib.hps_last_error()
    assert lib.hps_train_metrics_update(None, None) == -1


def test_workspace_kind():
    q = _capi.query_workspace
    per_set = (3 * 17 + 3 * 3 + 3) * 8 + 3 * 3 * 12 * 4
    assert _capi.WS_TRAIN_METRICS == 16 and q(_capi.WS_TRAIN_METRICS, 1) == per_set and q(_capi.WS_TRAIN_METRICS, 72) == 72 * per_set
    lib = _capi.load()
    assert lib.hps_query_workspace(7, 64, 0, 0) == -1 and lib.hps_query_workspace(99, 1, 1, 1) == -1 and lib.hps_query_workspace(17, 1, 0, 0) == -1
    assert tlm.NSLOT == S.NSLOT == 14 and tlm.METRIC_NAMES == S.METRICS
