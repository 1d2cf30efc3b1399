"""Generates tests/golden/train_tracker_golden.json by IMPORTING THE REFERENCE (only possible where /root/reference exists): the
reference's own metrics/train_loss_and_metrics_tracker.TrainingLossesAndMetricsTracker, run on the CPU on
tests/train_tracker_scenario.py's golden case -- two train and two val updates of B = 2 batches with 6890 vertices (the reference
hard-codes the number), 14 joints, 17 2-D joints with some invisible, 3 samples, all ten metrics -- then update_per_epoch.  What is
committed is data: the reference's ``epochs_history`` (one value per key) and the numpy version it ran under.  The inputs are not
stored; the tests regenerate them from the seeds.

    python tests/golden/make_train_tracker_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from metrics.train_loss_and_metrics_tracker import TrainingLossesAndMetricsTracker  # noqa: E402

import train_tracker_scenario as S  # noqa: E402


def main():
    tracker = TrainingLossesAndMetricsTracker(metrics_to_track=list(S.METRICS), img_wh=S.GOLDEN["img_wh"], log_save_path=None)
    tracker.initialise_loss_metric_sums()
    T = lambda a: torch.from_numpy(np.array(a))
    for split, c in S.golden_updates():
        pred = {"verts": T(c["pred_verts"]), "joints3D": T(c["pred_joints3d"]), "joints2D": T(c["pred_joints2d"]),
                "joints2Dsamples": T(c["pred_joints2d_samples"])}
        target = {"verts": T(c["target_verts"]), "joints3D": T(c["target_joints3d"]), "joints2D": T(c["target_joints2d"]),
                  "joints2D_vis": T(c["vis"])}
        tracker.update_per_batch(split, torch.tensor(float(c["loss"]), dtype=torch.float32), pred, target, c["B"],
                                 pred_reposed_vertices=T(c["pred_reposed"]), target_reposed_vertices=T(c["target_reposed"]))
    tracker.update_per_epoch()
    history = {k: [float(x) for x in v] for k, v in tracker.epochs_history.items()}
    sum_types = {k: type(v).__name__ for k, v in tracker.loss_metric_sums.items()}
    out = dict(case=dict(S.GOLDEN), numpy=np.__version__, epochs_history=history, loss_metric_sum_types=sum_types)
    path = os.path.join(HERE, "train_tracker_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print("wrote", path)


if __name__ == "__main__":
    main()
