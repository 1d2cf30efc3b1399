"""Times of the training loss-and-metrics tracker and of one full training step on the GPU.

    python tools/train_step_time.py [--batch 72] [--img 256] [--windows 9] [--iters 20] [--steps 6] [--out FILE.json]

At the reference's batch of 72, 256 x 256 inputs, 6890 vertices, 14 / 17 joints, 8 samples, all ten metrics:

  (a) TrainingLossesAndMetricsTracker.update_per_batch -- one hps_train_metrics_update call;
  (b) the same ten sums composed from what the package offered before: eight eval_utils.pointset_errors calls, torch operations for the
      two 2-D metrics, float64 adds into running sums on the device, and loss.item() as the reference's tracker calls it;
  (c) one full SyntheticTrainStep (data generation, forward, loss, backward, DeviceAdam, tracker) in stage 1 and in stage 2, on the
      synthetic SMPL model and a seeded DensePose-style asset set, with the tracker's share of it.

(a) and (b) are timed with device events around windows of ``--iters`` calls, ``--windows`` windows each, alternating, after a warm-up
of both; the figures are the median window's time per call and the spread (the windows' minimum and maximum).  (b) ends every call
with loss.item(), so its window is also a host wait; (a) never waits.  The kernels each issues are counted from a torch.profiler
(roctracer) trace of one call, not assumed.  (c) is a host clock around ``--steps`` steps ending in a synchronise, per window.
Required by the issue that added the tracker: (a) no slower than (b) beyond the spread, and at most four kernels per update.
Fails without a HIP device; nothing here runs on the CPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import configs, eval_utils, smpl_data  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd import textured_renderer as tr, train_poseMF_shapeGaussian_net as tp  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.device_optim import DeviceAdam  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.matrix_fisher_loss import PoseMFShapeGaussianLoss  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.poseMF_shapeGaussian_net import PoseMFShapeGaussianNet  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.smpl_official import SMPL  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.train_loss_and_metrics_tracker import METRIC_NAMES, TrainingLossesAndMetricsTracker  # noqa: E402

MODES = {"": eval_utils.MODE_RAW, "-SC": eval_utils.MODE_SC, "-PA": eval_utils.MODE_PA}


def tracker_inputs(B, P, J, K, N, img_wh, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g)
    target = {"verts": 0.3 * r(B, P, 3), "joints3D": 0.3 * r(B, J, 3), "joints2D": torch.rand(B, K, 2, generator=g) * img_wh,
              "joints2D_vis": torch.rand(B, K, generator=g) > 0.25}
    pred = {"verts": target["verts"] + 0.05 * r(B, P, 3), "joints3D": target["joints3D"] + 0.05 * r(B, J, 3),
            "joints2D": (target["joints2D"] + 6 * r(B, K, 2)) / (img_wh / 2.0) - 1,
            "joints2Dsamples": (target["joints2D"][:, None] + 9 * r(B, N, K, 2)) / (img_wh / 2.0) - 1}
    t_rep = 0.3 * r(B, P, 3)
    cuda = lambda d: {k: v.to(dev) for k, v in d.items()}
    return cuda(pred), cuda(target), (t_rep + 0.02 * r(B, P, 3)).to(dev), t_rep.to(dev), torch.tensor(3.5, device=dev)


class Composed:
    """(b): what the parent commit offers for the same sums."""

    def __init__(self, img_wh, dev):
        self.img_wh = img_wh
        self.sums = {m: torch.zeros((), dtype=torch.float64, device=dev) for m in METRIC_NAMES}
        self.visible = torch.zeros((), dtype=torch.float64, device=dev)
        self.loss, self.samples = 0.0, 0

    def update(self, loss, pred, target, batch_size, pred_reposed, target_reposed):
        self.loss += loss.item() * batch_size                       # the reference's line 114: drains the stream
        self.samples += batch_size
        for sfx, mode in MODES.items():
            self.sums["PVE" + sfx] += eval_utils.pointset_errors(pred["verts"], target["verts"], mode).sum()
            self.sums["MPJPE" + sfx] += eval_utils.pointset_errors(pred["joints3D"], target["joints3D"], mode).sum()
        for sfx in ("", "-SC"):
            self.sums["PVE-T" + sfx] += eval_utils.pointset_errors(pred_reposed, target_reposed, MODES[sfx]).sum()
        px = (pred["joints2D"] + 1) * (self.img_wh / 2.0)
        self.sums["joints2D-L2E"] += torch.norm(px - target["joints2D"], dim=-1).double().sum()
        ps = (pred["joints2Dsamples"] + 1) * (self.img_wh / 2.0)
        err = torch.norm(ps - target["joints2D"][:, None], dim=-1).double() * target["joints2D_vis"][:, None]
        self.sums["joints2Dsamples-L2E"] += err.sum()
        self.visible += target["joints2D_vis"].sum() * ps.shape[1]


def window(fn, iters):
    """Device-event time of ``iters`` calls, ms per call."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def kernels_of(fn):
    """Names of the kernels one call issues, from a torch.profiler trace (None if the profiler records no device activity here)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    return names or None


def summary(values):
    return dict(median=statistics.median(values), min=min(values), max=max(values))


def make_step(B, W, dev, stage, cfg):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import render_scenario as RS
    sc = RS.make_scene(7, 1, 64, 83, 83, num_faces=13774, duplicates=938.0 / 6891.0)
    dp = (torch.from_numpy(sc.verts_uv)[None], torch.from_numpy(sc.verts_iuv)[None], torch.from_numpy(np.minimum(sc.verts_map, 6889)),
          torch.from_numpy(sc.faces)[None])
    torch.manual_seed(0)
    net = PoseMFShapeGaussianNet(configs.SMPL_PARENTS, cfg).to(dev)
    smpl = SMPL(smpl_data.synthetic_smpl_model(0)).to(dev)
    d = cfg.DATA
    edge = CannyEdgeDetector(non_max_suppression=d.EDGE_NMS, gaussian_filter_std=d.EDGE_GAUSSIAN_STD, gaussian_filter_size=d.EDGE_GAUSSIAN_SIZE,
                             threshold=d.EDGE_THRESHOLD).to(dev)
    renderer = tr.TexturedIUVRenderer(dev, B, img_wh=W, projection_type="perspective",
                                      perspective_focal_length=cfg.TRAIN.SYNTH_DATA.FOCAL_LENGTH, render_rgb=True, densepose_uv=dp)
    criterion = PoseMFShapeGaussianLoss(loss_config=cfg.LOSS.STAGE1 if stage == 1 else cfg.LOSS.STAGE2, img_wh=W)
    opt = DeviceAdam(net.parameters(), lr=cfg.TRAIN.LR, refresh=(net,))
    metrics = list(METRIC_NAMES[:9]) + ["joints2Dsamples-L2E"] * (stage == 2)
    tracker = TrainingLossesAndMetricsTracker(metrics, W, None)
    tracker.initialise_loss_metric_sums()
    net.set_batchnorm_training(True)
    net.set_differentiable_factors(True)
    net.train()
    step = tp.SyntheticTrainStep(net, cfg, smpl, edge, renderer, dev, criterion, opt, tracker)
    g = torch.Generator().manual_seed(1)
    batch = {"pose": (0.3 * torch.randn(B, 72, generator=g)).to(dev), "background": torch.rand(B, 3, W, W, generator=g).to(dev),
             "texture": torch.rand(1, 1200, 800, 3, generator=g).to(dev).expand(B, -1, -1, -1).contiguous()}
    return step, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=72)
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--skip-step", action="store_true", help="(a) and (b) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/train_step_time.py needs a HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    B, W, N = args.batch, args.img, args.samples
    pred, target, p_rep, t_rep, loss = tracker_inputs(B, 6890, 14, 17, N, W, dev)
    tracker = TrainingLossesAndMetricsTracker(list(METRIC_NAMES), W, None)
    tracker.initialise_loss_metric_sums()
    composed = Composed(W, dev)
    a = lambda: tracker.update_per_batch("train", loss, pred, target, B, pred_reposed_vertices=p_rep, target_reposed_vertices=t_rep)
    b = lambda: composed.update(loss, pred, target, B, p_rep, t_rep)
    for _ in range(5):
        a()
        b()
    torch.cuda.synchronize()
    # the two compute the same sums
    got = tracker.device_sums()[0].cpu().numpy()
    for i, m in enumerate(METRIC_NAMES):
        want = float(composed.sums[m])
        assert abs(got[2 + i] - want) <= 1e-6 * abs(want), (m, got[2 + i], want)
    assert got[12] == float(composed.visible) and got[1] == composed.samples
    ka, kb = kernels_of(a), kernels_of(b)
    ta, tb = [], []
    for _ in range(args.windows):                                # alternating windows
        ta.append(window(a, args.iters))
        tb.append(window(b, args.iters))
    out = dict(batch=B, img_wh=W, samples=N, windows=args.windows, iters=args.iters,
               update_per_batch_ms=summary(ta), composed_ms=summary(tb),
               update_per_batch_kernels=None if ka is None else len(ka), composed_kernels=None if kb is None else len(kb),
               update_per_batch_kernel_names=ka)
    print("(a) update_per_batch        : median %.4f ms  (min %.4f, max %.4f) per call; kernels per call: %s" % (
        out["update_per_batch_ms"]["median"], min(ta), max(ta), out["update_per_batch_kernels"]))
    print("(b) composed + loss.item()  : median %.4f ms  (min %.4f, max %.4f) per call; kernels per call: %s" % (
        out["composed_ms"]["median"], min(tb), max(tb), out["composed_kernels"]))
    if ka is not None:
        print("    kernels of (a):", ka)
        assert len(ka) <= 4, ka
    assert out["update_per_batch_ms"]["median"] <= out["composed_ms"]["median"] + (max(ta) - min(ta)) + (max(tb) - min(tb)), "(a) is slower than (b)"
    if not args.skip_step:
        cfg = configs.get_cfg_defaults()
        cfg.DATA.PROXY_REP_SIZE, cfg.TRAIN.BATCH_SIZE, cfg.LOSS.NUM_SAMPLES, cfg.LOSS.SAMPLE_ON_CPU = W, B, N, False
        cfg.TRAIN.SYNTH_DATA.FOCAL_LENGTH = 300.0 * W / 256.0
        for stage in (1, 2):
            step, batch = make_step(B, W, dev, stage, cfg)
            for _ in range(3):
                step(batch, "train")
            torch.cuda.synchronize()
            times = []
            for _ in range(max(3, args.windows // 2)):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step(batch, "train")
                torch.cuda.synchronize()
                times.append(1e3 * (time.perf_counter() - t0) / args.steps)
            s = summary(times)
            out["train_step_stage%d_ms" % stage] = s
            print("(c) full train step, stage %d: median %.2f ms  (min %.2f, max %.2f); the tracker's update is %.2f %% of it" % (
                stage, s["median"], s["min"], s["max"], 100.0 * out["update_per_batch_ms"]["median"] / s["median"]))
            del step, batch
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
