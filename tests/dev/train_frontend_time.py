"""Times of the synthetic-data training front end (train/train_poseMF_shapeGaussian_net.py:199-256 minus the renderer) on one MI355X at
the reference's batch, B = 72, D = 256: train_augmentation.SyntheticTrainFrontEnd beside the reference's own way of doing it -- the
restatement of tests/train_frontend_scenario.py run with torch operations on the device, in the same process, on the same inputs and
the same random draws -- and the three new kernels one by one with the bytes they move.

    python tests/dev/train_frontend_time.py [--out profiles/train_frontend_time.txt]

Whole calls: 3 warm-up rounds, then the median of 10 rounds (HIP events around the call, host work included: the plan's draws and
upload on one side, the Python loops and host round trips of the torch route on the other).  Kernels: the median of the same 10
rounds with an event pair around every call into the library.  Bytes are what the algorithm needs, from shapes: the part plane read
by the box kernel; part plane + RGB + background read and rgb_in written by the crop kernel (sampled footprints and composited
pixels counted as whole tensors); joints, affine, counts and plan records for the joints kernel.  Rates as a fraction of the 8 TB/s
HBM peak."""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, train_augmentation as ta  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector  # noqa: E402
from hierarchicalprobabilistic3dhuman_amd.label_conversions import make_proxy_representation  # noqa: E402
import train_frontend_scenario as S  # noqa: E402

HBM_PEAK = 8.0e12
WARMUP, ROUNDS = 3, 10
med = lambda v: sorted(v)[len(v) // 2]


def timed(fn, per_call=None):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
        if per_call is not None:
            per_call()
    return med(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_frontend_time.txt"))
    ap.add_argument("--batch", type=int, default=72)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    B, D = args.batch, 256
    cfg_all = configs.get_cfg_defaults()
    cfg, data = cfg_all.TRAIN.SYNTH_DATA.AUGMENT, cfg_all.DATA
    case = SimpleNamespace(B=B, D=D, H=D, W=D, cfg="default", seed=7)
    inputs = S.make_inputs(case)
    d = {k: v.cuda() for k, v in inputs.items()}
    edge = CannyEdgeDetector(non_max_suppression=data.EDGE_NMS, gaussian_filter_std=data.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=data.EDGE_GAUSSIAN_SIZE, threshold=data.EDGE_THRESHOLD).cuda()
    fe = ta.SyntheticTrainFrontEnd(cfg, D, edge, data.HEATMAP_GAUSSIAN_STD, data.EDGE_NMS, bbox_scale_factor=data.BBOX_SCALE_FACTOR)
    seed = [0]

    def new_route():
        seed[0] += 1
        plan = ta.draw_augment_plan(cfg, B, D, *S.generators(seed[0]))
        return fe(d["iuv"], d["rgb"], d["background"], d["joints2d"], plan=plan)

    def torch_route():
        seed[0] += 1
        r = S.restate(d, cfg, D, *S.generators(seed[0]), device="cuda", record=False)
        out = torch.empty(B, 18, D, D, device="cuda")
        edge.edge_map_into(r["rgb_in"], out, nms=data.EDGE_NMS)
        make_proxy_representation(None, r["joints2D_input"], r["vis"].float(), D, data.HEATMAP_GAUSSIAN_STD, out=out)
        return out

    # every library call of the new route, timed in each of the rounds
    calls, real = {}, _capi.call
    pending = []

    def timed_call(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(name, *a)
        e1.record()
        pending.append((name, e0, e1))

    def collect():
        for name, e0, e1 in pending:
            calls.setdefault(name, []).append(e0.elapsed_time(e1))
        del pending[:]

    seed[0] = 0
    t_torch = timed(torch_route)
    seed[0] = 0
    t_new = timed(new_route)
    fe.check()
    seed[0] = 0
    _capi.call = timed_call
    try:
        timed(new_route, per_call=collect)
    finally:
        _capi.call = real
    plane, rgb = B * D * D * 4.0, B * 3 * D * D * 4.0
    nbytes = {"hps_seg_bbox_affine": plane + B * (ta.PLAN_WORDS + 32 * 4 * 2 + 6 + 4 + 1 + 8) * 4.0,
              "hps_train_crop_augment": plane + 2 * rgb + rgb + B * (ta.PLAN_WORDS + 4 + 8) * 4.0,
              "hps_train_joints2d": B * (ta.PLAN_WORDS + 6 + 8 + 17 * (2 + 2 + 2 + 1) + 5) * 4.0}
    lines = ["The synthetic-data training front end on one MI355X (gfx950): B = %d images of 256 x 256 to a 256 x 256 crop, default" % B,
             "TRAIN.SYNTH_DATA.AUGMENT configuration, inputs of tests/train_frontend_scenario.py.  tests/dev/train_frontend_time.py: HIP events;",
             "median of %d rounds after %d warm-up rounds; a fresh plan (fresh random draws) every round on both routes." % (ROUNDS, WARMUP), "",
             "whole call, renderer output -> proxy_rep_input (host work included):",
             "  torch operations on the device (the reference's way)   %9.3f ms" % t_torch,
             "  SyntheticTrainFrontEnd (plan on the host + 5 launches) %9.3f ms   = 1 / %.1f of the torch route" % (t_new, t_torch / t_new), "",
             "library calls of one SyntheticTrainFrontEnd call, in order (event pair around each; the first includes the plan's upload",
             "queued in front of it):"]
    total = 0.0
    for name, v in calls.items():
        ms = med(v)
        total += ms
        if name in nbytes:
            nb = nbytes[name]
            lines.append("  %-26s %9.4f ms   %9.3f MB   %6.3f TB/s = %.4f of 8 TB/s"
                         % (name, ms, nb / 1e6, nb / (ms * 1e-3) / 1e12, nb / (ms * 1e-3) / HBM_PEAK))
        else:
            lines.append("  %-26s %9.4f ms" % (name, ms))
    lines.append("  %-26s %9.4f ms" % ("all library calls", total))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
