"""Per-stage device time of detection.MaskRCNNBoxDetector: device events around each public stage, 3 warm-up and 20 timed calls,
median and quartiles in milliseconds.  Default: batch 1, a 720 x 960 input, default sizes, 91 classes, seeded random weights (the
time does not depend on the weights except through how many boxes survive the filters; the counts are printed).

    python tools/detector_time.py [--height 720 --width 960 --batch 1 --calls 20 --warmup 3]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    import detector_scenario as S
    from hierarchicalprobabilistic3dhuman_amd import detection
    dev = torch.device("cuda", torch.cuda.current_device())
    det = detection.maskrcnn_resnet50_fpn()
    det.load_state_dict(S.make_weights(args.seed, 91), strict=True)
    det = det.to(dev).eval()
    g = torch.Generator().manual_seed(args.seed)
    images = [torch.rand(3, args.height, args.width, generator=g).to(dev) for _ in range(args.batch)]
    stages = ("features", "proposals", "box_head", "detections", "forward")
    times = {s: [] for s in stages}
    counts = None
    for call in range(args.warmup + args.calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        feats = det.features(images)
        ev[1].record()
        props = det.proposals(feats)
        ev[2].record()
        head = det.box_head(feats, props)
        ev[3].record()
        out = det.detections(feats, props, head)
        ev[4].record()
        torch.cuda.synchronize()
        if call >= args.warmup:
            for k, s in enumerate(stages[:4]):
                times[s].append(ev[k].elapsed_time(ev[k + 1]))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = det(images)
            b.record()
            torch.cuda.synchronize()
            times["forward"].append(a.elapsed_time(b))
            counts = ([int((props["scores"][i] > float("-inf")).sum()) for i in range(args.batch)], [len(r["scores"]) for r in res])
    print("MaskRCNNBoxDetector  batch %d  input %d x %d  frame %s  resized %s" % (args.batch, args.height, args.width, feats["frame"], feats["sizes"]))
    print("proposals per image %s  detections per image %s" % counts)
    print("%-12s %10s %10s %10s   (ms over %d calls after %d warm-up)" % ("stage", "q1", "median", "q3", args.calls, args.warmup))
    for s in stages:
        q = torch.quantile(torch.tensor(times[s], dtype=torch.float64), torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)).tolist()
        print("%-12s %10.3f %10.3f %10.3f" % (s, q[0], q[1], q[2]))


if __name__ == "__main__":
    main()
