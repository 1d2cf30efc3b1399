"""Device time of the mask branch of detection.MaskRCNNBoxDetector, in tools/detector_time.py's configuration (batch 1, a 720 x 960
input, default sizes, 91 classes, seeded random weights filling the detection capacity).  Every round runs every route once, in turn
(the routes alternate), 3 warm-up and 20 timed rounds, median and quartiles in milliseconds:

  * the mask stages between device events: RoIAlign 14 into the haloed frames, the four 3x3 layers, hps_det_mask_predict, the paste;
  * ``forward()`` and ``forward(masks=True)`` (float and uint8), each with its synchronisation (a host clock round the call);
  * the fused predictor against its composition from existing kernels, built here only: four 1x1 hps_conv2d_bn_act_c16 problems (one
    per tap) that write the (K, 28, 28, 256) tensor, one 1x1 problem for all classes, a torch gather and sigmoid;
  * the paste's achieved bytes per second against the 8 TB/s HBM figure of DESIGN.md.

    python tools/detector_mask_time.py [--height 720 --width 960 --rounds 20 --warmup 3] [--out profiles/detector_mask_time.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import detector_scenario as S
    from hierarchicalprobabilistic3dhuman_amd import _capi, detection
    dev = torch.device("cuda", torch.cuda.current_device())
    det = detection.maskrcnn_resnet50_fpn()
    det.load_state_dict(S.make_weights(args.seed, 91), strict=True)
    det = det.to(dev).eval()
    H, W = args.height, args.width
    images = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(args.seed)).to(dev)]
    prep = det.prepare()
    NC, C = det.num_classes, _capi.DET_MASK_CHANNELS

    # the composition's layers, from the module's own parameters
    mp = det.roi_heads.mask_predictor
    taps = [detection._Layer16(mp.conv5_mask.weight.detach()[:, :, dy, dx].t().contiguous()[:, :, None, None], mp.conv5_mask.bias)
            for dy in range(2) for dx in range(2)]
    classes = detection._Layer16(mp.mask_fcn_logits.weight, mp.mask_fcn_logits.bias)

    stages = ("roi_align 14", "four 3x3 layers", "mask_predict", "paste float32", "paste uint8", "composition", "forward()",
              "forward(masks)", "forward(masks, uint8)")
    times = {s: [] for s in stages}
    note = {}
    for rnd in range(args.warmup + args.rounds):
        feats = det.features(images)
        props = det.proposals(feats)
        d = det.detections(feats, props, det.box_head(feats, props), with_rois=True)
        B, D, _ = d["roi_boxes"].shape
        K = B * D
        plan = det._mask_plan(prep, K, dev)
        levels = [(frame, 1, 1.0 / (4 << l)) for l, frame in enumerate(feats["P"])]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        ev[0].record()
        roi = detection.multiscale_roi_align(levels, d["roi_boxes"], d["roi_scores"], bins=_capi.DET_MASK_BINS, halo=1)
        ev[1].record()
        plan["roi"].copy_(roi)
        ev[2].record()
        _capi.run_enc_ops(plan["ops"], 0, len(plan["ops"]))
        ev[3].record()
        probs, logits = detection.mask_predict(plan["features"], prep["mask_wd"], prep["mask_bd"], prep["mask_wl"], prep["mask_bl"],
                                               d["labels"].view(K), d["roi_scores"].view(K), with_logits=True)
        ev[4].record()
        pasted = detection.paste_masks(probs, d["boxes"].view(K, 4), (H, W))
        ev[5].record()
        bits = detection.paste_masks(probs, d["boxes"].view(K, 4), (H, W), threshold=0.5)
        ev[6].record()
        # the composition: (4, K, 14, 14, 256) is the (K, 28, 28, 256) tensor in tap-major order
        up = torch.empty(4, K, 14, 14, C, device=dev)
        every = torch.empty(4 * K, 14, 14, NC, device=dev)
        ops = detection._conv_ops([taps[t].problem(plan["features"], K, 14, 14, 1, up[t], 0, True) for t in range(4)])
        ops += detection._conv_ops([classes.problem(up.view(4 * K, 14, 14, C), 4 * K, 14, 14, 0, every, 0, False)])
        ops = (_capi.HrnetOp * len(ops))(*ops)
        lab = d["labels"].view(1, K, 1, 1, 1).expand(4, K, 14, 14, 1)
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        detection._run(ops)
        picked = every.view(4, K, 14, 14, NC).gather(4, lab)[..., 0]
        comp_logits = picked.view(2, 2, K, 14, 14).permute(2, 3, 0, 4, 1).reshape(K, 28, 28)
        comp_probs = torch.sigmoid(comp_logits)
        c1.record()
        torch.cuda.synchronize()
        host = {}
        for name, kw in (("forward()", {}), ("forward(masks)", {"masks": True}), ("forward(masks, uint8)", {"masks": True, "mask_threshold": 0.5})):
            t0 = time.perf_counter()
            res = det(images, **kw)
            torch.cuda.synchronize()
            host[name] = (time.perf_counter() - t0) * 1e3
        if rnd < args.warmup:
            continue
        for k, s in enumerate(("roi_align 14", None, "four 3x3 layers", "mask_predict", "paste float32", "paste uint8")):
            if s:
                times[s].append(ev[k].elapsed_time(ev[k + 1]))
        times["composition"].append(c0.elapsed_time(c1))
        for name, v in host.items():
            times[name].append(v)
        present = d["roi_scores"].view(K) > float("-inf")
        note = {"detections": [len(r["scores"]) for r in res], "frame": feats["frame"], "sizes": feats["sizes"], "K": K,
                "composition_logit_diff": float((comp_logits - logits)[present].abs().max()), "logit_max": float(logits.abs().max()),
                "composition_prob_diff": float((comp_probs - probs)[present].abs().max()),
                "mask_pixels": float((bits != 0).sum()) / bits.numel(), "bytes_f32": pasted.numel() * 4, "bytes_u8": bits.numel()}
    q = lambda v: torch.quantile(torch.tensor(v, dtype=torch.float64), torch.tensor([0.25, 0.5, 0.75], dtype=torch.float64)).tolist()
    lines = ["MaskRCNNBoxDetector mask branch  batch 1  input %d x %d  frame %s  resized %s" % (H, W, note["frame"], note["sizes"]),
             "detections per image %s (K = %d mask rows)  share of pixels above 0.5: %.4f" % (note["detections"], note["K"], note["mask_pixels"]),
             "%-24s %10s %10s %10s   (ms over %d rounds after %d warm-up; every round runs every route once)"
             % ("route", "q1", "median", "q3", args.rounds, args.warmup)]
    med = {}
    for s in stages:
        a = q(times[s])
        med[s] = a[1]
        lines.append("%-24s %10.3f %10.3f %10.3f" % (s, a[0], a[1], a[2]))
    lines.append("forward() and forward(masks...) are host-clock times round the call and its synchronisation; the rest are device events")
    lines.append("fused predictor %.3f ms against its composition %.3f ms (ratio %.2f); max |composition - fused| logits %.3e (max |logit| %.3e), "
                 "probabilities %.3e" % (med["mask_predict"], med["composition"], med["composition"] / med["mask_predict"],
                                         note["composition_logit_diff"], note["logit_max"], note["composition_prob_diff"]))
    for s, nbytes in (("paste float32", note["bytes_f32"]), ("paste uint8", note["bytes_u8"])):
        rate = nbytes / (med[s] * 1e-3)
        lines.append("%s writes %.1f MB: %.2f TB/s = %.2f of the 8 TB/s HBM figure" % (s, nbytes / 1e6, rate / 1e12, rate / HBM_BYTES_PER_S))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
