"""The mask branch of detection.MaskRCNNBoxDetector on the device against tests/detector_mask_scenario.py (float64, CPU), stage by stage
as tests/test_gpu_detector.py does it: every comparison feeds the oracle stage THE DEVICE'S OWN fp32 inputs to that stage.  Values follow
the project's rule  err <= 4 max(e_cpu32, 2^-23 max|y64|)  with e_cpu32 from the same scenario code on float32 tensors; decisions (the
integer paste rectangles, which pixels are written, the thresholded bytes) are equal.  The committed scenario's preconditions are
checked without a GPU in tests/test_detector_mask_scenario_host.py; all of its detections map to level 0, hence the kernel-alone
RoIAlign test on all four levels.

Measured on an MI355X (worst err / bound per family, as the tests printed them; measured values, not limits):
    haloed roi_align kernel alone 0.250 (14 bins, halo 1; the 7-bin call through either entry point 0.254, as before)
    mask roi 0.250   mask head 0.302   mask logits 0.155   mask probabilities 0.280          (the scenario's 2 x 10 detections)
    mask_predict alone: logits 0.126 / 0.165 / 0.158 / 0.152, probabilities 0.243 / 0.204 / 0.199 / 0.219   (K 1, 3, 10 at 3 classes; K 10 at 91)
    paste alone 0.250 (23 x 31), 0.062 (1 x 1)   pasted masks of the composition 0.250
"""
import ctypes

import pytest
import torch

import detector_mask_scenario as M
import detector_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, detection

pytestmark = pytest.mark.gpu

CFG = S.config(**S.TINY)
FILL = 7.0


def _check(name, got, y64, y32, floor=None):
    """The rule on a whole tensor; ``floor``: the magnitude 2^-23 multiplies when it is not the tensor's own."""
    y64, y32, got = y64.double(), y32.double(), got.detach().cpu().double()
    assert got.shape == y64.shape, (name, got.shape, y64.shape)
    scale = float(y64.abs().max()) if floor is None else float(floor)
    e32 = float((y32 - y64).abs().max()) if y64.numel() else 0.0
    bound = S.rule(e32, scale)
    err = float((got - y64).abs().max()) if y64.numel() else 0.0
    print("%-34s max|dev - f64| = %.3e  e_cpu32 = %.3e  scale %.3e  err/bound = %.3f" % (name, err, e32, scale, err / bound))
    assert err == err and err <= bound, (name, err, bound)
    return err / bound


def _interior(frames):
    """(K, 16, 16, C) zero-haloed NHWC frames -> (K, C, 14, 14) on the CPU."""
    return frames[:, 1:-1, 1:-1].permute(0, 3, 1, 2).contiguous().cpu()


def _halo_is_zero(frames):
    f = frames.cpu().clone()
    f[:, 1:-1, 1:-1] = 0
    return float(f.abs().max()) == 0.0


@pytest.fixture(scope="module")
def world(dev):
    """The TINY detector with the committed seed's weights and one pass through the stages, mask branch included, with copies of what
    the tests read (the module's frames are overwritten by the next call)."""
    ims, sd = S.scenario_inputs(S.SEED)
    det = detection.maskrcnn_resnet50_fpn(**S.TINY)
    det.load_state_dict(sd, strict=True)
    det = det.to(dev).eval()
    dims = [im.to(dev) for im in ims]
    feats = det.features(dims)
    props = det.proposals(feats)
    dets = det.detections(feats, props, det.box_head(feats, props), with_rois=True)
    mask = det.mask_branch(feats, dets)
    torch.cuda.synchronize()
    return {"det": det, "ims": ims, "dims": dims, "sd": sd, "sd64": S.cast(sd, torch.float64), "P": [t.clone() for t in feats["P"]],
            "sizes": feats["sizes"], "frame": feats["frame"], "dets": {k: (v.clone() if torch.is_tensor(v) else v) for k, v in dets.items()},
            "mask": {k: v.clone() for k, v in mask.items()}}


def _roi_case(dev):
    """The geometry of test_gpu_detector.test_roi_align_kernel_alone: boxes on all four levels, one smaller than a bin, one on the
    right and bottom edges, one reaching outside, one absent row."""
    g = torch.Generator().manual_seed(9)
    B, C, F0 = 2, 12, 512
    maps = [torch.randn(B, C, F0 >> (2 + l), F0 >> (2 + l), generator=g) * (1.0 + l) for l in range(4)]
    boxes = torch.tensor([[[100.0, 120.0, 102.0, 121.5], [400.0, 380.0, 512.0, 512.0], [10.0, 20.0, 300.0, 330.0], [0.0, 0.0, 512.0, 500.0],
                           [30.25, 41.5, 77.0, 99.75], [-20.0, 480.0, 90.0, 540.0]],
                          [[5.0, 5.0, 6.0, 40.0], [256.0, 0.0, 512.0, 120.0], [3.5, 200.0, 260.0, 512.0], [12.0, 8.0, 500.0, 509.0],
                           [200.0, 210.0, 215.0, 222.0], [440.0, 300.0, 512.0, 512.0]]])
    lv, margin = S.level_of(boxes.reshape(-1, 4).double())
    assert margin >= 1e-3 and sorted(set(lv.tolist())) == [0, 1, 2, 3]
    frames = []
    for l, m in enumerate(maps):
        fr = torch.full((B, m.shape[2] + 2, m.shape[3] + 2, C), FILL)
        fr[:, 1:-1, 1:-1] = m.permute(0, 2, 3, 1)
        frames.append((fr.to(dev), 1, 1.0 / (4 << l)))
    scores = torch.zeros(B, 6)
    scores[1, 4] = float("-inf")
    return maps, boxes, frames, scores


def test_haloed_roi_align_kernel_alone(dev):
    maps, boxes, frames, scores = _roi_case(dev)
    B, C = 2, 12
    got = detection.multiscale_roi_align(frames, boxes.to(dev), scores.to(dev), bins=14, halo=1)
    assert tuple(got.shape) == (B * 6, 16, 16, C) and _halo_is_zero(got)
    assert float(got[6 + 4].abs().max()) == 0.0                                      # the absent row: a whole frame of zeros
    flat = detection.multiscale_roi_align(frames, boxes.to(dev), scores.to(dev), bins=14)
    assert tuple(flat.shape) == (B, 6, 14 * 14 * C) and torch.equal(flat.view(B * 6, 14, 14, C), got[:, 1:-1, 1:-1])
    inner = _interior(got).reshape(B, 6, C, 14, 14)
    top = max(float(m.abs().max()) for m in maps)
    worst = 0.0
    for b in range(B):
        want64 = S.roi_align([m[b].double() for m in maps], boxes[b].double(), bins=14)
        want32 = S.roi_align([m[b] for m in maps], boxes[b], bins=14)
        rows = [r for r in range(6) if (b, r) != (1, 4)]
        worst = max(worst, _check("haloed roi_align image %d" % b, inner[b][rows], want64[rows], want32[rows], floor=top))
    print("worst err/bound  detector haloed roi_align  %.3f" % worst)
    # 7 bins without a halo: the bits of the existing entry point, called directly
    seven = detection.multiscale_roi_align(frames, boxes.to(dev), scores.to(dev), bins=7, halo=0)
    bd, sc = boxes.to(dev).contiguous(), scores.to(dev).contiguous()
    outs = []
    for entry in ("hps_det_roi_align", "hps_det_roi_align_halo"):
        y = torch.full((B, 6, 49 * C), FILL, device=dev)
        a = _capi.DetRoiAlignArgs(struct_bytes=ctypes.sizeof(_capi.DetRoiAlignArgs), B=B, R=6, C=C, bins=7, n_levels=4, boxes=_capi.ptr(bd),
                                  scores=_capi.ptr(sc), y=_capi.ptr(y))
        for l, (frame, pad, scale) in enumerate(frames):
            lv = a.level[l]
            lv.x, lv.h, lv.w, lv.pad, lv.scale = _capi.ptr(frame), frame.shape[1] - 2, frame.shape[2] - 2, pad, scale
        _capi.call(entry, *([ctypes.byref(a), _capi.stream()] if entry == "hps_det_roi_align" else [ctypes.byref(a), 0, _capi.stream()]))
        outs.append(y)
    assert torch.equal(outs[0], seven) and torch.equal(outs[1], seven)
    want64 = S.roi_align([m[0].double() for m in maps], boxes[0].double())
    want32 = S.roi_align([m[0] for m in maps], boxes[0])
    _check("roi_align 7 bins image 0", seven[0].cpu().reshape(6, 7, 7, C).permute(0, 3, 1, 2), want64, want32, floor=top)


def test_mask_rois_and_head(world):
    d, m = world["dets"], world["mask"]
    B, D = d["labels"].shape
    worst = 0.0
    assert tuple(m["roi"].shape) == (B * D, 16, 16, 256) and tuple(m["features"].shape) == (B * D, 16, 16, 256)
    assert _halo_is_zero(m["roi"]) and _halo_is_zero(m["features"])
    counts = d["counts"].tolist()
    assert counts == [10, 10]                                                        # the scenario's 2 x 10 detections
    roi, feats = _interior(m["roi"]).reshape(B, D, 256, 14, 14), _interior(m["features"]).reshape(B, D, 256, 14, 14)
    for b in range(B):
        n = counts[b]
        present = d["roi_scores"][b].cpu() > float("-inf")
        assert present.tolist() == [True] * n + [False] * (D - n)
        rois = d["roi_boxes"][b, :n].cpu()
        # the RoIs are the gathered candidates before the rescale: the rescale of them is the detections' boxes, bit for bit
        oh, ow = world["ims"][b].shape[1:]
        rh, rw = world["sizes"][b]
        ratio = torch.stack([torch.tensor(float(ow)) / torch.tensor(float(rw)), torch.tensor(float(oh)) / torch.tensor(float(rh))] * 2)
        assert torch.equal(rois * ratio, d["boxes"][b, :n].cpu())
        order, top = d["order"][b].cpu(), torch.nonzero(d["keep_scores"][b].cpu() > float("-inf"))
        kept = {(int(c) + 1, int(order[c, q])) for c, q in top.tolist()}
        cb = d["cand_boxes"][b].cpu()
        for k in range(n):
            c = int(d["labels"][b, k])
            assert any(torch.equal(cb[c - 1, r], rois[k]) for cc, r in kept if cc == c), (b, k)
        Pd = [t[b, 1:-1, 1:-1].permute(2, 0, 1).contiguous().cpu() for t in world["P"]]
        _, margin = S.level_of(rois.double())
        assert margin >= 1e-4, "precondition: a detection sits on a level boundary"
        r64, r32 = S.roi_align([p.double() for p in Pd], rois.double(), bins=14), S.roi_align(Pd, rois, bins=14)
        worst = max(worst, _check("mask roi image %d" % b, roi[b, :n], r64, r32, floor=max(float(p.abs().max()) for p in Pd)))
        assert float(roi[b, n:].abs().sum()) == 0.0
        x = roi[b, :n].contiguous()
        worst = max(worst, _check("mask head image %d" % b, feats[b, :n], M.mask_head(x.double(), world["sd64"]), M.mask_head(x, world["sd"])))
        # the predictor on the device's own features
        lab = d["labels"][b, :n].cpu()
        f = feats[b, :n].contiguous()
        l64, l32 = M.mask_logits(f.double(), world["sd64"], lab), M.mask_logits(f, world["sd"], lab)
        worst = max(worst, _check("mask logits image %d" % b, m["logits"][b, :n], l64, l32))
        worst = max(worst, _check("mask probabilities image %d" % b, m["probs"][b, :n], torch.sigmoid(l64), torch.sigmoid(l32), floor=1.0))
        assert float(m["probs"][b, n:].abs().sum()) == 0.0 and float(m["logits"][b, n:].abs().sum()) == 0.0
    print("worst err/bound  detector mask rois + head + predictor  %.3f" % worst)


def _predict_case(K, NC, seed, dev):
    g = torch.Generator().manual_seed(seed)
    sd = {k: v for k, v in S.make_weights(seed, NC).items() if k.startswith("roi_heads.mask_predictor.")}
    sd["roi_heads.mask_predictor.mask_fcn_logits.weight"] = sd["roi_heads.mask_predictor.mask_fcn_logits.weight"] * 3.0
    x = torch.relu(torch.randn(K, 256, 14, 14, generator=g))                         # what a ReLU layer hands over
    frames = torch.full((K, 16, 16, 256), FILL)                                      # the halo is never read
    frames[:, 1:-1, 1:-1] = x.permute(0, 2, 3, 1)
    return sd, x, frames.to(dev)


def _predict(sd, frames, labels, scores, dev):
    p = "roi_heads.mask_predictor."
    NC = sd[p + "mask_fcn_logits.weight"].shape[0]
    return detection.mask_predict(frames, detection.mask_weights(sd[p + "conv5_mask.weight"]).to(dev), sd[p + "conv5_mask.bias"].to(dev),
                                  sd[p + "mask_fcn_logits.weight"].reshape(NC, 256).contiguous().to(dev), sd[p + "mask_fcn_logits.bias"].to(dev),
                                  labels.to(dev), None if scores is None else scores.to(dev), with_logits=True)


@pytest.mark.parametrize("K,NC", [(1, 3), (3, 3), (10, 3), (10, 91)])
def test_mask_predict_kernel_alone(K, NC, dev):
    sd, x, frames = _predict_case(K, NC, 11, dev)
    scores = None
    if K == 10:
        labels = torch.tensor([1, 2, 1, 2, 0, 1, 2, 1, 2, 1]) if NC == 3 else torch.tensor([1, 90, 45, 2, 0, 17, 64, 33, 89, 5])
        scores = torch.zeros(K)
        scores[8] = float("-inf")                                                    # an absent row; row 4 has label 0
        live = [k for k in range(K) if k not in (4, 8)]
    else:
        labels = torch.tensor([1, 2, 2][:K]) if K == 3 else torch.tensor([2])
        live = list(range(K))
    probs, logits = _predict(sd, frames, labels, scores, dev)
    assert tuple(probs.shape) == (K, 28, 28) and tuple(logits.shape) == (K, 28, 28)
    for k in range(K):
        if k not in live:
            assert float(probs[k].abs().max()) == 0.0 and float(logits[k].abs().max()) == 0.0, k
    sd64 = S.cast(sd, torch.float64)
    xs, ls = x[live].contiguous(), labels[live]
    l64, l32 = M.mask_logits(xs.double(), sd64, ls), M.mask_logits(xs, sd, ls)
    frac = float((l64 > 0).double().mean())
    assert 0.05 < frac < 0.95, "precondition: logits of both signs (%.3f positive)" % frac
    worst = _check("mask_predict logits K %d NC %d" % (K, NC), logits[live], l64, l32)
    worst = max(worst, _check("mask_predict probs K %d NC %d" % (K, NC), probs[live], torch.sigmoid(l64), torch.sigmoid(l32), floor=1.0))
    print("worst err/bound  detector mask_predict  %.3f" % worst)
    if K == 10:
        # a detection's bits alone (K = 1) and as row 7 of 10; a second run has the same bits
        p1, l1 = _predict(sd, frames[7:8].contiguous(), labels[7:8], None, dev)
        assert torch.equal(p1[0], probs[7]) and torch.equal(l1[0], logits[7])
        p2, l2 = _predict(sd, frames, labels, scores, dev)
        assert torch.equal(p2, probs) and torch.equal(l2, logits)
        no_logits = detection.mask_predict(frames, *[t for t in _weights(sd, dev)], labels.to(dev), scores.to(dev))
        assert no_logits[1] is None and torch.equal(no_logits[0], probs)


def _weights(sd, dev):
    p = "roi_heads.mask_predictor."
    NC = sd[p + "mask_fcn_logits.weight"].shape[0]
    return (detection.mask_weights(sd[p + "conv5_mask.weight"]).to(dev), sd[p + "conv5_mask.bias"].to(dev),
            sd[p + "mask_fcn_logits.weight"].reshape(NC, 256).contiguous().to(dev), sd[p + "mask_fcn_logits.bias"].to(dev))


@pytest.mark.parametrize("H,W", M.PASTE_SIZES)
def test_paste_masks_kernel_alone(H, W, dev):
    names, boxes = M.paste_boxes(H, W)
    n = len(names)
    probs = 0.05 + 0.9 * torch.rand(n, 28, 28, generator=torch.Generator().manual_seed(5))        # strictly positive
    got = detection.paste_masks(probs.to(dev), boxes.to(dev), (H, W))
    assert tuple(got.shape) == (n, 1, H, W) and got.dtype == torch.float32
    got = got[:, 0].cpu()
    ib = M.expand_and_truncate(boxes)
    k = names.index("truncation")
    assert int(ib[k, 0]) == 0 and int(ib[k, 1]) == 0
    want64, want32 = M.paste(probs.double(), ib, H, W), M.paste(probs, ib, H, W)
    for k, name in enumerate(names):
        (xa, xb), (ya, yb) = M.rectangle(ib[k], H, W)
        rect = torch.zeros(H, W, dtype=torch.bool)
        if xa < xb and ya < yb:
            rect[ya:yb, xa:xb] = True
        written = got[k] != 0
        # written pixels are those of the reference; a box wider than 30 pixels samples the ring of zeros exactly at its first pixel
        assert torch.equal(written, want64[k] != 0) and not bool((written & ~rect).any()), name
        if int(ib[k, 2]) - int(ib[k, 0]) + 1 <= 30 and int(ib[k, 3]) - int(ib[k, 1]) + 1 <= 30:
            assert torch.equal(written, rect), name
    if (H, W) == (23, 31):
        count = {name: int((got[k] != 0).sum()) for k, name in enumerate(names)}
        assert count["outside"] == 0 and count["zero"] == 1 and count["inside"] > 0
    worst = _check("paste %d x %d" % (H, W), got, want64, want32, floor=1.0)
    print("worst err/bound  detector paste  %.3f" % worst)
    for thr in (0.5, 0.25):
        bits = detection.paste_masks(probs.to(dev), boxes.to(dev), (H, W), threshold=thr)
        assert bits.dtype == torch.uint8 and tuple(bits.shape) == (n, 1, H, W)
        assert torch.equal(bits[:, 0].cpu(), (got > thr).to(torch.uint8)), thr
    assert torch.equal(detection.paste_masks(probs[:, None].to(dev), boxes.to(dev), (H, W))[:, 0].cpu(), got)
    assert tuple(detection.paste_masks(probs[:0].to(dev), boxes[:0].to(dev), (H, W)).shape) == (0, 1, H, W)


def test_composition(world, dev):
    det, dims, ims = world["det"], world["dims"], world["ims"]
    plain = det(dims)
    out = det(dims, masks=True)
    binary = det(dims, masks=True, mask_threshold=0.5)
    feats = det.features(dims)
    props = det.proposals(feats)
    d = det.detections(feats, props, det.box_head(feats, props), with_rois=True)
    probs = det.mask_branch(feats, d)["probs"].clone()
    counts = d["counts"].tolist()
    worst = 0.0
    for b in range(2):
        n = counts[b]
        H, W = ims[b].shape[1:]
        assert set(plain[b]) == {"boxes", "labels", "scores"} and set(out[b]) == {"boxes", "labels", "scores", "masks"}
        assert all(torch.equal(out[b][k], plain[b][k]) for k in ("boxes", "labels", "scores"))
        assert tuple(out[b]["masks"].shape) == (n, 1, H, W) and out[b]["masks"].dtype == torch.float32
        assert torch.equal(out[b]["masks"], detection.paste_masks(probs[b, :n], d["boxes"][b, :n], (H, W)))
        assert torch.equal(probs[b, :n], world["mask"]["probs"][b, :n])
        # the paste of the device's own probabilities into the device's own boxes
        ib = M.expand_and_truncate(out[b]["boxes"].cpu())
        p = probs[b, :n].cpu()
        worst = max(worst, _check("pasted masks image %d" % b, out[b]["masks"][:, 0], M.paste(p.double(), ib, H, W), M.paste(p, ib, H, W), floor=1.0))
        assert binary[b]["masks"].dtype == torch.uint8 and torch.equal(binary[b]["masks"], (out[b]["masks"] > 0.5).to(torch.uint8))
    print("worst err/bound  detector pasted masks  %.3f" % worst)
    pb, pl, ps, pc, pm = det.detect_padded(dims, masks=True)
    assert tuple(pm.shape) == (2, 10, 28, 28) and pc.tolist() == counts and torch.equal(pm, probs)
    four = det.detect_padded(dims)
    assert len(four) == 4 and torch.equal(four[0], pb) and torch.equal(four[1], pl) and torch.equal(four[2], ps)
    # rows past each count are zero: one image of the batch alone has fewer rows than the capacity only if the count is below it; a
    # detector with more capacity than detections shows it
    wide = detection.maskrcnn_resnet50_fpn(**dict(S.TINY, box_detections_per_img=40))
    wide.load_state_dict(world["sd"], strict=True)
    wide = wide.to(dev).eval()
    wb, wl, ws, wc, wm = wide.detect_padded(dims, masks=True)
    for b, n in enumerate(wc.tolist()):
        assert n < 40 and float(wm[b, n:].abs().sum()) == 0.0 and float(wm[b, :n].abs().sum()) > 0.0, (b, n)
    # an image alone in the batch's frame has the same mask bits
    for b in range(2):
        one = det([dims[b]], frame=world["frame"], masks=True)
        assert torch.equal(one[0]["masks"], out[b]["masks"]) and torch.equal(one[0]["boxes"], out[b]["boxes"]), b
