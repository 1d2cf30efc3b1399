"""detection.MaskRCNNBoxDetector on the device against tests/detector_scenario.py (float64, CPU), stage by stage: every comparison feeds
the oracle stage THE DEVICE'S OWN fp32 inputs to that stage, so a decision flipped upstream cannot pass for an error downstream.
Values follow the project's rule  err <= 4 max(e_cpu32, 2^-23 max|y64|)  with e_cpu32 from the same scenario code on float32 tensors;
decisions (top-k sets, kept sets, labels) are equal.  The end-to-end test asserts its preconditions on the CPU first (the oracle alone
returns >= 3 detections per image, every margin of the chain is >= 8 bounds; tests/test_detector_scenario_host.py checks the committed
seed without a GPU) and fails, never skips, when they do not hold.

"The same bits one image at a time": the batch frame's zero region is input to the convolutions (as in torchvision, where a batch's
padding shows in every image's features), so an image alone in its own smaller frame is another computation; the images are run one at
a time IN THE BATCH'S FRAME (``frame=``), where the bits are equal.  The transform's own output has the same bits in either frame.

Measured on an MI355X (worst err / bound per family, as the tests printed them; measured values, not limits):
    transform 0.250   C2 0.196   C3 0.234   C4 0.385   C5 0.358   P2 0.273   P3 0.305   P4 0.315   P5 0.368   pool 0.328
    rpn boxes 0.250 (per image and level 0.000 .. 0.250)          roi_align kernel alone 0.254
    roi 0.250   class logits 0.363   box deltas 0.611   probabilities 0.140   class boxes 0.240   detection boxes 0.204, scores 0.140
    end to end: boxes 0.390, scores 0.444 (10 detections per image)
With every layer summed over K in one run (hps_conv2d_bn_act_c16, or the wide kernel without K slices) P2 stood at 1.056 and 1.191 of
the bound: the 3x3 layers sum 2 304 products, and a float32 chain of that length is four times less accurate than the CPU's blocked
sums.  The wide layers now sum K in slices of 256 products (detection._wide_layer).
"""
import pytest
import torch

import detector_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, detection

pytestmark = pytest.mark.gpu

CFG = S.config(**S.TINY)
FILL = 7.0


def _check(name, got, y64, y32, floor=None):
    """The rule on a whole tensor; ``floor``: the magnitude 2^-23 multiplies when it is not the tensor's own (boxes: the image size)."""
    y64, y32, got = y64.double(), y32.double(), got.detach().cpu().double()
    assert got.shape == y64.shape, (name, got.shape, y64.shape)
    scale = float(y64.abs().max()) if floor is None else float(floor)
    e32 = float((y32 - y64).abs().max()) if y64.numel() else 0.0
    bound = S.rule(e32, scale)
    err = float((got - y64).abs().max()) if y64.numel() else 0.0
    print("%-34s max|dev - f64| = %.3e  e_cpu32 = %.3e  scale %.3e  err/bound = %.3f" % (name, err, e32, scale, err / bound))
    assert err == err and err <= bound, (name, err, bound)
    return err / bound


def _nchw(frame, pad=1):
    """The interior of a zero-haloed NHWC frame as an NCHW CPU tensor."""
    f = frame[:, pad:frame.shape[1] - pad, pad:frame.shape[2] - pad] if pad else frame
    return f.permute(0, 3, 1, 2).contiguous().cpu()


def _halo_is_zero(frame, pad):
    f = frame.cpu()
    inner = torch.zeros_like(f, dtype=torch.bool)
    inner[:, pad:f.shape[1] - pad, pad:f.shape[2] - pad] = True
    return float(f[~inner].abs().max()) == 0.0


@pytest.fixture(scope="module")
def world(dev):
    """The TINY detector with the committed seed's weights, the two images, and one pass through the stages with copies of everything
    the tests read (the module's frames are overwritten by the next call)."""
    ims, sd = S.scenario_inputs(S.SEED)
    det = detection.maskrcnn_resnet50_fpn(**S.TINY)
    det.load_state_dict(sd, strict=True)
    det = det.to(dev).eval()
    dims = [im.to(dev) for im in ims]
    feats = det.features(dims)
    snap = {"input": feats["input"].clone(), "C": [t.clone() for t in feats["C"]], "P": [t.clone() for t in feats["P"]],
            "pool": feats["pool"].clone(), "sizes": feats["sizes"], "frame": feats["frame"]}
    props = det.proposals(feats)
    psnap = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in props.items() if k not in ("logits", "deltas", "top")}
    psnap["logits"], psnap["deltas"] = [t.clone() for t in props["logits"]], [t.clone() for t in props["deltas"]]
    psnap["top"] = [(v.clone(), i.clone()) for v, i in props["top"]]
    head = det.box_head(feats, props)
    hsnap = {k: v.clone() for k, v in head.items()}
    dets = det.detections(feats, props, head, with_probs=True)
    torch.cuda.synchronize()
    return {"det": det, "ims": ims, "dims": dims, "sd": sd, "sd64": S.cast(sd, torch.float64), "feats": snap, "props": psnap, "head": hsnap,
            "dets": dets}


def test_transform_and_features(world, dev):
    det, ims, f = world["det"], world["ims"], world["feats"]
    assert f["sizes"] == [(86, 64), (57, 96)] and f["frame"] == (96, 96)                    # two sizes, one frame
    worst = 0.0
    b64, _ = S.transform([im.double() for im in ims], CFG)
    b32, _ = S.transform(ims, CFG)
    x = f["input"]
    assert tuple(x.shape) == (2, 102, 102, 4) and _halo_is_zero(x, 3) and float(x[..., 3].abs().max()) == 0.0
    got = _nchw(x, 3)[:, :3]
    worst = max(worst, _check("transform", got, b64, b32))
    assert float(got[0, :, 86:].abs().max()) == 0.0 and float(got[0, :, :, 64:].abs().max()) == 0.0 and float(got[1, :, 57:].abs().max()) == 0.0
    # backbone on the device's own input, FPN on the device's own C2..C5
    C64, C32 = S.backbone(got.double(), world["sd64"], CFG), S.backbone(got, world["sd"], CFG)
    for k in range(4):
        assert _halo_is_zero(f["C"][k], 1) and _halo_is_zero(f["P"][k], 1)
        worst = max(worst, _check("C%d" % (k + 2), _nchw(f["C"][k]), C64[k], C32[k]))
    Cd = [_nchw(t) for t in f["C"]]
    (P64, pool64), (P32, pool32) = S.fpn([c.double() for c in Cd], world["sd64"]), S.fpn(Cd, world["sd"])
    for k in range(4):
        worst = max(worst, _check("P%d" % (k + 2), _nchw(f["P"][k]), P64[k], P32[k]))
    assert tuple(f["pool"].shape) == (2, 4, 4, 256) and _halo_is_zero(f["pool"], 1)
    worst = max(worst, _check("pool", _nchw(f["pool"]), pool64, pool32))
    assert torch.equal(_nchw(f["pool"]), _nchw(f["P"][3])[:, :, ::2, ::2])
    print("worst err/bound  detector transform + features  %.3f" % worst)
    # an image's transform has the same bits alone (its own frame) and in the batch; its features the same bits alone in the batch's frame
    for b in range(2):
        alone = det.features([world["dims"][b]])
        oh, ow = f["sizes"][b]
        assert alone["frame"] == ((oh + 31) // 32 * 32, (ow + 31) // 32 * 32)
        assert torch.equal(alone["input"][0, 3:3 + oh, 3:3 + ow], x[b, 3:3 + oh, 3:3 + ow])
        same = det.features([world["dims"][b]], frame=(96, 96))
        assert torch.equal(same["input"][0], x[b])
        for k in range(4):
            assert torch.equal(same["C"][k][0], f["C"][k][b]) and torch.equal(same["P"][k][0], f["P"][k][b]), (b, k)
        assert torch.equal(same["pool"][0], f["pool"][b])


def test_rpn_decode_filter_and_nms(world):
    p, f = world["props"], world["feats"]
    FH, FW = f["frame"]
    worst = 0.0
    N = p["cand_scores"].shape[2]
    for b in range(2):
        size = f["sizes"][b]
        kept_boxes, kept_scores = [], []
        for l in range(5):
            lg, dl = p["logits"][l][b].cpu(), p["deltas"][l][b].cpu()
            h, w, _ = lg.shape
            k = min(CFG["rpn_pre_nms_top_n_test"], h * w * 3)
            out = []
            for dt in (torch.float64, torch.float32):
                anc = S.anchors(S.LEVEL_SIZES[l], h, w, FH // h, FW // w, dt)
                out.append(S.rpn_level(lg.to(dt).reshape(-1), dl.to(dt).reshape(-1, 4), anc, CFG["rpn_pre_nms_top_n_test"], size))
            (idx, bx64, valid, sc, m), (_, bx32, _, _, _) = out
            assert m["topk"] > 0 and torch.equal(p["top"][l][1][b].cpu(), idx), (b, l)                  # the same k candidates, in order
            cs = p["cand_scores"][b, l, :k].cpu()
            assert torch.equal(cs > float("-inf"), valid), (b, l)                                        # the same boxes survive the filter
            assert torch.equal(cs[valid].double(), sc[valid]) and bool((p["cand_scores"][b, l, k:] == float("-inf")).all())
            got = p["cand_boxes"][b, l, :k].cpu()
            assert float(got[~valid].abs().max() if (~valid).any() else 0.0) == 0.0
            worst = max(worst, _check("rpn boxes image %d level %d" % (b, l), got[valid], bx64[valid], bx32[valid], floor=max(size)))
            # NMS on the device's own candidates
            vb, vs = got[valid].double(), cs[valid].double()
            keep, margin = S.nms(vb, vs, CFG["rpn_nms_thresh"])
            assert margin >= 1e-5, "precondition: an IoU sits on the threshold"
            want = torch.zeros(N, dtype=torch.bool)
            want[torch.nonzero(valid)[:, 0][keep]] = True
            assert torch.equal(p["keep_scores"][b, l].cpu() > float("-inf"), want), (b, l)
            kept_boxes.append(vb[keep])
            kept_scores.append(vs[keep])
        kb, ks = torch.cat(kept_boxes), torch.cat(kept_scores)
        order = torch.argsort(ks, descending=True, stable=True)[:CFG["rpn_post_nms_top_n_test"]]
        n = order.numel()
        assert torch.equal(p["boxes"][b, :n].cpu().double(), kb[order]) and torch.equal(p["scores"][b, :n].cpu().double(), ks[order])
        assert bool((p["scores"][b, n:] == float("-inf")).all()) and float(p["boxes"][b, n:].abs().sum()) == 0.0
    print("worst err/bound  detector rpn boxes  %.3f" % worst)


def _nms_case(seed):
    """200 boxes on a quarter-pixel lattice in 3 categories of 0, 1 and 199 boxes, distinct scores; identical, nested and zero-area
    boxes among them."""
    g = torch.Generator().manual_seed(seed)
    n = 200
    xy = torch.randint(0, 160, (n, 2), generator=g).double() / 4
    wh = torch.randint(4, 120, (n, 2), generator=g).double() / 4
    boxes = torch.cat([xy, xy + wh], dim=1)
    boxes[10] = boxes[3]                                             # identical
    boxes[11] = boxes[3]
    boxes[20] = boxes[5] + torch.tensor([1.0, 1.0, -1.0, -1.0])      # nested
    boxes[21] = boxes[6] + torch.tensor([0.25, 0.5, -0.25, -0.5])
    boxes[30, 2] = boxes[30, 0]                                      # zero area: no width, no height, a point
    boxes[31, 3] = boxes[31, 1]
    boxes[32, 2:] = boxes[32, :2]
    boxes[33] = boxes[32]
    scores = (torch.randperm(n, generator=g).double() + 1) / (n + 1)
    cats = torch.full((n,), 2, dtype=torch.int64)
    cats[77] = 1
    return boxes, scores, cats


def test_nms_kernel_alone(dev):
    boxes, scores, cats = _nms_case(8)
    assert sorted(int((cats == c).sum()) for c in range(3)) == [0, 1, 199] and scores.unique().numel() == 200
    for thresh in (0.5, 0.7):
        keep, margin = S.nms_per_category(boxes, scores, cats, thresh)
        assert margin >= 1e-4, "precondition: every compared IoU at least 1e-4 from the threshold (fix the seed)"
        sel = torch.nonzero(cats == 2)[:, 0]
        assert sorted(keep) == sorted([int(sel[i]) for i in S.nms_brute(boxes[sel], scores[sel], thresh)] + [77])
        got = detection.nms_per_category(boxes.float().to(dev), scores.float().to(dev), cats.to(dev), 3, thresh)
        assert got.cpu().tolist() == keep, thresh
        assert 77 in keep and 1 < len(keep) < 200
    # one group of the capacity, every box apart: everything is kept; absent rows stay absent
    N = _capi.DET_NMS_MAX_BOXES
    far = torch.arange(N, dtype=torch.float32)[:, None] * torch.tensor([4.0, 0.0, 4.0, 0.0]) + torch.tensor([0.0, 0.0, 2.0, 2.0])
    sc = torch.linspace(1.0, 0.1, N)
    sc[5::9] = float("-inf")
    out = detection.nms_groups(far[None].to(dev).contiguous(), sc[None].to(dev).contiguous(), 0.5)
    assert torch.equal(out.cpu()[0], sc)


def test_roi_align_kernel_alone(dev):
    """Boxes on all four levels, one smaller than a bin (the max(., 1)), one on the image's right and bottom edges, one reaching outside."""
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
    scores[1, 4] = float("-inf")                                     # an absent row: zeros
    got = detection.multiscale_roi_align(frames, boxes.to(dev), scores.to(dev)).cpu().reshape(B, 6, 7, 7, C).permute(0, 1, 4, 2, 3)
    assert float(got[1, 4].abs().max()) == 0.0
    top = max(float(m.abs().max()) for m in maps)
    worst = 0.0
    for b in range(B):
        want64 = S.roi_align([m[b].double() for m in maps], boxes[b].double())
        want32 = S.roi_align([m[b] for m in maps], boxes[b])
        rows = [r for r in range(6) if (b, r) != (1, 4)]
        worst = max(worst, _check("roi_align image %d" % b, got[b][rows], want64[rows], want32[rows], floor=top))
    print("worst err/bound  detector roi_align  %.3f" % worst)


def test_box_head_and_detections(world):
    f, p, h, d = world["feats"], world["props"], world["head"], world["dets"]
    worst = 0.0
    NC, R = CFG["num_classes"], p["boxes"].shape[1]
    for b in range(2):
        size = f["sizes"][b]
        n = int((p["scores"][b] > float("-inf")).sum())
        props = p["boxes"][b, :n].cpu()
        # RoIAlign on the device's own P2..P5 and proposals
        Pd = [_nchw(t)[b] for t in f["P"]]
        _, margin = S.level_of(props.double())
        assert margin >= 1e-4, "precondition: a proposal sits on a level boundary"
        roi64, roi32 = S.roi_align([m.double() for m in Pd], props.double()), S.roi_align(Pd, props)
        got = h["roi"][b, :n].cpu().reshape(n, 7, 7, 256).permute(0, 3, 1, 2)
        worst = max(worst, _check("roi image %d" % b, got, roi64, roi32, floor=max(float(m.abs().max()) for m in Pd)))
        assert float(h["roi"][b, n:].abs().sum()) == 0.0
        # the box head on the device's own RoI features
        (lg64, dl64), (lg32, dl32) = S.box_head(got.double(), world["sd64"]), S.box_head(got.contiguous(), world["sd"])
        worst = max(worst, _check("class logits image %d" % b, h["logits"][b, :n], lg64, lg32))
        worst = max(worst, _check("box deltas image %d" % b, h["deltas"][b, :n], dl64, dl32))
        # soft-max, decode, filters, NMS and the cut on the device's own logits, deltas and proposals
        lg, dl = h["logits"][b, :n].cpu(), h["deltas"][b, :n].cpu()
        (pr64, cb64), (pr32, cb32) = S.class_candidates(lg.double(), dl.double(), props.double(), size), S.class_candidates(lg, dl, props, size)
        worst = max(worst, _check("probabilities image %d" % b, d["probs"][b, :n], pr64, pr32, floor=1.0))
        present = d["cand_scores"][b].cpu() > float("-inf")                                  # (NC - 1, R)
        ws, hs = cb64[:, 1:, 2] - cb64[:, 1:, 0], cb64[:, 1:, 3] - cb64[:, 1:, 1]
        want = ((pr64[:, 1:] > CFG["box_score_thresh"]) & (ws >= 1e-2) & (hs >= 1e-2)).t()
        assert torch.equal(present[:, :n], want) and not bool(present[:, n:].any()), b
        gotb = d["cand_boxes"][b, :, :n].cpu().permute(1, 0, 2)                               # (n, NC - 1, 4)
        sel = want.t()
        worst = max(worst, _check("class boxes image %d" % b, gotb[sel], cb64[:, 1:][sel], cb32[:, 1:][sel], floor=max(size)))
        orig = tuple(world["ims"][b].shape[1:])
        out = [S.postprocess(lg.to(dt), dl.to(dt), props.to(dt), size, orig, CFG) for dt in (torch.float64, torch.float32)]
        (bx64, lb64, sc64, m, kept), (bx32, lb32, sc32, _, _) = out
        assert min(m["score"], m["topk"]) > 1e-6 and m["iou"] > 1e-5 and lb64.tolist() == lb32.tolist(), "precondition: a decision on its threshold"
        cnt = int(d["counts"][b])
        assert cnt == len(lb64) and d["labels"][b, :cnt].cpu().tolist() == lb64.tolist(), b      # the kept set, in order
        keep_dev = torch.nonzero(d["keep_scores"][b].cpu() > float("-inf"))
        order = d["order"][b].cpu()
        kept_dev = sorted((int(order[c, q]), int(c) + 1) for c, q in keep_dev.tolist())
        pairs = [(r, c) for r in range(n) for c in range(1, NC) if want[c - 1, r]]
        assert pairs, "precondition: no candidate survives the filters"
        k64, _ = S.nms_per_category(torch.stack([cb64[r, c] for r, c in pairs]), torch.stack([pr64[r, c] for r, c in pairs]),
                                    torch.tensor([c for _, c in pairs]), CFG["box_nms_thresh"])
        assert kept_dev == sorted(pairs[i] for i in k64), b                                      # the kept set before the cut
        worst = max(worst, _check("detection boxes image %d" % b, d["boxes"][b, :cnt], bx64, bx32, floor=max(orig)))
        worst = max(worst, _check("detection scores image %d" % b, d["scores"][b, :cnt], sc64, sc32, floor=1.0))
        assert float(d["boxes"][b, cnt:].abs().sum()) == 0.0 and float(d["scores"][b, cnt:].abs().sum()) == 0.0 and int(d["labels"][b, cnt:].sum()) == 0
    print("worst err/bound  detector box head + detections  %.3f" % worst)


def test_end_to_end(world, dev):
    det, ims, dims = world["det"], world["ims"], world["dims"]
    r64, i64, bounds, problems = S.chain_preconditions(ims, world["sd"], CFG)
    assert not problems, "precondition (pick another detector_scenario.SEED): %s" % problems
    assert all(len(r["scores"]) >= 3 for r in r64)
    out = det(dims)
    worst = 0.0
    for b in range(2):
        assert set(out[b]) == {"boxes", "labels", "scores"} and out[b]["labels"].dtype == torch.int64
        assert out[b]["labels"].cpu().tolist() == r64[b]["labels"].tolist(), b
        eb = float((out[b]["boxes"].cpu().double() - r64[b]["boxes"]).abs().max())
        es = float((out[b]["scores"].cpu().double() - r64[b]["scores"]).abs().max())
        print("end to end image %d: %d detections  boxes err/bound = %.3f  scores err/bound = %.3f"
              % (b, len(r64[b]["scores"]), eb / bounds[b]["final_box"], es / bounds[b]["final_score"]))
        assert eb <= bounds[b]["final_box"] and es <= bounds[b]["final_score"]
        worst = max(worst, eb / bounds[b]["final_box"], es / bounds[b]["final_score"])
        s = out[b]["scores"]
        assert bool((s[:-1] >= s[1:]).all())
    print("worst err/bound  detector end to end  %.3f" % worst)
    same = lambda a, c: all(torch.equal(a[b][k], c[b][k]) for b in range(len(a)) for k in ("boxes", "labels", "scores"))
    # forward is the chained stages, and detect_padded[:n]
    feats = det.features(dims)
    props = det.proposals(feats)
    d = det.detections(feats, props, det.box_head(feats, props))
    n = d["counts"].tolist()
    assert same(out, [{"boxes": d["boxes"][b, :n[b]], "labels": d["labels"][b, :n[b]], "scores": d["scores"][b, :n[b]]} for b in range(2)])
    pb, pl, ps, pc = det.detect_padded(dims)
    assert tuple(pb.shape) == (2, 10, 4) and pc.tolist() == n
    assert same(out, [{"boxes": pb[b, :n[b]], "labels": pl[b, :n[b]], "scores": ps[b, :n[b]]} for b in range(2)])
    # a second call, a (B, 3, H, W) tensor and the list form, the images one at a time in the batch's frame (see the module docstring)
    assert same(out, det(dims))
    for b in range(2):
        one = det([dims[b]], frame=feats["frame"])
        assert same([out[b]], one), b
        assert same(one, det(dims[b][None], frame=feats["frame"]))


def test_through_the_consumers(world, dev):
    """predict_hrnet and DevicePredictFrontEnd with the detector as object_detect_model pick the box the oracle's detections pick."""
    import hrnet_scenario as HS
    from hierarchicalprobabilistic3dhuman_amd import configs, predict_frontend as PF, predict_hrnet
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet
    det = world["det"]
    image = world["ims"][0]
    H, W = image.shape[1:]
    r64, _, bounds, problems = S.chain_preconditions([image], world["sd"], CFG)
    assert not problems, problems
    thr = 0.5
    person = [k for k in range(len(r64[0]["scores"])) if int(r64[0]["labels"][k]) == 1 and float(r64[0]["scores"][k]) > thr]
    assert len(person) >= 2 and min(abs(float(s) - thr) for s in r64[0]["scores"]) >= 8 * bounds[0]["final_score"]
    bx = r64[0]["boxes"]
    dist = [((bx[k, 1] + bx[k, 3]) / 2 - H / 2.0) ** 2 + ((bx[k, 0] + bx[k, 2]) / 2 - W / 2.0) ** 2 for k in person]
    ranked = sorted(range(len(person)), key=lambda i: float(dist[i]))
    pick = person[ranked[0]]
    # a centre moves by at most one box bound, a squared distance by 2 (distance + bound) bound
    slack = 2 * (float(dist[ranked[1]]) ** 0.5 + 1) * bounds[0]["final_box"]
    assert float(dist[ranked[1]] - dist[ranked[0]]) >= 8 * slack, "precondition: two persons equally central"
    hcfg = HS.config("SMALL")
    hcfg["MODEL"]["IMAGE_SIZE"], hcfg["MODEL"]["HEATMAP_SIZE"] = [64, 96], [16, 24]
    hrnet = PoseHighResolutionNet(HS.config("SMALL")).eval()
    hrnet.load_state_dict(HS.seeded_state_dict(HS.shapes_of(hrnet.state_dict()), 0), strict=True)
    hrnet = hrnet.to(dev)
    with torch.no_grad():
        out = predict_hrnet.predict_hrnet(hrnet, hcfg, image.to(dev), object_detect_model=det, object_detect_threshold=thr)
    want_centre = torch.stack([(bx[pick, 1] + bx[pick, 3]) / 2, (bx[pick, 0] + bx[pick, 2]) / 2])
    err = float((out["bbox_centre"].cpu().double() - want_centre).abs().max())
    print("predict_hrnet box centre: |dev - f64| = %.3e  bound %.3e" % (err, bounds[0]["final_box"]))
    assert err <= bounds[0]["final_box"] and out["joints2D"].shape == (17, 2)
    pcfg = configs.get_cfg_defaults()
    pcfg.DATA.PROXY_REP_SIZE, pcfg.DATA.BBOX_THRESHOLD = 64, thr
    edge = CannyEdgeDetector(non_max_suppression=pcfg.DATA.EDGE_NMS, gaussian_filter_std=pcfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=pcfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=pcfg.DATA.EDGE_THRESHOLD).to(dev)
    front = PF.DevicePredictFrontEnd(pcfg, hrnet, hcfg, edge, det, 0.75, dev)
    res = front([image.to(dev)])
    assert int(res["records"][0, 10]) == pick
    err = float((res["bbox_centre"][0].cpu().double() - want_centre).abs().max())
    assert err <= bounds[0]["final_box"] and tuple(res["proxy_rep"].shape) == (1, 18, 64, 64)
