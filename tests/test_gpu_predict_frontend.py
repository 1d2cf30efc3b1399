"""The batched predict front end on the device (csrc/predict_frontend.hip, predict_frontend.DevicePredictFrontEnd, the
``batched_front_end`` route of predict_poseMF_shapeGaussian_net) against tests/predict_frontend_scenario.py.

    boxes        the device record equals the scenario's float32 record BIT FOR BIT: every selection case, both aspect steps,
                 B = 1 and a mixed batch
    crop         |dev - y64| <= 4 max(e_ref32, 2^-23 max|y64|); y64 is the reference's theta -> affine_grid -> grid_sample route in
                 float64 and e_ref32 the error of that SAME route in float32 (never the code under test); a sentinel around every
                 output; an entirely outside box gives zeros; normalised within 2 ulp of (raw - mean) / std; same bits alone and in a batch
    key points   exact against the scenario (first maximum, zeroed at max <= 0, visibility strictly above the threshold or forced);
                 proxy-crop joints within 4 * 2^-23 * D of float64
    chain        DevicePredictFrontEnd with the seeded SMALL HRNet: crops within the bound, key points = the arg-max of the model's own
                 heat maps, channel 0 = hps_canny_edge_map and channels 1..17 = hps_proxy_rep on the front end's own outputs, B = 4 equals
                 four B = 1 calls bit for bit, no host synchronisation, no growth of allocated memory
    predict      predict_poseMF_shapeGaussian_net with the device HRNet at batch sizes 1, 2, 3: the same .pt keys, the same key points
                 on both routes (precondition: top-2 heat-map gaps of at least 8 bounds), cam within 1e-4 of the network on each route's
                 own proxy representation, the three pictures per image

Worst err / bound as the tests printed them on an MI355X (measured values, not limits):

    crop  u8 1 x 1 source              0.540   (up-sampling x3 to 384 x 288: the position (j + 1/2) / 3 of a far output pixel carries
                                               the rounding of box / out; every other box on this source 0.30 or less)
    crop  u8 37 x 53 source            0.236
    crop  u8 200 x 150 source          0.259
    crop  f32 64 x 32 source           0.321
    proxy-crop joints                  0.062   (of 4 * 2^-23 * D; 96 x 72 maps 0.055, the rest exact)
    chain crops, toy detector          0.306   (no detector: 0.269)
    predict, both routes               key points equal on all five photographs (max|diff| = 0), smallest top-2 gap = 19.9 bounds

Records, key points, confidences, visibility, the proxy representation's channels and batch invariance are bit-for-bit checks.
No family is above 0.54; photographs sit at 0.24 .. 0.31.
"""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import hrnet_scenario as HS
import predict_frontend_scenario as S
from hierarchicalprobabilistic3dhuman_amd import _capi, configs, predict_frontend as PF
from hierarchicalprobabilistic3dhuman_amd.pose2D_hrnet import PoseHighResolutionNet

pytestmark = pytest.mark.gpu

SENTINEL = -7.5


def _bits(t):
    return np.ascontiguousarray(torch.as_tensor(t).detach().cpu().float().numpy()).view(np.int32)


def _det(boxes, labels, scores):
    return (torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), torch.tensor(labels, dtype=torch.int64),
            torch.tensor(scores, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_predict_boxes
# ---------------------------------------------------------------------------------------------------------------------------------
OUT_WH = (288, 384)
BOX_CASES = [  # name, H, W, detector output or None
    ("no detector", 200, 150, None),
    ("n = 0", 200, 150, _det([], [], [])),
    ("below the threshold", 200, 150, _det([[20.0, 30.0, 100.0, 170.0]], [1], [0.79])),
    ("only non-persons", 200, 150, _det([[20.0, 30.0, 100.0, 170.0], [1.0, 2.0, 3.0, 4.0]], [2, 17], [0.99, 0.9])),
    ("one person, width grows", 200, 150, _det([[40.5, 20.25, 90.0, 180.0]], [1], [0.9])),
    ("one person, height grows", 37, 53, _det([[2.0, 10.5, 50.0, 30.0]], [1], [0.85])),
    ("three persons", 200, 150, _det([[0.0, 0.0, 40.0, 90.0], [60.0, 70.0, 100.0, 150.0], [0.0, 0.0, 150.0, 200.0], [100.0, 120.0, 149.0, 199.0]],
                                     [1, 1, 5, 1], [0.9, 0.81, 0.99, 0.95])),
    ("two at equal distance", 200, 150, _det([[95.0, 80.0, 125.0, 120.0], [25.0, 80.0, 55.0, 120.0]], [1, 1], [0.9, 0.9])),
    ("1 x 1", 1, 1, None),
    ("37 x 53", 37, 53, None),
    ("exact aspect box", 200, 150, _det([[30.0, 20.0, 120.0, 140.0]], [1], [0.9])),          # 90 x 120: h == w * 4 / 3 exactly
]
EXPECT_PICK = {"one person, width grows": 0, "one person, height grows": 0, "three persons": 1, "two at equal distance": 0, "exact aspect box": 0}


def _dev_det(det, dev):
    return None if det is None else tuple(t.to(dev) for t in det)


def test_box_records_equal_the_scenario_bit_for_bit(dev):
    want = []
    for name, H, W, det in BOX_CASES:
        m = S.aspect_margin(H, W, det, OUT_WH, 0.8)
        assert m == 0.0 or m >= 1e-3, (name, m)                                       # precondition, CPU side
        rec = S.box_record(H, W, det, OUT_WH, 0.8, 1.2)
        assert int(rec[10]) == EXPECT_PICK.get(name, -1), name
        want.append(rec)
    grew_w = want[4][3] > (90.0 - 40.5) and want[4][2] == 180.0 - 20.25
    grew_h = want[5][2] > (30.0 - 10.5) and want[5][3] == 48.0
    assert grew_w and grew_h
    sizes = [(H, W) for _, H, W, _ in BOX_CASES]
    dets = [_dev_det(d, dev) for _, _, _, d in BOX_CASES]
    # a mixed batch of 7 (with and without detector outputs), the rest as a second batch, and every image alone
    got = torch.cat([PF.predict_boxes(sizes[:7], dets[:7], OUT_WH, 0.8, 1.2), PF.predict_boxes(sizes[7:], dets[7:], OUT_WH, 0.8, 1.2)]).cpu()
    for i, (name, _, _, _) in enumerate(BOX_CASES):
        assert np.array_equal(_bits(got[i]), _bits(want[i])), (name, got[i].tolist(), want[i].tolist())
        alone = PF.predict_boxes(sizes[i:i + 1], dets[i:i + 1], OUT_WH, 0.8, 1.2).cpu()
        assert np.array_equal(_bits(alone[0]), _bits(want[i])), name
    # no detector at all (detections=None), and the image of the output's own aspect with scale factor 1.0: neither side grows
    got = PF.predict_boxes([(384, 288), (1, 1)], None, OUT_WH, 0.8, 1.0).cpu()
    for i, (H, W) in enumerate([(384, 288), (1, 1)]):
        assert np.array_equal(_bits(got[i]), _bits(S.box_record(H, W, None, OUT_WH, 0.8, 1.0)))
    assert got[0].tolist()[:10] == [192.0, 144.0, 384.0, 288.0, 384.0, 288.0, 1.0, 1.0, 0.0, 0.0]
    # the static records of the second crop (no predict_hrnet aspect step)
    got = PF.predict_boxes([(384, 288)], None, (256, 256), 0.0, 1.0, hrnet_aspect_fix=False).cpu()
    assert np.array_equal(_bits(got[0]), _bits(S.box_record(384, 288, None, (256, 256), 0.0, 1.0, hrnet_fix=False)))
    assert got[0, 2] == 384 and got[0, 3] == 384


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_crop_bilinear
# ---------------------------------------------------------------------------------------------------------------------------------
def _source(kind, H, W, seed):
    rs = np.random.RandomState(seed)
    if kind == "u8":
        return torch.from_numpy(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
    return torch.from_numpy(rs.rand(3, H, W).astype(np.float32))


SOURCES = {"u8 1x1": ("u8", 1, 1), "u8 37x53": ("u8", 37, 53), "u8 200x150": ("u8", 200, 150), "f32 64x32": ("f32", 64, 32)}
OUTPUTS = [(32, 64), (12, 20), (288, 384)]


def _crop_record(kind, H, W, ow, oh):
    """A record with the fields the resample reads: centre (v, h), box height and width."""
    cv, ch = H / 2.0, W / 2.0
    if kind == "inside":
        bh, bw = 0.6 * H, 0.6 * W
    elif kind == "overhang":
        bh, bw = 1.15 * H + 1.0, 1.1 * W + 1.5
    elif kind == "larger":
        bh, bw = 3.0 * H, 2.5 * W
    elif kind == "outside":
        cv, ch, bh, bw = -2.0 * H - 5.0, 3.5 * W + 7.0, float(H), float(W)
    elif kind == "up x3":
        cv, ch, bh, bw = 0.37 * H, 0.61 * W, oh / 3.0, ow / 3.0
    elif kind == "down x5":
        bh, bw = 5.0 * oh, 5.0 * ow
    rec = torch.zeros(S.REC, dtype=torch.float32)
    rec[0], rec[1], rec[4], rec[5] = cv, ch, bh, bw
    return rec


def _guarded(shape, dev):
    n = int(np.prod(shape))
    buf = torch.full((n + 512,), SENTINEL, device=dev)
    return buf, buf[256:256 + n].view(shape)


def _assert_guard(buf, n):
    assert bool((buf[:256] == SENTINEL).all()) and bool((buf[256 + n:] == SENTINEL).all())


@pytest.mark.parametrize("src_name", list(SOURCES))
def test_crop_against_float64(dev, src_name):
    kind, H, W = SOURCES[src_name]
    img = _source(kind, H, W, H * 7 + W)
    d_img = img.to(dev)
    worst = 0.0
    for ow, oh in OUTPUTS:
        for box in ("inside", "overhang", "larger", "outside", "up x3", "down x5"):
            rec = _crop_record(box, H, W, ow, oh)
            y64, y32 = (S.crop_theta(img, (ow, oh), rec, dt) for dt in (torch.float64, torch.float32))
            raw_buf, raw = _guarded((1, 3, oh, ow), dev)
            nrm_buf, nrm = _guarded((1, 3, oh, ow), dev)
            PF.crop_bilinear([d_img], rec[None].to(dev), (ow, oh), normalise=(S.IMAGENET_MEAN, S.IMAGENET_STD), raw=raw, normalised=nrm)
            _assert_guard(raw_buf, raw.numel())
            _assert_guard(nrm_buf, nrm.numel())
            got = raw[0].cpu()
            if box == "outside":
                assert float(y64.abs().max()) == 0.0 and float(got.abs().max()) == 0.0
            elif H > 1:
                assert float(y64.abs().max()) > 0.0
            worst = max(worst, S.check("%s -> %dx%d %s" % (src_name, oh, ow, box), got, y64, y32))
            want_n = S.normalise(got)
            ulp = float(((nrm[0].cpu() - want_n).abs() / (S.EPS32 * want_n.abs().clamp_min(1e-30))).max())
            assert ulp <= 2.0, (src_name, box, ulp)
            # without the normalised output nothing else changes
            raw2_buf, raw2 = _guarded((1, 3, oh, ow), dev)
            PF.crop_bilinear([d_img], rec[None].to(dev), (ow, oh), raw=raw2)
            assert torch.equal(raw2, raw)
            _assert_guard(raw2_buf, raw2.numel())
    print("worst err/bound  crop %s  %.3f" % (src_name, worst))


def test_crop_has_the_same_bits_alone_and_in_a_mixed_batch(dev):
    ow, oh = 32, 64
    names = ["u8 37x53", "f32 64x32", "u8 1x1", "u8 200x150", "u8 37x53"]
    imgs = [_source(*SOURCES[n], seed=i).to(dev) for i, n in enumerate(names)]
    recs = torch.stack([_crop_record(b, SOURCES[n][1], SOURCES[n][2], ow, oh)
                        for n, b in zip(names, ("overhang", "inside", "larger", "down x5", "up x3"))]).to(dev)
    raw, nrm = PF.crop_bilinear(imgs, recs, (ow, oh), normalise=(S.IMAGENET_MEAN, S.IMAGENET_STD))
    for i in range(len(imgs)):
        r1, n1 = PF.crop_bilinear(imgs[i:i + 1], recs[i:i + 1], (ow, oh), normalise=(S.IMAGENET_MEAN, S.IMAGENET_STD))
        assert torch.equal(r1[0], raw[i]) and torch.equal(n1[0], nrm[i]), names[i]


# ---------------------------------------------------------------------------------------------------------------------------------
# hps_hrnet_keypoints
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [17, 1])
@pytest.mark.parametrize("h,w", [(5, 7), (16, 8), (96, 72)])
def test_keypoints_equal_the_scenario(dev, h, w, K):
    hm = torch.cat([S.special_heatmaps(K, h, w, s) for s in (0, 1, 2)])
    hm[2] = -hm[2].abs() - 0.01 if K == 1 else hm[2]                                  # K = 1: also an all-negative single map
    D, factor = 64, 4.0
    rec = torch.stack([S.box_record(4 * h, 4 * w, None, (D, D), 0.0, 1.0, hrnet_fix=False)] * 3)
    worst = 0.0
    for mask in (S.ALWAYS_VISIBLE, ()):
        bits = sum(1 << k for k in mask)
        idx, joints, confs, crop32, visib = S.keypoints(hm, factor, rec, 0.75, bits)
        crop64 = S.keypoints(hm, factor, rec, 0.75, bits, dtype=torch.float64)[3]
        g_joints, g_confs, g_crop, g_visib = PF.hrnet_keypoints(hm.to(dev), factor, rec.to(dev), 0.75, mask)
        assert np.array_equal(_bits(g_joints), _bits(joints)) and np.array_equal(_bits(g_confs), _bits(confs))
        assert torch.equal(g_visib.cpu(), visib)
        err = float((g_crop.cpu().double() - crop64).abs().max())
        worst = max(worst, err / (4 * S.EPS32 * D))
        assert err <= 4 * S.EPS32 * D
        # without records: the same key points, no crop joints
        g2 = PF.hrnet_keypoints(hm.to(dev), factor, None, 0.75, mask)
        assert g2[2] is None and torch.equal(g2[0], g_joints) and torch.equal(g2[1], g_confs) and torch.equal(g2[3], g_visib)
    if K == 17:
        n = h * w
        assert idx[0, 0] == 0 and idx[0, 1] == n - 1 and idx[0, 2] == n // 3 and confs[0, 4] == 0 and confs[0, 5] == 0.75
        assert g_joints[0, 3].tolist() == [0.0, 0.0] and g_joints[0, 4].tolist() == [0.0, 0.0] and float(g_confs[0, 3]) < 0
        assert g_visib[0, 5] == 0 and g_visib[0, 6] == 1                              # last pass: no forced joints
    print("worst err/bound  proxy-crop joints %dx%d K %d  %.3f" % (h, w, K, worst))


# ---------------------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------------------
class _ToyDetector(torch.nn.Module):
    """Stand-in for the injected person detector: one confident person inside the image, one less central, one non-person."""

    def forward(self, images):
        H, W = images.shape[-2:]
        d = images.device
        boxes = torch.tensor([[0.0, 0.0, 0.4 * W, 0.5 * H], [0.2 * W, 0.1 * H, 0.85 * W, 0.95 * H], [0.0, 0.0, W, H]], device=d)
        return [{"labels": torch.tensor([1, 1, 3], device=d), "scores": torch.tensor([0.97, 0.99, 1.0], device=d), "boxes": boxes}]


def _hrnet_cfg():
    cfg = HS.config("SMALL")
    cfg["MODEL"]["IMAGE_SIZE"], cfg["MODEL"]["HEATMAP_SIZE"] = [64, 96], [16, 24]
    return cfg


def _pose_cfg(D):
    cfg = configs.get_cfg_defaults()
    cfg.DATA.PROXY_REP_SIZE = D
    return cfg


def _photos(sizes, seed):
    rs = np.random.RandomState(seed)
    out = []
    for h, w in sizes:
        base = rs.rand((h + 3) // 4, (w + 3) // 4, 3)
        out.append((np.kron(base, np.ones((4, 4, 1)))[:h, :w] * 255).astype(np.uint8))
    return out


@pytest.fixture(scope="module")
def small_hrnet(dev):
    shapes = HS.shapes_of(PoseHighResolutionNet(HS.config("SMALL")).state_dict())
    sd = HS.seeded_state_dict(shapes, 0)
    net = PoseHighResolutionNet(HS.config("SMALL")).eval()
    net.load_state_dict(sd, strict=True)
    return net.to(dev), sd


@pytest.fixture(scope="module")
def edge(dev):
    from hierarchicalprobabilistic3dhuman_amd.canny_edge_detector import CannyEdgeDetector
    cfg = configs.get_cfg_defaults()
    return CannyEdgeDetector(non_max_suppression=cfg.DATA.EDGE_NMS, gaussian_filter_std=cfg.DATA.EDGE_GAUSSIAN_STD,
                             gaussian_filter_size=cfg.DATA.EDGE_GAUSSIAN_SIZE, threshold=cfg.DATA.EDGE_THRESHOLD).to(dev)


CHAIN_SIZES = [(60, 60), (48, 72), (101, 67), (64, 64)]
CHAIN_KEYS = ("proxy_rep", "cropped_rgb", "joints2D", "joints2D_hrnet", "joints2Dconfs", "visib", "hrnet_input", "bbox_centre", "bbox_height",
              "bbox_width", "bbox_wh")


@pytest.mark.parametrize("with_detector", [True, False], ids=["toy detector", "no detector"])
def test_chain_with_the_small_hrnet(dev, small_hrnet, edge, with_detector):
    from hierarchicalprobabilistic3dhuman_amd.label_conversions import make_proxy_representation
    hrnet, _ = small_hrnet
    D, hcfg = 64, _hrnet_cfg()
    pcfg = _pose_cfg(D)
    detector = _ToyDetector().to(dev) if with_detector else None
    front = PF.DevicePredictFrontEnd(pcfg, hrnet, hcfg, edge, detector, 0.75, dev)
    photos = _photos(CHAIN_SIZES, 5)
    out = front(photos)
    B = len(photos)
    assert set(CHAIN_KEYS) <= set(out)
    assert out["proxy_rep"].shape == (B, 18, D, D) and out["cropped_rgb"].shape == (B, 3, D, D) and out["hrnet_input"].shape == (B, 3, 96, 64)
    assert out["joints2D"].shape == (B, 17, 2) and out["bbox_centre"].shape == (B, 2) and out["bbox_wh"].shape == (B,)
    in_wh = (64, 96)
    rec2 = S.box_record(96, 64, None, (D, D), 0.0, 1.0, hrnet_fix=False)
    worst = 0.0
    for b, u8 in enumerate(photos):
        H, W = u8.shape[:2]
        det = None
        if with_detector:
            det = tuple(t.cpu() for t in (lambda p: (p["boxes"], p["labels"], p["scores"]))(detector(torch.zeros(1, 3, H, W, device=dev))[0]))
        rec = S.box_record(H, W, det, in_wh, pcfg.DATA.BBOX_THRESHOLD, pcfg.DATA.BBOX_SCALE_FACTOR)
        assert np.array_equal(_bits(out["records"][b]), _bits(rec)), b
        assert int(rec[10]) == (1 if with_detector else -1)
        assert np.array_equal(_bits(out["bbox_centre"][b]), _bits(rec[0:2])) and np.array_equal(_bits(out["bbox_wh"][b]), _bits(rec[11]))
        y64, y32 = (S.normalise(S.crop_theta(u8, in_wh, rec, dt), dt) for dt in (torch.float64, torch.float32))
        worst = max(worst, S.check("chain hrnet_input %d" % b, out["hrnet_input"][b].cpu(), y64, y32))
        raw = out["hrnet_crop"][b].cpu()
        z64, z32 = (S.crop_theta(raw, (D, D), rec2, dt) for dt in (torch.float64, torch.float32))
        worst = max(worst, S.check("chain cropped_rgb %d" % b, out["cropped_rgb"][b].cpu(), z64, z32))
    print("worst err/bound  chain crops (%s)  %.3f" % ("toy detector" if with_detector else "no detector", worst))
    # the threshold steps on identical inputs: the model's own heat maps, the front end's own crop and joints
    hm = hrnet(out["hrnet_input"])
    idx, joints, confs, crop64, visib = S.keypoints(hm.cpu(), 64 / 16, torch.stack([rec2] * B), 0.75, dtype=torch.float64)
    assert np.array_equal(_bits(out["joints2D_hrnet"]), _bits(joints)) and np.array_equal(_bits(out["joints2Dconfs"]), _bits(confs))
    assert torch.equal(out["visib"].cpu(), visib)
    assert float((out["joints2D"].cpu().double() - crop64).abs().max()) <= 4 * S.EPS32 * D
    want = torch.empty(B, 18, D, D, device=dev)
    edge.edge_map_into(out["cropped_rgb"], want, nms=bool(pcfg.DATA.EDGE_NMS))
    assert torch.equal(out["proxy_rep"][:, 0], want[:, 0])
    make_proxy_representation(None, out["joints2D"], out["visib"], D, pcfg.DATA.HEATMAP_GAUSSIAN_STD, out=want)
    assert torch.equal(out["proxy_rep"], want)
    assert float(out["proxy_rep"][:, 0].abs().sum()) > 0 and float(out["proxy_rep"][:, 1:].abs().sum()) > 0
    # B = 4 equals four B = 1 calls, bit for bit; host arrays, page-locked and device tensors are the same images
    for b in range(B):
        forms = [photos[b], torch.from_numpy(photos[b]).pin_memory(), torch.from_numpy(photos[b]).to(dev)]
        for form in forms[:1] if b else forms:
            one = front([form])
            for k in CHAIN_KEYS:
                assert torch.equal(one[k][0], out[k][b]), (k, b)
    f_img = (torch.from_numpy(photos[0]).float() / 255.0).permute(2, 0, 1).contiguous()      # a true division (torch's device kernel
    one = front([f_img.to(dev)])                                                   # multiplies by 1 / 255): the (3,H,W) float contract
    assert torch.equal(one["hrnet_input"][0], out["hrnet_input"][0]) and torch.equal(one["proxy_rep"][0], out["proxy_rep"][0])


def test_chain_steady_state_has_no_host_synchronisation_and_no_memory_growth(dev, small_hrnet, edge):
    hrnet, _ = small_hrnet
    front = PF.DevicePredictFrontEnd(_pose_cfg(64), hrnet, _hrnet_cfg(), edge, None, 0.75, dev)
    resident = [torch.from_numpy(p).to(dev) for p in _photos(CHAIN_SIZES, 6)]
    first = {k: v.clone() for k, v in front(resident).items() if torch.is_tensor(v)}
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = front(resident)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for k in CHAIN_KEYS:
        assert torch.equal(second[k], first[k]), k
    del second
    front(resident)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    for _ in range(10):
        front(resident)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before


# ---------------------------------------------------------------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------------------------------------------------------------
PREDICT_SIZES = {"a": (60, 60), "b": (48, 72), "c": (64, 64), "d": (101, 67), "e": (80, 56)}
WH = 64


def _densepose(num_verts, seed=31, num_faces=300):
    """A synthetic DensePose table over the synthetic SMPL's vertices: every vertex once, 5 % twice, ``num_faces`` faces over them."""
    rs = np.random.RandomState(seed)
    verts_map = np.concatenate([np.arange(num_verts), rs.randint(0, num_verts, num_verts // 20)])
    Nd = len(verts_map)
    faces = np.stack([rs.choice(Nd, 3, replace=False) for _ in range(num_faces)]).astype(np.int64)
    iuv = np.stack([1 + np.arange(Nd) % 24, rs.rand(Nd), rs.rand(Nd)], axis=1).astype(np.float32)
    return (torch.from_numpy(rs.rand(1, Nd, 2).astype(np.float32)), torch.from_numpy(iuv)[None], torch.from_numpy(verts_map),
            torch.from_numpy(faces)[None])


@pytest.fixture(scope="module")
def predict_harness(dev, net_gpu, smpl_gpu, small_hrnet, edge, tmp_path_factory):
    from hierarchicalprobabilistic3dhuman_amd import predict_poseMF_shapeGaussian_net as P, textured_renderer as tr
    root = tmp_path_factory.mktemp("predict_frontend")
    image_dir = root / "images"
    os.makedirs(str(image_dir))
    photos = dict(zip(PREDICT_SIZES, _photos(list(PREDICT_SIZES.values()), 9)))
    for name, u8 in photos.items():
        np.save(str(image_dir / (name + ".npy")), u8)
    hrnet, sd = small_hrnet
    cfg, hcfg = configs.get_cfg_defaults(), _hrnet_cfg()
    renderer = tr.TexturedIUVRenderer(dev, 1, img_wh=WH, projection_type="orthographic", render_rgb=True, bin_size=32,
                                      densepose_uv=_densepose(smpl_gpu.num_verts))
    runs = {}

    def run(batch_size, batched, vis=False):
        key = (batch_size, batched, vis)
        if key not in runs:
            save_dir = root / ("out_b%d_%s_%d" % key)
            torch.manual_seed(11)
            P.predict_poseMF_shapeGaussian_net(net_gpu, cfg, smpl_gpu, hrnet, hcfg, edge, dev, str(image_dir), str(save_dir),
                                               visualise_wh=WH, visualise_uncropped=True, visualise_samples=True, num_samples=12,
                                               batch_size=batch_size, vis_renderer=renderer if vis else None, batched_front_end=batched)
            runs[key] = save_dir
        return runs[key]
    return NS(run=run, photos=photos, cfg=cfg, hcfg=hcfg, hrnet=hrnet, sd=sd, image_dir=image_dir, P=P)


def test_predict_routes_agree_on_the_key_points(predict_harness, dev, edge, net_gpu):
    h = predict_harness
    front = PF.DevicePredictFrontEnd(h.cfg, h.hrnet, h.hcfg, edge, None, 0.75, dev)
    names = sorted(h.photos)
    out = front([h.photos[n] for n in names])
    # precondition (CPU side): every joint's two largest float64 heat-map values are at least 8 bounds apart
    x = out["hrnet_input"].cpu()
    with torch.no_grad():
        y64, y32 = HS.forward64(h.sd, h.hcfg, x.double()), HS.forward64(h.sd, h.hcfg, x)
    bound = HS.bound(y64, y32)[0]
    gaps = HS.top2_gap(y64)
    print("top-2 gaps: min %.3e, bound %.3e, min gap / bound = %.1f" % (float(gaps.min()), bound, float(gaps.min()) / bound))
    assert float(gaps.min()) >= 8 * bound, "precondition: pick another seed for the photographs"
    per_image = h.P._reference_front_end(h.cfg, h.hrnet, h.hcfg, edge, None, 0.75, dev)
    D = h.cfg.DATA.PROXY_REP_SIZE
    for b, n in enumerate(names):
        ex = per_image.with_extras(str(h.image_dir / (n + ".npy")))
        d = float((ex["joints2D"][0] - out["joints2D"][b]).abs().max())
        print("%s: max|joints2D batched - per image| = %.3e" % (n, d))
        assert torch.equal(ex["joints2D"][0], out["joints2D"][b]), n
        assert float((ex["bbox_centre"] - out["bbox_centre"][b]).abs().max()) == 0.0
        assert float((ex["cropped_rgb"][0] - out["cropped_rgb"][b]).abs().max()) <= 1e-4


@pytest.mark.parametrize("batch_size", [1, 2, 3])          # hipGraph replays (and the eager path for a last, smaller group); the pipeline
def test_predict_with_the_device_hrnet(predict_harness, dev, edge, net_gpu, batch_size):
    h = predict_harness
    names = sorted(h.photos)
    dirs = {flag: h.run(batch_size, flag) for flag in (True, False)}
    keys = {"verts_mode", "joints_mode", "verts_tpose", "unc", "cam", "glob_rotmats"}
    fronts = {True: PF.DevicePredictFrontEnd(h.cfg, h.hrnet, h.hcfg, edge, None, 0.75, dev),
              False: h.P._reference_front_end(h.cfg, h.hrnet, h.hcfg, edge, None, 0.75, dev)}
    for flag, d in dirs.items():
        assert sorted(os.listdir(str(d))) == [n + ".pt" for n in names]
        for n in names:
            saved = torch.load(str(d / (n + ".pt")))
            assert set(saved) == keys
            path = str(h.image_dir / (n + ".npy"))
            proxy = fronts[True]([np.load(path)])["proxy_rep"] if flag else fronts[False](path)
            with torch.no_grad():
                cam = net_gpu(proxy.float())[7][0].cpu()
            err = float((saved["cam"] - cam).abs().max())
            assert err <= 1e-4, (flag, n, err)
    if batch_size != 3:
        return
    for n in names:                                                               # None selects the batched route for the device HRNet
        a, b = torch.load(str(h.run(batch_size, None) / (n + ".pt"))), torch.load(str(dirs[True] / (n + ".pt")))
        assert all(torch.equal(a[k], b[k]) for k in ("verts_mode", "verts_tpose", "cam", "glob_rotmats")), n


@pytest.mark.parametrize("batch_size", [1, 3])
def test_predict_writes_the_three_pictures_on_the_batched_route(predict_harness, batch_size):
    h = predict_harness
    d = h.run(batch_size, True, vis=True)
    from PIL import Image
    for n, (hh, ww) in PREDICT_SIZES.items():
        for suffix, shape in (("", (2 * WH, 4 * WH, 3)), ("_uncrop", (hh, ww, 3)), ("_samples", (3 * WH, 6 * WH, 3))):
            path = d / (n + suffix + ".png")
            assert path.exists(), path
            assert np.asarray(Image.open(str(path))).shape == shape
        assert (d / (n + ".pt")).exists()
        fig = np.asarray(Image.open(str(d / (n + ".png"))))
        assert fig[:WH, WH:2 * WH].std() > 0 and fig[WH:, :WH].max() == 255           # a body over a crop; red discs on the proxy panel
