"""CPU restatement of the predict front end (csrc/predict_frontend.hip, predict_frontend.DevicePredictFrontEnd) with torch, for
tests/test_predict_frontend_host.py, tests/test_gpu_predict_frontend.py and tests/golden/make_predict_frontend_golden.py.  Nothing
here touches a device.

Two parts:

  box_record       the person box, both aspect steps, the scale factor and the forward affine in float32, every operation one torch
                   float32 operation in the reference's order (predict/predict_hrnet.py:48-87, utils/image_utils.py:310-334) -> the
                   12-float record of include/hps.h.  Held bit for bit to the reference (fixture) and by the device.
  crop_theta, crop_pixels, keypoints
                   the resample, the joint transform and the arg-max FROM that float32 record, in float32 or float64.  crop_theta is
                   the reference's own route (normalised inverse theta -> affine_grid -> grid_sample); crop_pixels is the pixel-space
                   form the kernel evaluates.  crop_theta in float64 is the truth y64 of the accuracy rule, crop_theta in float32 the
                   reference's own float32 route, whose error e_ref32 sets the bound:

                       |dev - y64| <= 4 max(e_ref32, 2^-23 max|y64|)
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -23
REC = 12
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
ALWAYS_VISIBLE = (0, 1, 2, 3, 4, 5, 6, 11, 12)
ALWAYS_VISIBLE_MASK = sum(1 << k for k in ALWAYS_VISIBLE)

f32 = lambda v: torch.tensor(v, dtype=torch.float32)


def select_box(H, W, det, threshold):
    """predict_hrnet.py:48-80 -> (centre_v, centre_h, height, width) as float32 0-dim tensors and the chosen index (-1: whole image).
    ``det``: None (no detector) or (boxes (n,4) x1 y1 x2 y2, labels (n) int64, scores (n))."""
    whole = (f32(float(H)) * 0.5, f32(float(W)) * 0.5, f32(float(H)), f32(float(W)), -1)
    if det is None:
        return whole
    boxes, labels, scores = (torch.as_tensor(t) for t in det)
    boxes, scores = boxes.float().reshape(-1, 4), scores.float().reshape(-1)
    keep = [k for k in range(boxes.shape[0]) if int(labels[k]) == 1 and bool(scores[k] > threshold)]
    if not keep:
        return whole
    cv = [(boxes[k, 1] + boxes[k, 3]) / 2.0 for k in keep]
    ch = [(boxes[k, 0] + boxes[k, 2]) / 2.0 for k in keep]
    dist = [(v - H / 2.0) ** 2 + (h - W / 2.0) ** 2 for v, h in zip(cv, ch)]
    best = 0
    for i in range(1, len(keep)):
        if bool(dist[i] < dist[best]):
            best = i
    k = keep[best]
    return cv[best], ch[best], boxes[k, 3] - boxes[k, 1], boxes[k, 2] - boxes[k, 0], k


def box_record(H, W, det, out_wh, threshold, scale_factor, hrnet_fix=True):
    """The float32 record (12,) of one image; see include/hps.h.  ``out_wh`` = (width, height) of the crop."""
    cv, ch, h, w, picked = select_box(H, W, det, threshold)
    h, w = h.clone(), w.clone()
    ow, oh = f32(float(out_wh[0])), f32(float(out_wh[1]))
    if hrnet_fix:                                                     # predict_hrnet.py:83-87
        aspect = float(out_wh[1]) / float(out_wh[0])
        if bool(h > w * aspect):
            w = h / aspect
        elif bool(h < w * aspect):
            h = w * aspect
    aspect = (oh / ow).item()                                         # image_utils.py:310-312
    if bool(h > w * aspect):
        w = h / aspect
    if bool(h < w * aspect):
        h = w * aspect
    bh, bw = h * scale_factor, w * scale_factor                       # :321-322
    sx, sy = ow / bw, oh / bh                                         # :331-333
    tx, ty = ow * 0.5 - sx * ch, oh * 0.5 - sy * cv                   # :329, :334
    side = torch.max(h, w) * scale_factor
    rec = torch.stack([cv, ch, h, w, bh, bw, sx, sy, tx, ty, f32(float(picked)), side]).float()
    assert rec.dtype == torch.float32 and rec.shape == (REC,)
    return rec


def aspect_margin(H, W, det, out_wh, threshold):
    """The relative distance of the chosen box's  h  from  w aspect  (0.0: exactly equal in float32) -- the precondition of the
    device box tests: a comparison is either exact or separated by at least 1e-3."""
    _, _, h, w, _ = select_box(H, W, det, threshold)
    a = float(out_wh[1]) / float(out_wh[0])
    if bool(h == w * a) and bool(h == w * (f32(float(out_wh[1])) / f32(float(out_wh[0])))):
        return 0.0
    return abs(float(h) - float(w) * a) / max(abs(float(h)), 1e-30)


def to_chw(image, dtype=torch.float32):
    """A source as the kernel reads it: (H,W,3) uint8 -> float32(u8) / 255 (a true float32 division), or (3,H,W) float; as ``dtype``."""
    image = torch.as_tensor(image)
    if image.dtype == torch.uint8:
        image = (image.float() / 255.0).permute(2, 0, 1)
    return image.contiguous().to(dtype)


def crop_theta(image, out_wh, rec, dtype):
    """utils/image_utils.py:329-370 from the float32 record: (3, out_h, out_w) in ``dtype``."""
    img = to_chw(image, dtype)
    H, W = img.shape[1:]
    r = rec.to(dtype)
    in_wh = torch.tensor([W, H], dtype=dtype)
    out = torch.tensor([out_wh[0], out_wh[1]], dtype=dtype)
    centre, bwh = r[0:2][None], torch.stack([r[5], r[4]])[None]
    A = torch.zeros(1, 2, 3, dtype=dtype)
    A[:, 0, 0] = out[0] / bwh[:, 0]
    A[:, 1, 1] = out[1] / bwh[:, 1]
    A[:, :, 2] = out * 0.5 - (out / bwh) * centre[:, [1, 0]]
    T = torch.zeros(1, 2, 3, dtype=dtype)
    T[:, 0, 0] = bwh[:, 0] / in_wh[0]
    T[:, 1, 1] = bwh[:, 1] / in_wh[1]
    T[:, :, 2] = -A[:, :, 2] / (out / bwh)
    T[:, :, 2] = T[:, :, 2] / (in_wh * 0.5) + (bwh / in_wh) - 1
    grid = F.affine_grid(T, [1, 1, int(out_wh[1]), int(out_wh[0])], align_corners=False)
    return F.grid_sample(img[None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0]


def sample_positions(out_wh, rec, dtype):
    """x (out_w), y (out_h): the pixel-space sample positions of include/hps.h's hps_crop_bilinear."""
    r = rec.to(dtype)
    ow, oh = int(out_wh[0]), int(out_wh[1])
    x = (torch.arange(ow, dtype=dtype) + 0.5) * (r[5] / ow) + ((r[1] - r[5] * 0.5) - 0.5)
    y = (torch.arange(oh, dtype=dtype) + 0.5) * (r[4] / oh) + ((r[0] - r[4] * 0.5) - 0.5)
    return x, y


def crop_pixels(image, out_wh, rec, dtype):
    """The kernel's form: four taps around the pixel-space position, each zero on its own outside the image, summed in the order
    ((t00 + t01) + t10) + t11."""
    img = to_chw(image, dtype)
    H, W = img.shape[1:]
    x, y = sample_positions(out_wh, rec, dtype)
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0

    def tap(yy, xx):
        ok = ((yy >= 0) & (yy < H))[:, None] & ((xx >= 0) & (xx < W))[None, :]
        v = img[:, yy.clamp(0, H - 1).long()][:, :, xx.clamp(0, W - 1).long()]
        return v * ok

    return (((tap(y0, x0) * ((1 - fy)[:, None] * (1 - fx)[None]) + tap(y0, x0 + 1) * ((1 - fy)[:, None] * fx[None]))
             + tap(y0 + 1, x0) * (fy[:, None] * (1 - fx)[None])) + tap(y0 + 1, x0 + 1) * (fy[:, None] * fx[None]))


def normalise(raw, dtype=torch.float32):
    """transforms.Normalize with the ImageNet constants (predict_hrnet.py:101-102)."""
    mean = torch.tensor(IMAGENET_MEAN, dtype=dtype)[:, None, None]
    std = torch.tensor(IMAGENET_STD, dtype=dtype)[:, None, None]
    return (raw.to(dtype) - mean) / std


def bound(y64, y_ref32):
    """(4 max(e_ref32, 2^-23 max|y64|), e_ref32, max|y64|)."""
    scale = float(y64.abs().max())
    e = float((y_ref32.double() - y64).abs().max())
    return 4.0 * max(e, EPS32 * scale), e, scale


def check(name, got, y64, y_ref32):
    """Prints the figures, asserts the accuracy rule on the whole tensor, returns err / bound (0 / 0 counts as 0)."""
    b, e, scale = bound(y64, y_ref32)
    err = float((torch.as_tensor(got).detach().cpu().double() - y64).abs().max())
    ratio = 0.0 if err == 0.0 else (err / b if b > 0 else float("inf"))
    print("%-52s max|got - f64| = %.3e  e_ref32 = %.3e  max|y64| = %.3e  err/bound = %.3f" % (name, err, e, scale, ratio))
    assert err == err and err <= b, (name, err, b)
    return ratio


def keypoints(heatmaps, factor, rec_proxy=None, vis_threshold=0.75, always_visible=ALWAYS_VISIBLE_MASK, dtype=torch.float32):
    """predict_hrnet.py:7-31, :104-107 and the joint transform / visibility of the caller: heatmaps (B,K,h,w) float32 ->
    idx (B,K) int64 (FIRST maximum), joints_hrnet (B,K,2), confs (B,K) float32, joints_crop (B,K,2) in ``dtype`` (None without records
    (B,12)), visib (B,K) float32 0/1."""
    hm = torch.as_tensor(heatmaps).float()
    B, K, h, w = hm.shape
    flat = hm.reshape(B, K, -1)
    confs = flat.max(dim=2).values
    idx = (flat == confs[:, :, None]).to(torch.uint8).argmax(dim=2)                 # argmax of 0/1: documented to return the first 1
    for b in range(B):                                                            # ... and checked, cheaply
        for k in range(K):
            assert int(idx[b, k]) == int(torch.nonzero(flat[b, k] == confs[b, k])[0])
    kp = torch.stack([(idx % w).float(), torch.floor(idx / float(w)).float()], dim=-1)
    kp = kp * (confs > 0.0)[:, :, None]
    joints = kp * factor
    crop = None
    if rec_proxy is not None:
        r = torch.as_tensor(rec_proxy).to(dtype).reshape(B, REC)
        crop = joints.to(dtype) * r[:, None, 6:8] + r[:, None, 8:10]
    visib = confs > vis_threshold
    for k in range(K):
        if (always_visible >> k) & 1:
            visib[:, k] = True
    return idx, joints, confs, crop, visib.float()


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases of tests/golden/predict_frontend_vectors.npz: IMAGE_SIZE = [32, 64] (width, height), HEATMAP_SIZE = [8, 16], proxy size 32
# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN_IMAGE_SIZE, GOLDEN_HEATMAP_SIZE, GOLDEN_PROXY = (32, 64), (8, 16), 32
GOLDEN_THRESHOLD, GOLDEN_SCALE_FACTOR, GOLDEN_VIS_THRESHOLD = 0.8, 1.2, 0.75
Case = collections.namedtuple("Case", "H W det seed")
GOLDEN_CASES = collections.OrderedDict([
    ("none_37x53", Case(37, 53, None, 1)),
    ("none_1x1", Case(1, 1, None, 2)),
    ("none_64x32", Case(64, 32, None, 3)),                                                  # the output's own aspect: neither side grows
    ("empty_40x50", Case(40, 50, ([], [], []), 4)),
    ("low_40x50", Case(40, 50, ([[5.0, 4.0, 30.0, 38.0]], [1], [0.5]), 5)),               # a person below the threshold
    ("other_40x50", Case(40, 50, ([[5.0, 4.0, 30.0, 38.0]], [3], [0.99]), 6)),            # only a non-person
    ("one_60x45", Case(60, 45, ([[10.25, 6.5, 31.0, 55.75]], [1], [0.9]), 7)),            # tall: the width grows
    ("wide_45x60", Case(45, 60, ([[3.0, 12.5, 57.5, 30.0]], [1], [0.97]), 8)),            # wide: the height grows
    ("three_60x80", Case(60, 80, ([[1.0, 2.0, 20.0, 40.0], [30.0, 10.0, 52.5, 55.0], [0.0, 0.0, 80.0, 60.0], [50.0, 5.0, 79.0, 58.0]],
                                  [1, 1, 7, 1], [0.95, 0.85, 0.99, 0.9]), 9)),
    ("tie_60x80", Case(60, 80, ([[50.0, 20.0, 70.0, 40.0], [10.0, 20.0, 30.0, 40.0]], [1, 1], [0.9, 0.9]), 10)),   # equal distance: the first
])


def case_det(case):
    if case.det is None:
        return None
    b, l, s = case.det
    return (torch.tensor(b, dtype=torch.float32).reshape(-1, 4), torch.tensor(l, dtype=torch.int64), torch.tensor(s, dtype=torch.float32))


def case_image(case):
    """(H, W, 3) uint8, seeded."""
    return np.random.RandomState(case.seed).randint(0, 256, (case.H, case.W, 3)).astype(np.uint8)


def special_heatmaps(K, h, w, seed):
    """(1, K, h, w) float32, seeded; the first maps carry the edge cases of the arg-max: 0 maximum at the first element, 1 at the last,
    2 two equal maxima, 3 all negative, 4 maximum exactly 0, 5 maximum exactly at the visibility threshold 0.75, 6 just above it."""
    g = torch.Generator().manual_seed(100 + seed)
    hm = torch.rand(1, K, h, w, generator=g) * 0.7
    n = h * w
    flat = hm.view(1, K, n)

    def put(k, fn):
        if k < K:
            fn(flat[0, k])
    put(0, lambda m: m.__setitem__(0, 0.9))
    put(1, lambda m: m.__setitem__(n - 1, 0.95))
    put(2, lambda m: (m.__setitem__(n // 3, 0.8), m.__setitem__(n - 1 - n // 4, 0.8)))
    put(3, lambda m: m.copy_(-m - 0.1))
    put(4, lambda m: (m.copy_(-m - 0.1), m.__setitem__(n // 2, 0.0)))
    put(5, lambda m: m.__setitem__(n // 5, 0.75))
    put(6, lambda m: m.__setitem__(n // 7, 0.7500001))
    return hm
