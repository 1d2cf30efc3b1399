"""CPU restatement of the person detector's mask branch (torchvision 0.7.0's RoIHeads mask path, MaskRCNNPredictor,
maskrcnn_inference and paste_masks_in_image as the issue describes them), on top of the unchanged tests/detector_scenario.py: written
from that description and not from the device code, and never run against torchvision either.  The chain uses torch's CPU
``F.conv2d`` / ``F.conv_transpose2d`` / ``F.interpolate`` and computes in the dtype of its inputs (float64: the oracle; float32: e_cpu32
of the rule  err <= 4 max(e_cpu32, 2^-23 max|y64|)).  ``paste_explicit`` is a second, per-pixel statement of the paste from the
formula in include/hps.h; ``expand_and_truncate`` is the float32 box arithmetic, one rounded operation at a time.
"""
import torch
import torch.nn.functional as F

import detector_scenario as S

BINS, SIZE, PAD = 14, 28, 1
SCALE = float(SIZE + 2 * PAD) / SIZE


# ---- mask head and predictor -----------------------------------------------------------------------------------------------------
def mask_head(roi, sd):
    """roi (n, 256, 14, 14) -> (n, 256, 14, 14): four 3x3 / pad 1 layers, each followed by ReLU."""
    x = roi
    for i in range(1, 5):
        p = "roi_heads.mask_head.mask_fcn%d" % i
        x = F.relu(F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], padding=1))
    return x


def upsample(x, sd):
    """ConvTranspose2d(256, 256, 2, 2) without the ReLU: (n, 256, 14, 14) -> (n, 256, 28, 28)."""
    p = "roi_heads.mask_predictor.conv5_mask"
    return F.conv_transpose2d(x, sd[p + ".weight"], sd[p + ".bias"], stride=2)


def upsample_as_products(x, sd):
    """The same as four 1x1 products: out[:, co, 2 y + dy, 2 x + dx] = b[co] + sum_ci x[:, ci, y, x] W[ci, co, dy, dx]."""
    p = "roi_heads.mask_predictor.conv5_mask"
    W, b = sd[p + ".weight"], sd[p + ".bias"]
    n, _, h, w = x.shape
    out = torch.zeros(n, W.shape[1], 2 * h, 2 * w, dtype=x.dtype)
    for dy in range(2):
        for dx in range(2):
            out[:, :, dy::2, dx::2] = torch.einsum("nchw,cd->ndhw", x, W[:, :, dy, dx]) + b[None, :, None, None]
    return out


def mask_logits(x, sd, labels):
    """features (n, 256, 14, 14), labels (n,) -> the pre-sigmoid mask of each row's own class (n, 28, 28)."""
    p = "roi_heads.mask_predictor.mask_fcn_logits"
    all_classes = F.conv2d(F.relu(upsample(x, sd)), sd[p + ".weight"], sd[p + ".bias"])
    return all_classes[torch.arange(x.shape[0]), labels]


# ---- paste -----------------------------------------------------------------------------------------------------------------------
def expand_and_truncate(boxes):
    """boxes (n, 4) -> int64 (n, 4) x0 y0 x1 y1: expand_boxes by float32(30 / 28) about the centre on float32 tensors, every operation
    rounded once, then the conversion to int64 (toward zero)."""
    b = boxes.float()
    w_half, h_half = (b[:, 2] - b[:, 0]) * 0.5, (b[:, 3] - b[:, 1]) * 0.5
    x_c, y_c = (b[:, 2] + b[:, 0]) * 0.5, (b[:, 3] + b[:, 1]) * 0.5
    w_half, h_half = w_half * SCALE, h_half * SCALE          # a Python scalar times a float32 tensor: the scalar becomes float32
    assert w_half.dtype == torch.float32
    return torch.stack([x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half], dim=1).to(torch.int64)


def rectangle(ibox, H, W):
    """(x range, y range) written for an integer box: [max(x0, 0), min(x1 + 1, W)) x [max(y0, 0), min(y1 + 1, H))."""
    x0, y0, x1, y1 = (int(v) for v in ibox)
    return (max(x0, 0), min(x1 + 1, W)), (max(y0, 0), min(y1 + 1, H))


def paste(probs, iboxes, H, W):
    """probs (n, 28, 28), iboxes (n, 4) int64 -> (n, H, W) in probs' dtype, through F.interpolate."""
    out = torch.zeros(probs.shape[0], H, W, dtype=probs.dtype)
    for k in range(probs.shape[0]):
        x0, y0, x1, y1 = (int(v) for v in iboxes[k])
        w, h = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
        m = F.interpolate(F.pad(probs[k][None, None], (PAD,) * 4), size=(h, w), mode="bilinear", align_corners=False)[0, 0]
        (xa, xb), (ya, yb) = rectangle(iboxes[k], H, W)
        if xa < xb and ya < yb:
            out[k, ya:yb, xa:xb] = m[ya - y0:yb - y0, xa - x0:xb - x0]
    return out


def paste_explicit(probs, iboxes, H, W):
    """The same, pixel by pixel in Python floats (float64) from the formula in include/hps.h."""
    n = probs.shape[0]
    out = torch.zeros(n, H, W, dtype=torch.float64)
    S30 = SIZE + 2 * PAD
    for k in range(n):
        m = [[0.0] * S30 for _ in range(S30)]
        rows = probs[k].double().tolist()
        for i in range(SIZE):
            m[i + 1][1:SIZE + 1] = rows[i]
        x0, y0, x1, y1 = (int(v) for v in iboxes[k])
        w, h = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
        (xa, xb), (ya, yb) = rectangle(iboxes[k], H, W)

        def axis(j, size):
            f = max((j + 0.5) * (S30 / size) - 0.5, 0.0)
            lo = min(int(f), S30 - 1)
            return lo, min(lo + 1, S30 - 1), f - lo

        for y in range(ya, yb):
            i0, i1, ly = axis(y - y0, h)
            for x in range(xa, xb):
                j0, j1, lx = axis(x - x0, w)
                out[k, y, x] = (1 - ly) * ((1 - lx) * m[i0][j0] + lx * m[i0][j1]) + ly * ((1 - lx) * m[i1][j0] + lx * m[i1][j1])
    return out


PASTE_SIZES = ((23, 31), (1, 1))


def paste_boxes(H, W):
    """The kernel-alone boxes for an (H, W) image, named: inside, cut by each border, larger than the image, outside, zero width (and
    height: one pixel), and one whose expanded corner lies in (-1, 0)."""
    h, w = float(H), float(W)
    boxes = {"inside": [w * 0.25, h * 0.25, w * 0.6, h * 0.7], "left": [-w * 0.3, h * 0.2, w * 0.4, h * 0.6],
             "top": [w * 0.3, -h * 0.4, w * 0.7, h * 0.5], "right": [w * 0.5, h * 0.3, w * 1.4, h * 0.8],
             "bottom": [w * 0.2, h * 0.5, w * 0.6, h * 1.5], "larger": [-w * 0.5, -h * 0.25, w * 1.5, h * 1.75],
             "outside": [w * 2.0, h * 2.0, w * 3.0, h * 3.0], "zero": [w * 0.5, h * 0.5, w * 0.5, h * 0.5],
             "truncation": [0.0, 0.0, w * 0.75, h * 0.75]}
    return list(boxes), torch.tensor(list(boxes.values()), dtype=torch.float32)


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def mask_chain(images, sd, cfg):
    """S.detect and the mask branch in the dtype of ``images`` / ``sd``.  Per image a dict: ``rois`` (n, 4) the detections' boxes in
    resized pixels (the candidates the final cut kept, before the rescale), ``labels``, ``boxes`` (input pixels), ``roi`` (n, 256, 14,
    14), ``features``, ``pre`` (the transposed convolution's pre-activations), ``logits`` / ``probs`` (n, 28, 28), ``iboxes`` (the
    integer paste boxes from the float32 of ``boxes``), ``masks`` (n, H, W)."""
    results, _, inter = S.detect(images, sd, cfg)
    out = []
    for b, im in enumerate(images):
        a = inter["images"][b]
        _, cand = S.class_candidates(a["logits"], a["deltas"], a["proposals"], inter["sizes"][b])
        rr, cc = a["kept"]
        rois, labels = cand[rr, cc], results[b]["labels"]
        roi = S.roi_align([P[b] for P in inter["P"]], rois, bins=BINS)
        feats = mask_head(roi, sd)
        logits = mask_logits(feats, sd, labels)
        probs = torch.sigmoid(logits)
        iboxes = expand_and_truncate(results[b]["boxes"])
        H, W = im.shape[1:]
        out.append({"rois": rois, "labels": labels, "boxes": results[b]["boxes"], "roi": roi, "features": feats, "pre": upsample(feats, sd),
                    "logits": logits, "probs": probs, "iboxes": iboxes, "masks": paste(probs, iboxes, H, W)})
    return out


def cut_by_border(ibox, H, W):
    x0, y0, x1, y1 = (int(v) for v in ibox)
    return x0 < 0 or y0 < 0 or x1 + 1 > W or y1 + 1 > H
