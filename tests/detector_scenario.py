"""CPU restatement of the person detector's stages (Mask R-CNN's box path, torchvision 0.7.0 as the issue describes it), written from
that description and not from the device code: torch.nn.functional for the convolutions, explicit tensor code and loops for the
resize, the anchors, NMS and RoIAlign.  Every function computes in the dtype of its inputs: float64 is the oracle, the same code on
float32 tensors gives e_cpu32 of the project's error rule  err <= 4 max(e_cpu32, 2^-23 max|y64|).

Decision stages also return their MARGINS -- how far each decision was from going the other way: the score gap at a top-k cut, the
least |IoU - thresh| over the pairs NMS compared, the least |score - thresh|, the gap to the small-box limit, the distance of the level
mapper's argument from an integer.  This restatement has never been run against torchvision either.
"""
import math

import torch
import torch.nn.functional as F

TINY = dict(num_classes=3, min_size=64, max_size=96, rpn_pre_nms_top_n_test=50, rpn_post_nms_top_n_test=30, box_detections_per_img=10)
DEFAULTS = dict(num_classes=91, min_size=800, max_size=1333, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225),
                rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, box_score_thresh=0.05, box_nms_thresh=0.5,
                box_detections_per_img=100, frozen_bn_eps=0.0)
LEVEL_SIZES = (32, 64, 128, 256, 512)
SEED = 1                    # the committed seed of the end-to-end test (test_detector_scenario_host.py checks its preconditions)
CLAMP = math.log(1000.0 / 16.0)
INF = float("inf")


def config(**kw):
    return dict(DEFAULTS, **kw)


# ---- the released file's keys -------------------------------------------------------------------------------------------------------
def expected_keys(num_classes=91):
    """{key: shape} of maskrcnn_resnet50_fpn_coco as the issue lists it."""
    keys = {}

    def bn(p, c):
        for n in ("weight", "bias", "running_mean", "running_var"):
            keys["%s.%s" % (p, n)] = (c,)

    body = "backbone.body"
    keys[body + ".conv1.weight"] = (64, 3, 7, 7)
    bn(body + ".bn1", 64)
    inplanes = 64
    for li, (planes, blocks) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), 1):
        for b in range(blocks):
            p = "%s.layer%d.%d" % (body, li, b)
            keys[p + ".conv1.weight"] = (planes, inplanes, 1, 1)
            bn(p + ".bn1", planes)
            keys[p + ".conv2.weight"] = (planes, planes, 3, 3)
            bn(p + ".bn2", planes)
            keys[p + ".conv3.weight"] = (planes * 4, planes, 1, 1)
            bn(p + ".bn3", planes * 4)
            if b == 0:
                keys[p + ".downsample.0.weight"] = (planes * 4, inplanes, 1, 1)
                bn(p + ".downsample.1", planes * 4)
            inplanes = planes * 4

    def conv(p, cout, cin, k):
        keys[p + ".weight"], keys[p + ".bias"] = (cout, cin, k, k), (cout,)

    def fc(p, cout, cin):
        keys[p + ".weight"], keys[p + ".bias"] = (cout, cin), (cout,)

    for i, c in enumerate((256, 512, 1024, 2048)):
        conv("backbone.fpn.inner_blocks.%d" % i, 256, c, 1)
        conv("backbone.fpn.layer_blocks.%d" % i, 256, 256, 3)
    conv("rpn.head.conv", 256, 256, 3)
    conv("rpn.head.cls_logits", 3, 256, 1)
    conv("rpn.head.bbox_pred", 12, 256, 1)
    fc("roi_heads.box_head.fc6", 1024, 256 * 7 * 7)
    fc("roi_heads.box_head.fc7", 1024, 1024)
    fc("roi_heads.box_predictor.cls_score", num_classes, 1024)
    fc("roi_heads.box_predictor.bbox_pred", 4 * num_classes, 1024)
    for i in range(1, 5):
        conv("roi_heads.mask_head.mask_fcn%d" % i, 256, 256, 3)
    conv("roi_heads.mask_predictor.conv5_mask", 256, 256, 2)            # ConvTranspose2d: (in, out, 2, 2)
    conv("roi_heads.mask_predictor.mask_fcn_logits", num_classes, 256, 1)
    return keys


def make_weights(seed, num_classes):
    """A seeded random state dict (float32 values, every bias non-zero): fan-in scaled filters, BatchNorm statistics away from the
    identity, and output layers wide enough that the random detector makes confident, well separated decisions."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in expected_keys(num_classes).items():
        leaf = key.rsplit(".", 1)[1]
        if leaf == "weight" and len(shape) == 1:
            v = 0.6 + 0.8 * torch.rand(shape, generator=g, dtype=torch.float64)
        elif leaf == "running_var":
            v = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif leaf in ("bias", "running_mean"):
            v = 0.2 * torch.randn(shape, generator=g, dtype=torch.float64)
        else:
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            v = torch.randn(shape, generator=g, dtype=torch.float64) * math.sqrt(2.0 / fan_in)
        if key.endswith("bn3.weight"):                      # the residual branch stays small: sixteen blocks do not blow the maps up
            v = v * 0.2
        if key.startswith("rpn.head.bbox_pred") and leaf == "weight":         # deltas of order 1: boxes that move but stay in the image
            v = v * 0.02
        if key.startswith("rpn.head.cls_logits") and leaf == "weight":
            v = v * 0.1
        if key.startswith("roi_heads.box_predictor") and leaf == "weight":
            v = v * 0.3
        sd[key] = v.float()
    return sd


def scenario_inputs(seed, sizes=((50, 37), (48, 80)), num_classes=TINY["num_classes"]):
    """The tests' seeded images ((3, H, W) float32 in [0, 1]) and weights."""
    g = torch.Generator().manual_seed(seed + 1000)
    return [torch.rand(3, h, w, generator=g, dtype=torch.float32) for h, w in sizes], make_weights(seed, num_classes)


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


# ---- 1. transform -----------------------------------------------------------------------------------------------------------------
def resized_size(H, W, cfg):
    s = cfg["min_size"] / min(H, W)
    if max(H, W) * s > cfg["max_size"]:
        s = cfg["max_size"] / max(H, W)
    return int(math.floor(H * s)), int(math.floor(W * s))


def resize_bilinear(x, oh, ow):
    """(C, H, W) -> (C, oh, ow), bilinear, align_corners = False: source = (dst + 0.5) (in / out) - 0.5 held to >= 0, indices held
    to <= in - 1."""
    _, H, W = x.shape

    def axis(n_in, n_out):
        src = (torch.arange(n_out, dtype=x.dtype) + 0.5) * (n_in / n_out) - 0.5
        src = src.clamp(min=0)
        i0 = src.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        return i0, i1, src - i0.to(x.dtype)

    y0, y1, ly = axis(H, oh)
    x0, x1, lx = axis(W, ow)
    ly, lx = ly[None, :, None], lx[None, None, :]
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return top * (1 - ly) + bot * ly


def transform(images, cfg):
    """[(3, H, W)] -> (batch (B, 3, FH, FW), [(oh, ow)]): normalise, resize, place top-left in a zero frame of multiples of 32."""
    dt = images[0].dtype
    mean = torch.tensor(cfg["image_mean"], dtype=dt)[:, None, None]
    std = torch.tensor(cfg["image_std"], dtype=dt)[:, None, None]
    out, sizes = [], []
    for im in images:
        oh, ow = resized_size(im.shape[1], im.shape[2], cfg)
        out.append(resize_bilinear((im - mean) / std, oh, ow))
        sizes.append((oh, ow))
    FH = (max(s[0] for s in sizes) + 31) // 32 * 32
    FW = (max(s[1] for s in sizes) + 31) // 32 * 32
    batch = torch.zeros(len(images), 3, FH, FW, dtype=dt)
    for b, t in enumerate(out):
        batch[b, :, :t.shape[1], :t.shape[2]] = t
    return batch, sizes


# ---- 2. backbone and FPN ----------------------------------------------------------------------------------------------------------
def _bn(x, sd, p, eps):
    scale = sd[p + ".weight"] * torch.rsqrt(sd[p + ".running_var"] + eps)
    shift = sd[p + ".bias"] - sd[p + ".running_mean"] * scale
    return x * scale[None, :, None, None] + shift[None, :, None, None]


def backbone(x, sd, cfg):
    """(B, 3, FH, FW) -> [C2, C3, C4, C5] (NCHW): ResNet-50 with the stride on the 3x3, frozen statistics."""
    eps, body = cfg["frozen_bn_eps"], "backbone.body"
    x = F.relu(_bn(F.conv2d(x, sd[body + ".conv1.weight"], stride=2, padding=3), sd, body + ".bn1", eps))
    x = F.max_pool2d(x, 3, 2, 1)
    outs = []
    for li, blocks in enumerate((3, 4, 6, 3), 1):
        for b in range(blocks):
            p = "%s.layer%d.%d" % (body, li, b)
            stride = 2 if (b == 0 and li > 1) else 1
            idt = x
            y = F.relu(_bn(F.conv2d(x, sd[p + ".conv1.weight"]), sd, p + ".bn1", eps))
            y = F.relu(_bn(F.conv2d(y, sd[p + ".conv2.weight"], stride=stride, padding=1), sd, p + ".bn2", eps))
            y = _bn(F.conv2d(y, sd[p + ".conv3.weight"]), sd, p + ".bn3", eps)
            if b == 0:
                idt = _bn(F.conv2d(x, sd[p + ".downsample.0.weight"], stride=stride), sd, p + ".downsample.1", eps)
            x = F.relu(y + idt)
        outs.append(x)
    return outs


def fpn(Cs, sd):
    """[C2..C5] -> ([P2..P5], pool): no ReLU anywhere."""
    p = "backbone.fpn."
    inner = lambda k, x: F.conv2d(x, sd[p + "inner_blocks.%d.weight" % k], sd[p + "inner_blocks.%d.bias" % k])
    layer = lambda k, x: F.conv2d(x, sd[p + "layer_blocks.%d.weight" % k], sd[p + "layer_blocks.%d.bias" % k], padding=1)
    t = inner(3, Cs[3])
    Ps = [layer(3, t)]
    for k in (2, 1, 0):
        t = inner(k, Cs[k]) + t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        Ps.insert(0, layer(k, t))
    return Ps, Ps[3][:, :, ::2, ::2]


# ---- 3. RPN -----------------------------------------------------------------------------------------------------------------------
def rpn_head(maps, sd):
    """Five NCHW maps -> per level (logits (B, h, w, 3), deltas (B, h, w, 12)) in NHWC order: delta channel a * 4 + k."""
    out = []
    for m in maps:
        t = F.relu(F.conv2d(m, sd["rpn.head.conv.weight"], sd["rpn.head.conv.bias"], padding=1))
        lg = F.conv2d(t, sd["rpn.head.cls_logits.weight"], sd["rpn.head.cls_logits.bias"])
        dl = F.conv2d(t, sd["rpn.head.bbox_pred.weight"], sd["rpn.head.bbox_pred.bias"])
        out.append((lg.permute(0, 2, 3, 1).contiguous(), dl.permute(0, 2, 3, 1).contiguous()))
    return out


def base_anchors(size, dtype=torch.float64):
    out = []
    for r in (0.5, 1.0, 2.0):
        hr = math.sqrt(r)
        wr = 1.0 / hr
        out.append([round(-wr * size / 2), round(-hr * size / 2), round(wr * size / 2), round(hr * size / 2)])
    return torch.tensor(out, dtype=dtype)


def anchors(size, h, w, stride_h, stride_w, dtype=torch.float64):
    """(h * w * 3, 4), ordered (y, x, a)."""
    base = base_anchors(size, dtype)
    ys = torch.arange(h, dtype=dtype) * stride_h
    xs = torch.arange(w, dtype=dtype) * stride_w
    shift = torch.stack([xs[None, :].expand(h, w), ys[:, None].expand(h, w), xs[None, :].expand(h, w), ys[:, None].expand(h, w)], dim=2)
    return (shift[:, :, None, :] + base[None, None, :, :]).reshape(-1, 4)


def decode(deltas, boxes, weights):
    """BoxCoder.decode: deltas (n, 4) / weights, dw and dh held to <= log(1000 / 16)."""
    w, h = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cx, cy = boxes[:, 0] + 0.5 * w, boxes[:, 1] + 0.5 * h
    dx, dy = deltas[:, 0] / weights[0], deltas[:, 1] / weights[1]
    dw, dh = (deltas[:, 2] / weights[2]).clamp(max=CLAMP), (deltas[:, 3] / weights[3]).clamp(max=CLAMP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = torch.exp(dw) * w, torch.exp(dh) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], dim=1)


def clip(boxes, size):
    h, w = size
    return torch.stack([boxes[:, 0].clamp(0, w), boxes[:, 1].clamp(0, h), boxes[:, 2].clamp(0, w), boxes[:, 3].clamp(0, h)], dim=1)


def _cut_gap(sorted_scores, k):
    """Gap between the last score inside a top-k cut and the first one outside (inf when nothing is cut)."""
    if k <= 0 or k >= sorted_scores.numel():
        return INF
    return float(sorted_scores[k - 1] - sorted_scores[k])


def rpn_level(logits, deltas, anc, k, size, min_size=1e-3):
    """One image, one level: logits (h w 3,), deltas (h w 3, 4) -> (top-k indices, boxes (k, 4), valid (k,), scores (k,), margins)."""
    k = min(k, logits.numel())
    order = torch.argsort(logits, descending=True, stable=True)
    idx = order[:k]
    boxes = clip(decode(deltas[idx], anc[idx], (1.0, 1.0, 1.0, 1.0)), size)
    ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    valid = (ws >= min_size) & (hs >= min_size)
    return idx, boxes, valid, logits[idx], {"topk": _cut_gap(logits[order], k), "small": _small_gap(ws, hs, min_size)}


def iou_pair(a, b):
    iw = (torch.minimum(a[2], b[2]) - torch.maximum(a[0], b[0])).clamp(min=0)
    ih = (torch.minimum(a[3], b[3]) - torch.maximum(a[1], b[1])).clamp(min=0)
    inter = iw * ih
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter)


def nms(boxes, scores, thresh, trace=None):
    """Greedy NMS of ONE category: kept indices by descending score, and the least |IoU - thresh| over the compared pairs (a kept box
    against every later box still alive; a 0 / 0 IoU suppresses nothing and has no margin).  ``trace``: a list that receives every
    compared IoU in order."""
    order = torch.argsort(scores, descending=True, stable=True).tolist()
    alive = [True] * len(order)
    keep, margin = [], INF
    for p, i in enumerate(order):
        if not alive[p]:
            continue
        keep.append(i)
        for q in range(p + 1, len(order)):
            if not alive[q]:
                continue
            v = float(iou_pair(boxes[i], boxes[order[q]]))
            if v != v:
                continue
            if trace is not None:
                trace.append(v)
            margin = min(margin, abs(v - thresh))
            if v > thresh:
                alive[q] = False
    return keep, margin


def nms_brute(boxes, scores, thresh):
    """O(n^2) definition: box i (by descending score) is kept iff no KEPT earlier box overlaps it by more than thresh."""
    order = torch.argsort(scores, descending=True, stable=True).tolist()
    keep = []
    for i in order:
        if all(not (float(iou_pair(boxes[j], boxes[i])) > thresh) for j in keep):
            keep.append(i)
    return keep


def nms_per_category(boxes, scores, cats, thresh, trace=None):
    keep, margin = [], INF
    for c in sorted(set(cats.tolist())):
        sel = torch.nonzero(cats == c)[:, 0]
        k, m = nms(boxes[sel], scores[sel], thresh, trace)
        keep += sel[k].tolist()
        margin = min(margin, m)
    keep.sort(key=lambda i: -float(scores[i]))
    return keep, margin


def _small_gap(ws, hs, min_size):
    """Least distance of a side from the small-box limit.  A side that is exactly 0 is left out: both of its ends were clipped to the
    same edge of the image, which gives exactly 0 in every precision."""
    d = torch.cat([ws[ws != 0], hs[hs != 0]])
    return float((d - min_size).abs().min()) if d.numel() else INF


def rpn_image(levels, frame, size, cfg, trace=None):
    """One image: levels = [(logits (h, w, 3), deltas (h, w, 12))] -> (proposals (n, 4), their logits (n,), margins, per-level parts)."""
    FH, FW = frame
    boxes, scores, margins, parts = [], [], {"topk": INF, "small": INF, "iou": INF}, []
    for l, (lg, dl) in enumerate(levels):
        h, w, _ = lg.shape
        anc = anchors(LEVEL_SIZES[l], h, w, FH // h, FW // w, lg.dtype)
        idx, bx, valid, sc, m = rpn_level(lg.reshape(-1), dl.reshape(-1, 4), anc, cfg["rpn_pre_nms_top_n_test"], size)
        vb, vs = bx[valid], sc[valid]
        keep, miou = nms(vb, vs, cfg["rpn_nms_thresh"], trace)
        parts.append({"idx": idx, "boxes": bx, "valid": valid, "scores": sc, "keep": torch.nonzero(valid)[:, 0][keep]})
        boxes.append(vb[keep])
        scores.append(vs[keep])
        margins["topk"], margins["small"], margins["iou"] = min(margins["topk"], m["topk"]), min(margins["small"], m["small"]), min(margins["iou"], miou)
    boxes, scores = torch.cat(boxes), torch.cat(scores)
    order = torch.argsort(scores, descending=True, stable=True)
    n = cfg["rpn_post_nms_top_n_test"]
    margins["post"] = _cut_gap(scores[order], n)
    return boxes[order[:n]], scores[order[:n]], margins, parts


# ---- 4. multi-scale RoIAlign ------------------------------------------------------------------------------------------------------
def level_argument(boxes):
    """4 + log2(sqrt(area) / 224 + 1e-6): its floor, held to [2, 5], minus 2 is the level."""
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return 4 + torch.log2(torch.sqrt(area) / 224 + 1e-6)


def level_of(boxes):
    arg = level_argument(boxes)
    return (arg.floor().clamp(2, 5) - 2).long(), float((arg - arg.round()).abs().min()) if boxes.shape[0] else INF


def _bilinear(f, y, x):
    """f (C, H, W) at (y, x) by the RoIAlign rule."""
    C, H, W = f.shape
    if y < -1.0 or y > H or x < -1.0 or x > W:
        return torch.zeros(C, dtype=f.dtype)
    y, x = max(y, 0.0), max(x, 0.0)
    yl, xl = int(y), int(x)
    if yl >= H - 1:
        yh = yl = H - 1
        y = float(yl)
    else:
        yh = yl + 1
    if xl >= W - 1:
        xh = xl = W - 1
        x = float(xl)
    else:
        xh = xl + 1
    ly, lx = y - yl, x - xl
    hy, hx = 1.0 - ly, 1.0 - lx
    return hy * hx * f[:, yl, xl] + hy * lx * f[:, yl, xh] + ly * hx * f[:, yh, xl] + ly * lx * f[:, yh, xh]


def roi_align(levels, boxes, bins=7):
    """levels = [P2..P5] of ONE image, each (C, h, w); boxes (n, 4) -> (n, C, bins, bins).  Scalar geometry in the boxes' dtype."""
    lv, _ = level_of(boxes)
    dt = boxes.dtype
    out = torch.zeros(boxes.shape[0], levels[0].shape[0], bins, bins, dtype=levels[0].dtype)
    for r in range(boxes.shape[0]):
        f = levels[int(lv[r])]
        scale = torch.tensor(1.0 / (4 << int(lv[r])), dtype=dt)
        x1, y1 = boxes[r, 0] * scale, boxes[r, 1] * scale
        rw = torch.clamp(boxes[r, 2] * scale - x1, min=1.0)
        rh = torch.clamp(boxes[r, 3] * scale - y1, min=1.0)
        bw, bh = rw / bins, rh / bins
        for ph in range(bins):
            for pw in range(bins):
                acc = torch.zeros(f.shape[0], dtype=f.dtype)
                for iy in range(2):
                    for ix in range(2):
                        yy = y1 + ph * bh + (iy + 0.5) * bh / 2
                        xx = x1 + pw * bw + (ix + 0.5) * bw / 2
                        acc = acc + _bilinear(f, float(yy), float(xx))
                out[r, :, ph, pw] = acc / 4
    return out


# ---- 5. box head and post-processing ---------------------------------------------------------------------------------------------
def box_head(roi, sd):
    """roi (n, 256, 7, 7), flattened (c, ph, pw) -> (class logits (n, NC), deltas (n, 4 NC))."""
    p = "roi_heads."
    x = F.relu(F.linear(roi.flatten(1), sd[p + "box_head.fc6.weight"], sd[p + "box_head.fc6.bias"]))
    x = F.relu(F.linear(x, sd[p + "box_head.fc7.weight"], sd[p + "box_head.fc7.bias"]))
    return (F.linear(x, sd[p + "box_predictor.cls_score.weight"], sd[p + "box_predictor.cls_score.bias"]),
            F.linear(x, sd[p + "box_predictor.bbox_pred.weight"], sd[p + "box_predictor.bbox_pred.bias"]))


def class_candidates(logits, deltas, props, size):
    """Soft-max and the per-class decode: (probs (n, NC), boxes (n, NC, 4) clipped to the resized image)."""
    n, NC = logits.shape
    probs = F.softmax(logits, dim=1)
    boxes = torch.stack([clip(decode(deltas[:, 4 * c:4 * c + 4], props, (10.0, 10.0, 5.0, 5.0)), size) for c in range(NC)], dim=1)
    return probs, boxes


def postprocess(logits, deltas, props, size, orig, cfg, min_size=1e-2, trace=None):
    """One image -> (boxes (m, 4) in the input's pixels, labels (m,), scores (m,), margins, (candidate index pairs kept))."""
    probs, boxes = class_candidates(logits, deltas, props, size)
    n, NC = probs.shape
    rr, cc = torch.meshgrid(torch.arange(n), torch.arange(1, NC), indexing="ij")
    rr, cc = rr.reshape(-1), cc.reshape(-1)
    sc, bx = probs[rr, cc], boxes[rr, cc]
    margins = {"score": float((sc - cfg["box_score_thresh"]).abs().min()) if sc.numel() else INF}
    sel = sc > cfg["box_score_thresh"]
    rr, cc, sc, bx = rr[sel], cc[sel], sc[sel], bx[sel]
    ws, hs = bx[:, 2] - bx[:, 0], bx[:, 3] - bx[:, 1]
    margins["small"] = _small_gap(ws, hs, min_size)
    sel = (ws >= min_size) & (hs >= min_size)
    rr, cc, sc, bx = rr[sel], cc[sel], sc[sel], bx[sel]
    keep, margins["iou"] = nms_per_category(bx, sc, cc, cfg["box_nms_thresh"], trace)
    D = cfg["box_detections_per_img"]
    margins["topk"] = _cut_gap(sc[keep], D)
    keep = keep[:D]
    dt = bx.dtype
    ratio_h = torch.tensor(float(orig[0]), dtype=torch.float32) / torch.tensor(float(size[0]), dtype=torch.float32)
    ratio_w = torch.tensor(float(orig[1]), dtype=torch.float32) / torch.tensor(float(size[1]), dtype=torch.float32)
    out = bx[keep] * torch.stack([ratio_w, ratio_h, ratio_w, ratio_h]).to(dt)
    return out, cc[keep], sc[keep], margins, (rr[keep], cc[keep])


def rule(err32, ymax):
    """The project's bound: 4 max(e_cpu32, 2^-23 max|y64|)."""
    return 4.0 * max(float(err32), 2.0 ** -23 * float(ymax))


def chain_preconditions(images, sd, cfg, min_detections=3, factor=8.0):
    """The end-to-end test's preconditions, all on the CPU: the float64 chain and the same chain on float32 tensors.  Returns
    (float64 results, intermediates, bounds, problems): ``bounds`` holds the rule's bound per family, measured between the two chains;
    ``problems`` lists every violated precondition -- fewer than ``min_detections`` detections, a float32 chain that decides otherwise,
    or a margin below ``factor`` bounds.  Margins and their bounds: score gaps (RPN top-k and the cut across levels) against the
    objectness logits' bound; the class-score threshold and the final cut against the probabilities' bound; the small-box gaps against
    the boxes' bound (proposal candidates, class candidates); |IoU - thresh| against the bound of the compared IoUs themselves; the
    level mapper's argument against its own bound."""
    r64, m64, i64 = detect([im.double() for im in images], cast(sd, torch.float64), cfg)
    r32, m32, i32 = detect([im.float() for im in images], cast(sd, torch.float32), cfg)
    problems, bounds = [], []
    d = lambda a, b: float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
    top = lambda a: float(a.abs().max()) if a.numel() else 0.0
    for b in range(len(images)):
        a64, a32 = i64["images"][b], i32["images"][b]
        same = (r64[b]["labels"].tolist() == r32[b]["labels"].tolist() and a64["proposals"].shape == a32["proposals"].shape
                and len(a64["ious"]) == len(a32["ious"]) and all(torch.equal(p["idx"], q["idx"]) and torch.equal(p["keep"], q["keep"])
                                                                  for p, q in zip(a64["rpn_parts"], a32["rpn_parts"])))
        if not same:
            problems.append("image %d: the float32 chain decides otherwise" % b)
            bounds.append(None)
            continue
        if len(r64[b]["scores"]) < min_detections:
            problems.append("image %d: %d detections" % (b, len(r64[b]["scores"])))
        lg64 = torch.cat([lg[b].reshape(-1) for lg, _ in i64["rpn"]])
        lg32 = torch.cat([lg[b].reshape(-1) for lg, _ in i32["rpn"]])
        cand64 = torch.cat([p["boxes"] for p in a64["rpn_parts"]])
        cand32 = torch.cat([p["boxes"] for p in a32["rpn_parts"]])
        size = i64["sizes"][b]
        p64, c64 = class_candidates(a64["logits"], a64["deltas"], a64["proposals"], size)
        p32, c32 = class_candidates(a32["logits"], a32["deltas"], a32["proposals"], size)
        arg64, arg32 = level_argument(a64["proposals"]), level_argument(a32["proposals"])
        io64, io32 = torch.tensor(a64["ious"], dtype=torch.float64), torch.tensor(a32["ious"], dtype=torch.float64)
        bd = {"logit": rule(d(lg64, lg32), top(lg64)), "prob": rule(d(p64, p32), 1.0), "rpn_box": rule(d(cand64, cand32), max(size)),
              "class_box": rule(d(c64, c32), max(size)), "iou": rule(d(io64, io32), 1.0), "level": rule(d(arg64, arg32), top(arg64)),
              "final_box": rule(d(r64[b]["boxes"], r32[b]["boxes"]), max(images[b].shape[1:])),
              "final_score": rule(d(r64[b]["scores"], r32[b]["scores"]), 1.0)}
        bounds.append(bd)
        m = m64[b]
        for name, margin, bound in (("rpn top-k", m["rpn"]["topk"], bd["logit"]), ("rpn cut across levels", m["rpn"]["post"], bd["logit"]),
                                    ("rpn small box", m["rpn"]["small"], bd["rpn_box"]), ("rpn IoU", m["rpn"]["iou"], bd["iou"]),
                                    ("level", m["level"], bd["level"]), ("class score", m["box"]["score"], bd["prob"]),
                                    ("class small box", m["box"]["small"], bd["class_box"]), ("class IoU", m["box"]["iou"], bd["iou"]),
                                    ("final cut", m["box"]["topk"], bd["prob"])):
            if not margin >= factor * bound:
                problems.append("image %d: %s margin %.3g < %g x %.3g" % (b, name, margin, factor, bound))
    return r64, i64, bounds, problems


# ---- the chain --------------------------------------------------------------------------------------------------------------------
def detect(images, sd, cfg):
    """The whole chain in the dtype of ``images`` / ``sd``: per image {"boxes", "labels", "scores"}, the margins of every decision
    stage, and the intermediates."""
    batch, sizes = transform(images, cfg)
    Cs = backbone(batch, sd, cfg)
    Ps, pool = fpn(Cs, sd)
    heads = rpn_head(Ps + [pool], sd)
    frame = (batch.shape[2], batch.shape[3])
    results, margins, inter = [], [], {"batch": batch, "sizes": sizes, "C": Cs, "P": Ps, "pool": pool, "rpn": heads, "images": []}
    for b, im in enumerate(images):
        ious = []
        props, pscores, m_rpn, parts = rpn_image([(lg[b], dl[b]) for lg, dl in heads], frame, sizes[b], cfg, ious)
        _, m_level = level_of(props)
        roi = roi_align([P[b] for P in Ps], props)
        logits, deltas = box_head(roi, sd)
        boxes, labels, scores, m_box, kept = postprocess(logits, deltas, props, sizes[b], (im.shape[1], im.shape[2]), cfg, trace=ious)
        results.append({"boxes": boxes, "labels": labels, "scores": scores})
        margins.append({"rpn": m_rpn, "level": m_level, "box": m_box})
        inter["images"].append({"proposals": props, "proposal_scores": pscores, "rpn_parts": parts, "roi": roi, "logits": logits,
                                "deltas": deltas, "kept": kept, "ious": ious})
    return results, margins, inter
