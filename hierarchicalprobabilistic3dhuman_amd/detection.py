"""Person detector: Mask R-CNN with a ResNet-50-FPN backbone (its box path, and opt-in its mask branch), the detector the reference builds with
``torchvision.models.detection.maskrcnn_resnet50_fpn(pretrained=True)`` (run_predict.py:43) and reads in one place
(predict/predict_hrnet.py:52-57: ``boxes``, ``labels``, ``scores``).  Module tree and state-dict keys are those of the released
``maskrcnn_resnet50_fpn_coco`` file (strict loading; the later torchvision spelling ``inner_blocks.N.0.*`` / ``layer_blocks.N.0.*`` /
``rpn.head.conv.0.0.*`` is renamed on load, ``num_batches_tracked`` entries are dropped).

    detector = maskrcnn_resnet50_fpn().to("cuda")
    detector.load_state_dict(torch.load("maskrcnn_resnet50_fpn_coco.pth"))
    out = detector([image_a, image_b])        # (3, H, W) float32 device tensors in [0, 1], any sizes; or one (B, 3, H, W) tensor
    out[0]["boxes"], out[0]["labels"], out[0]["scores"]          # (n, 4) x1 y1 x2 y2 in the input's pixels, (n,) int64, (n,) descending
    out = detector([image_a, image_b], masks=True)               # opt-in: also out[0]["masks"], (n, 1, H, W) float32 probabilities
    out = detector([image_a, image_b], masks=True, mask_threshold=0.5)          # ... or (n, 1, H, W) uint8, probability > 0.5

THE SEMANTICS ARE A RESTATEMENT of torchvision 0.7.0 (the version the reference pins) written from its description; torchvision is
not part of this stack and this restatement HAS NEVER BEEN RUN AGAINST TORCHVISION.  tests/detector_scenario.py restates the same
stages in float64 on the CPU; the device code is held to that.

Eval mode only, no backward (an input that requires grad is refused, ``.train()`` is refused).  Without ``masks=True`` the mask branch
is held (its parameters load) and not computed: no ``masks`` key, and the call launches and allocates what the box path alone does.
Not here: training, keypoint R-CNN, other backbones.

THE MASK BRANCH (``masks=True``; the same caveat: restated from torchvision 0.7.0's description, never run against torchvision;
tests/detector_mask_scenario.py is its float64 restatement).  ``detections(..., with_rois=True)`` also returns the detections' boxes in
resized-image pixels -- the candidates hps_det_gather selects, before its rescale -- and their presence mark; ``mask_branch`` runs
hps_det_roi_align_halo (MultiScaleRoIAlign over P2..P5, 14 x 14, sampling ratio 2, the box head's level mapper) into zero-haloed frames,
the four 3x3 + ReLU layers over the B D maps of 14 x 14 on the wide kernel (K in slices of 256 products, frames and launch list cached
like the box head's), and hps_det_mask_predict: ConvTranspose2d(256, 256, 2, 2) + ReLU, the 1x1 logit of the detection's own class and
the sigmoid in one launch on the fp32 matrix instructions -- the (B D, 28, 28, 256) tensor (80 MB at 100 detections) is never written
and no other class's logit is formed.  ``forward`` pastes after its one synchronisation (hps_det_paste_masks: one launch per image that
writes every pixel of the n masks; torchvision's paste_masks_in_image with padding 1, probabilities, not thresholded).  100 float masks
of 720 x 960 take 276 MB; the uint8 form (``mask_threshold``) takes a quarter of that.  ``detect_padded(masks=True)`` returns the
(B, D, 28, 28) probabilities as a fifth tensor and does not synchronise.

Stages (public, ``forward`` is their composition): ``features`` (hps_det_transform writes the stem's input frame; the project's
ResNet-50 encoder with frozen statistics, tapped after layer1..4 by ``ResNet.stage_taps``; the FPN's laterals and 3x3 output layers on
the encoder's wide kernel, hps_hrnet_fuse for "nearest up-sample and add"), ``proposals`` (the RPN's 3x3 layer on the wide kernel, its
two 1x1 outputs as hps_conv2d_bn_act_c16 problems, per-level top-k, hps_det_rpn_decode, hps_det_nms per level, top-k across levels),
``box_head`` (hps_det_roi_align writes fc6's input in (bin, channel) order -- fc6's weight is permuted once to it -- and fc6 / fc7 run as
1x1 convolutions over a map of R boxes on the wide kernel, the two predictors on hps_conv2d_bn_act_c16), ``detections``
(hps_det_box_decode, per-class hps_det_nms, top-k, hps_det_gather).  The wide layers (Cin % 32 == 0, Cout % 64 == 0) sum K in slices
of 256 products (``_wide_layer``): summed in one run, the 2 304 products of a 3x3 layer left P2 outside the accuracy rule.
``torch.topk`` / ``torch.sort`` / ``gather`` order rows; all arithmetic is in the kernels.

Capacities are fixed by the constructor: at most ``rpn_pre_nms_top_n_test`` candidates per level, ``rpn_post_nms_top_n_test``
proposals and as many candidates per class (both at most 2048, the NMS kernel's LDS), ``box_detections_per_img`` detections.  Counts
stay on the device: an absent row has score -infinity and a zero box, and every later stage skips it.  THE ONE HOST SYNCHRONISATION
of ``forward`` is its last step, which reads the per-image counts to size the returned tensors; ``detect_padded`` returns the padded
tensors and the counts and does not synchronise.

An image's result does not depend on the images it is batched with as long as the batch's frame (the largest resized size rounded up
to 32) leaves every backbone layer on the kernel it has for the image alone; the backbone picks Winograd or direct kernels and split K
by the map size (resnet._ConvBN._route), so frames of another size may differ in the last bits.
"""
import ctypes
import math

import torch
from torch import nn

from . import _capi
from .device_state import DeviceStateModule
from .resnet import Bottleneck, ResNet, _ConvBN

_NEG_INF = float("-inf")
_LEVEL_SIZES = (32, 64, 128, 256, 512)
_RATIOS = (0.5, 1.0, 2.0)


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d with fixed statistics and affine parameters, all four as buffers (torchvision.ops.misc.FrozenBatchNorm2d);
    ``eps`` 0.0 in torchvision 0.7.0, 1e-5 later.  A parameter container: resnet._ConvBN.fold reads it."""

    def __init__(self, num_features, eps=0.0):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)


def _freeze_batchnorm(module, eps):
    for name, child in list(module.named_children()):
        if isinstance(child, nn.BatchNorm2d):
            setattr(module, name, FrozenBatchNorm2d(child.num_features, eps))
        else:
            _freeze_batchnorm(child, eps)


class _Layer16:
    """Kernel-side form of a convolution / FC layer with a bias for hps_conv2d_bn_act_c16: w (k * k, ceil16(Cout), Cin), scale 1,
    shift = bias."""

    def __init__(self, weight, bias):
        w = weight.detach().float()
        cout, cin, k, _ = w.shape
        assert cin % 16 == 0
        coutp = (cout + 15) // 16 * 16
        wk = torch.zeros(k, k, coutp, cin, device=w.device, dtype=torch.float32)
        wk[:, :, :cout] = w.permute(2, 3, 0, 1)
        self.w = wk.reshape(k * k, coutp, cin).contiguous()
        self.scale = torch.ones(cout, device=w.device, dtype=torch.float32)
        self.shift = bias.detach().float().contiguous().clone()
        self.cin, self.cout, self.k = cin, cout, k

    def problem(self, x, B, H, W, ipad, y, opad, relu):
        P = _capi.ptr
        return _capi.C16Problem(x=P(x), w=P(self.w), scale=P(self.scale), shift=P(self.shift), residual=None, y=P(y), B=B, H=H, W=W,
                                ipad=ipad, Cin=self.cin, Cout=self.cout, K=self.k, stride=1, opad=opad, relu=1 if relu else 0)


class _Bias:
    """A convolution's bias in the shape resnet._ConvBN.fold reads a BatchNorm: scale 1, shift = bias."""

    def __init__(self, conv):
        c, d = conv.out_channels, conv.weight.device
        self.weight, self.bias, self.eps = torch.ones(c, device=d), conv.bias, 0.0
        self.running_mean, self.running_var = torch.zeros(c, device=d), torch.ones(c, device=d)


class _AsConv:
    """A weight (Cout, Cin, k, k) and a bias in the shape resnet._ConvBN reads a convolution (an FC layer: k = 1)."""

    def __init__(self, weight, bias, pad):
        self.weight, self.bias, self.out_channels = weight, bias, weight.shape[0]
        self.stride, self.padding = (1, 1), (pad, pad)


def _wide_layer(weight, bias, pad):
    """A wide layer (Cin % 32 == 0, Cout % 64 == 0) on the encoder's direct kernel with K in slices of 256 products (8 chunks of 32)
    where the chunk count divides that way: a slice is summed in order and the slices are added in order, so an output's rounding error
    grows with the slice length and the slice count, not with K -- fc6 sums 12 544 products, the 3x3 layers 2 304.  The rule depends on
    the layer alone: an image has the same bits in every batch."""
    conv = _AsConv(weight, bias, pad)
    cb = _ConvBN(conv, _Bias(conv))
    chunks = cb.kh * cb.kw * cb.cin_p // 32
    cb.ksplit = chunks // 8 if chunks % 8 == 0 and chunks >= 16 else 1
    return cb


def _wide_ops(jobs, device):
    """[(resnet._ConvBN, input frame, input halo, output frame, output halo, relu)] -> (EncOp array, the scratch it points at): the wide
    3x3 layers (256 -> 256) on the encoder's kernels (csrc/conv_pad.hip, conv_wino.hip), routed by resnet._ConvBN."""
    ops, keep = [], []
    for cb, x, ipad, y, opad, relu in jobs:
        need = cb.workspace_bytes(x.shape[0], x.shape[1] - 2 * ipad, x.shape[2] - 2 * ipad, ipad)
        ws = torch.empty(need // 4, device=device, dtype=torch.float32) if need else None
        keep.append(ws)
        ops.append(cb.op(x, ipad, y, opad, relu=relu, ws=ws))
    return (_capi.EncOp * len(ops))(*ops), keep


def _conv_ops(problems):
    ops = []
    for i in range(0, len(problems), _capi.C16_MAX_PROBLEMS):
        group = problems[i:i + _capi.C16_MAX_PROBLEMS]
        op = _capi.HrnetOp(kind=_capi.HRNET_CONV, n_problems=len(group))
        for k, p in enumerate(group):
            op.conv[k] = p
        ops.append(op)
    return ops


def _run(ops):
    _capi.call("hps_hrnet_run", ops, len(ops), _capi.stream())


def resized_size(H, W, min_size, max_size):
    """GeneralizedRCNNTransform.resize's output size, in Python floats."""
    s = float(min_size) / float(min(H, W))
    if float(max(H, W)) * s > float(max_size):
        s = float(max_size) / float(max(H, W))
    return int(math.floor(H * s)), int(math.floor(W * s))


def base_anchors(size, ratios=_RATIOS):
    """AnchorGenerator.generate_anchors for one level: (A, 4) float32, round([-w, -h, w, h] / 2) in float32 arithmetic."""
    scales = torch.tensor([float(size)], dtype=torch.float32)
    r = torch.tensor(ratios, dtype=torch.float32)
    hr = torch.sqrt(r)
    wr = 1.0 / hr
    ws, hs = (wr[:, None] * scales[None, :]).view(-1), (hr[:, None] * scales[None, :]).view(-1)
    return (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()


def _set_sizes(field, sizes):
    for b, row in enumerate(sizes):
        for e, v in enumerate(row):
            field[b][e] = int(v)


def nms_groups(boxes, scores, thresh, order=None):
    """hps_det_nms: boxes (G, N, 4), scores (G, N) in descending order per group (-inf: absent), position i of group g being box
    ``order[g, i]`` (None: i) -> keep_scores (G, N): the score where kept, -inf elsewhere."""
    _capi.require_device(boxes, "boxes")
    G, N = scores.shape
    keep = torch.empty(G, N, device=boxes.device, dtype=torch.float32)
    if N > _capi.DET_NMS_MAX_BOXES:
        raise _capi.HpsError("nms: at most %d boxes per group, got %d" % (_capi.DET_NMS_MAX_BOXES, N))
    a = _capi.DetNmsArgs(struct_bytes=ctypes.sizeof(_capi.DetNmsArgs), G=G, N=N, thresh=float(thresh), boxes=_capi.ptr(boxes),
                         order=_capi.ptr(order, torch.int64) if order is not None else None, scores=_capi.ptr(scores), keep_scores=_capi.ptr(keep))
    _capi.call("hps_det_nms", ctypes.byref(a), _capi.stream())
    return keep


def nms_per_category(boxes, scores, categories, num_categories, thresh):
    """Per-category NMS of boxes (n, 4) with scores (n,) and categories (n,) in [0, num_categories): the kept indices by descending
    score.  The device kernel on a (category, position) layout; sorting and the scatter into it are torch plumbing."""
    _capi.require_device(boxes, "boxes")
    n = boxes.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    boxes, scores, categories = _capi.f32c(boxes), _capi.f32c(scores), categories.to(torch.int64)
    G, N = int(num_categories), n
    gb = torch.zeros(G, N, 4, device=boxes.device, dtype=torch.float32)
    gs = torch.full((G, N), _NEG_INF, device=boxes.device, dtype=torch.float32)
    col = torch.arange(n, device=boxes.device)
    gb[categories, col] = boxes
    gs[categories, col] = scores
    ss, order = torch.sort(gs, dim=1, descending=True)
    keep = nms_groups(gb, ss.contiguous(), thresh, order.contiguous())
    kept = keep > _NEG_INF
    idx, sc = order[kept], keep[kept]
    return idx[torch.argsort(sc, descending=True)]


def multiscale_roi_align(levels, boxes, scores=None, bins=7, halo=0):
    """hps_det_roi_align: ``levels`` = [(frame (B, h + 2 pad, w + 2 pad, C), pad, scale)] for P2.., boxes (B, R, 4), scores (B, R) or
    None (every box present) -> (B, R, bins * bins * C), (bin row, bin column, channel) order.  With ``halo`` > 0
    (hps_det_roi_align_halo): (B * R, bins + 2 halo, bins + 2 halo, C), the same values inside a border of zeros -- the input frames of
    a 3x3 layer over the boxes."""
    _capi.require_device(boxes, "boxes")
    boxes = _capi.f32c(boxes)
    B, R, _ = boxes.shape
    if scores is None:
        scores = torch.zeros(B, R, device=boxes.device, dtype=torch.float32)
    C = levels[0][0].shape[3]
    halo = int(halo)
    if halo:
        y = torch.empty(B * R, bins + 2 * halo, bins + 2 * halo, C, device=boxes.device, dtype=torch.float32)
    else:
        y = torch.empty(B, R, bins * bins * C, device=boxes.device, dtype=torch.float32)
    a = _capi.DetRoiAlignArgs(struct_bytes=ctypes.sizeof(_capi.DetRoiAlignArgs), B=B, R=R, C=C, bins=bins, n_levels=len(levels),
                              boxes=_capi.ptr(boxes), scores=_capi.ptr(scores), y=_capi.ptr(y))
    for l, (frame, pad, scale) in enumerate(levels):
        if frame.shape[0] != B or frame.shape[3] != C:
            raise _capi.HpsError("roi_align: level %d is %s; expected batch %d and %d channels" % (l, tuple(frame.shape), B, C))
        lv = a.level[l]
        lv.x, lv.h, lv.w, lv.pad, lv.scale = _capi.ptr(frame), frame.shape[1] - 2 * pad, frame.shape[2] - 2 * pad, pad, float(scale)
    if halo:
        _capi.call("hps_det_roi_align_halo", ctypes.byref(a), halo, _capi.stream())
    else:
        _capi.call("hps_det_roi_align", ctypes.byref(a), _capi.stream())
    return y


def _check_threshold(threshold):
    if threshold is not None and not 0.0 < float(threshold) < 1.0:
        raise ValueError("mask threshold %r: a probability strictly between 0 and 1 (None: the probabilities themselves)" % (threshold,))
    return None if threshold is None else float(threshold)


def mask_weights(conv5_weight):
    """hps_det_mask_predict's form of ConvTranspose2d(256, 256, 2, 2).weight (ci, co, dy, dx): (4, 128, 64, 8) with element
    [2 dy + dx][s][lane][t] = W[2 s + (lane >> 5)][32 t + (lane & 31)][dy][dx] -- a lane's eight row blocks are two 16-byte loads."""
    w = conv5_weight.detach().float()
    C = _capi.DET_MASK_CHANNELS
    if tuple(w.shape) != (C, C, 2, 2):
        raise _capi.HpsError("mask predictor: conv5_mask.weight is %s; expected (%d, %d, 2, 2)" % (tuple(w.shape), C, C))
    w = w.permute(2, 3, 0, 1).reshape(4, C // 2, 2, C // 32, 32)              # tap, s, h, t, i
    return w.permute(0, 1, 2, 4, 3).reshape(4, C // 2, 64, C // 32).contiguous()


def mask_predict(frames, weights, bias, logit_weight, logit_bias, labels, scores=None, with_logits=False):
    """hps_det_mask_predict: frames (K, 16, 16, 256) zero-haloed NHWC (the last mask-head layer's output), ``weights`` from
    mask_weights, bias (256,), logit_weight (NC, 256), logit_bias (NC,), labels (K,) int64, scores (K,) or None (every row present) ->
    (probs (K, 28, 28), logits (K, 28, 28) or None).  A row that is absent or has label 0 is zero."""
    _capi.require_device(frames, "frames")
    K, S, F, C = frames.shape[0], _capi.DET_MASK_SIZE, _capi.DET_MASK_BINS + 2, _capi.DET_MASK_CHANNELS
    NC = logit_weight.shape[0]
    if tuple(frames.shape) != (K, F, F, C) or tuple(weights.shape) != (4, C // 2, 64, C // 32) or tuple(bias.shape) != (C,) or \
            tuple(logit_weight.shape) != (NC, C) or tuple(logit_bias.shape) != (NC,) or tuple(labels.shape) != (K,) or \
            (scores is not None and tuple(scores.shape) != (K,)):
        raise _capi.HpsError("mask_predict: frames (K, %d, %d, %d), weights (4, %d, 64, %d), bias (%d,), logit weight (NC, %d) and bias "
                             "(NC,), labels (K,)" % (F, F, C, C // 2, C // 32, C, C))
    probs = torch.empty(K, S, S, device=frames.device, dtype=torch.float32)
    logits = torch.empty(K, S, S, device=frames.device, dtype=torch.float32) if with_logits else None
    a = _capi.DetMaskPredictArgs(struct_bytes=ctypes.sizeof(_capi.DetMaskPredictArgs), K=K, NC=NC, x=_capi.ptr(frames), wd=_capi.ptr(weights),
                                 bd=_capi.ptr(bias), wl=_capi.ptr(logit_weight), bl=_capi.ptr(logit_bias), labels=_capi.ptr(labels, torch.int64),
                                 scores=_capi.ptr(scores), probs=_capi.ptr(probs), logits=_capi.ptr(logits))
    _capi.call("hps_det_mask_predict", ctypes.byref(a), _capi.stream())
    return probs, logits


def paste_masks(mask_probs, boxes, image_size, threshold=None):
    """hps_det_paste_masks (torchvision's paste_masks_in_image, padding 1) for ONE image: mask_probs (n, 28, 28) or (n, 1, 28, 28), boxes
    (n, 4) in the image's pixels, image_size (H, W) -> (n, 1, H, W): float32 probabilities (torchvision does not threshold), or with
    ``threshold`` in (0, 1) uint8 ``probability > threshold``.  One launch that writes every pixel; no synchronisation."""
    threshold = _check_threshold(threshold)
    _capi.require_device(mask_probs, "mask_probs")
    _capi.require_device(boxes, "boxes")
    S = _capi.DET_MASK_SIZE
    n = mask_probs.shape[0]
    if tuple(mask_probs.shape) not in ((n, S, S), (n, 1, S, S)) or tuple(boxes.shape) != (n, 4):
        raise _capi.HpsError("paste_masks: mask_probs (n, %d, %d) and boxes (n, 4), got %s and %s" % (S, S, tuple(mask_probs.shape), tuple(boxes.shape)))
    H, W = int(image_size[0]), int(image_size[1])
    probs, boxes = _capi.f32c(mask_probs), _capi.f32c(boxes)
    out = torch.empty(n, 1, H, W, device=probs.device, dtype=torch.float32 if threshold is None else torch.uint8)
    a = _capi.DetPasteMasksArgs(struct_bytes=ctypes.sizeof(_capi.DetPasteMasksArgs), n=n, H=H, W=W, binary=0 if threshold is None else 1,
                                threshold=0.0 if threshold is None else threshold, probs=_capi.ptr(probs), boxes=_capi.ptr(boxes),
                                out=_capi._P(out.data_ptr()))
    _capi.call("hps_det_paste_masks", ctypes.byref(a), _capi.stream())
    return out


class MaskRCNNBoxDetector(DeviceStateModule):
    """See the module docstring.  Keywords carry torchvision's names and defaults."""

    def __init__(self, num_classes=91, min_size=800, max_size=1333, image_mean=(0.485, 0.456, 0.406), image_std=(0.229, 0.224, 0.225),
                 rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, box_score_thresh=0.05,
                 box_nms_thresh=0.5, box_detections_per_img=100, frozen_bn_eps=0.0):
        super().__init__()
        if num_classes < 2:
            raise ValueError("num_classes counts the background: at least 2")
        for name, v in (("rpn_pre_nms_top_n_test", rpn_pre_nms_top_n_test), ("rpn_post_nms_top_n_test", rpn_post_nms_top_n_test)):
            if not 1 <= v <= _capi.DET_NMS_MAX_BOXES:
                raise ValueError("%s = %r: the device NMS takes 1 to %d boxes per category" % (name, v, _capi.DET_NMS_MAX_BOXES))
        if box_detections_per_img < 1:
            raise ValueError("box_detections_per_img must be at least 1")
        self.num_classes, self.min_size, self.max_size = int(num_classes), int(min_size), int(max_size)
        self.image_mean, self.image_std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
        self.rpn_pre_nms_top_n, self.rpn_post_nms_top_n = int(rpn_pre_nms_top_n_test), int(rpn_post_nms_top_n_test)
        self.rpn_nms_thresh, self.box_score_thresh, self.box_nms_thresh = float(rpn_nms_thresh), float(box_score_thresh), float(box_nms_thresh)
        self.box_detections_per_img, self.frozen_bn_eps = int(box_detections_per_img), float(frozen_bn_eps)
        conv = lambda cin, cout, k: nn.Conv2d(cin, cout, kernel_size=k, padding=k // 2)
        body = ResNet([3, 4, 6, 3], 3, block=Bottleneck)
        _freeze_batchnorm(body, self.frozen_bn_eps)
        self.backbone = nn.Module()
        self.backbone.body = body
        self.backbone.fpn = nn.Module()
        self.backbone.fpn.inner_blocks = nn.ModuleList([conv(c, 256, 1) for c in (256, 512, 1024, 2048)])
        self.backbone.fpn.layer_blocks = nn.ModuleList([conv(256, 256, 3) for _ in range(4)])
        self.rpn = nn.Module()
        self.rpn.head = nn.Module()
        self.rpn.head.conv, self.rpn.head.cls_logits, self.rpn.head.bbox_pred = conv(256, 256, 3), conv(256, 3, 1), conv(256, 12, 1)
        self.roi_heads = nn.Module()
        self.roi_heads.box_head = nn.Module()
        self.roi_heads.box_head.fc6, self.roi_heads.box_head.fc7 = nn.Linear(256 * 7 * 7, 1024), nn.Linear(1024, 1024)
        self.roi_heads.box_predictor = nn.Module()
        self.roi_heads.box_predictor.cls_score = nn.Linear(1024, self.num_classes)
        self.roi_heads.box_predictor.bbox_pred = nn.Linear(1024, 4 * self.num_classes)
        # the mask branch: run by mask_branch (detect_padded / forward with masks=True)
        self.roi_heads.mask_head = nn.Module()
        for i in range(1, 5):
            setattr(self.roi_heads.mask_head, "mask_fcn%d" % i, conv(256, 256, 3))
        self.roi_heads.mask_predictor = nn.Module()
        self.roi_heads.mask_predictor.conv5_mask = nn.ConvTranspose2d(256, 256, 2, 2)
        self.roi_heads.mask_predictor.mask_fcn_logits = conv(256, self.num_classes, 1)
        self._register_load_state_dict_pre_hook(self._rename_later_spelling)
        super().train(False)

    @staticmethod
    def _rename_later_spelling(state_dict, prefix, *_):
        """``inner_blocks.N.0.*`` / ``layer_blocks.N.0.*`` / ``rpn.head.conv.0.0.*`` of later torchvision releases -> this tree's names."""
        for key in list(state_dict):
            if not key.startswith(prefix):
                continue
            parts = key[len(prefix):].split(".")
            new = None
            if parts[:2] == ["backbone", "fpn"] and len(parts) == 6 and parts[2] in ("inner_blocks", "layer_blocks") and parts[4] == "0":
                new = parts[:4] + parts[5:]
            elif parts[:3] == ["rpn", "head", "conv"] and len(parts) == 6 and parts[3:5] == ["0", "0"]:
                new = parts[:3] + parts[5:]
            if new is not None:
                state_dict[prefix + ".".join(new)] = state_dict.pop(key)

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("the device detector runs in eval mode only: no training, no backward")
        return super().train(False)

    # ---- weight preparation ----
    def prepare(self):
        fpn, head, rh = self.backbone.fpn, self.rpn.head, self.roi_heads
        L = lambda m: _Layer16(m.weight, m.bias)
        fc = lambda m: _Layer16(m.weight.detach()[:, :, None, None], m.bias)
        with torch.no_grad():
            # fc6 reads (c, ph, pw); hps_det_roi_align writes (ph, pw, c)
            w6 = rh.box_head.fc6.weight.detach().reshape(1024, 256, 7, 7).permute(0, 2, 3, 1).reshape(1024, 256 * 49)
            W = lambda m: _wide_layer(m.weight, m.bias, m.padding[0])
            prep = {"inner": [W(m) for m in fpn.inner_blocks], "layer": [W(m) for m in fpn.layer_blocks], "rpn_conv": W(head.conv), "rpn_cls": L(head.cls_logits), "rpn_box": L(head.bbox_pred),
                    "fc6": _wide_layer(w6[:, :, None, None], rh.box_head.fc6.bias, 0),
                    "fc7": _wide_layer(rh.box_head.fc7.weight.detach()[:, :, None, None], rh.box_head.fc7.bias, 0),
                    "cls": fc(rh.box_predictor.cls_score), "box": fc(rh.box_predictor.bbox_pred),
                    "anchors": [base_anchors(s) for s in _LEVEL_SIZES],
                    "mask": [W(getattr(rh.mask_head, "mask_fcn%d" % i)) for i in range(1, 5)],
                    "mask_wd": mask_weights(rh.mask_predictor.conv5_mask.weight),
                    "mask_bd": rh.mask_predictor.conv5_mask.bias.detach().float().contiguous().clone(),
                    "mask_wl": rh.mask_predictor.mask_fcn_logits.weight.detach().float().reshape(self.num_classes, -1).contiguous().clone(),
                    "mask_bl": rh.mask_predictor.mask_fcn_logits.bias.detach().float().contiguous().clone()}
        self._prepared = prep
        return prep

    # ---- stage 1 + 2: transform, backbone, FPN ----
    def _images(self, images):
        if isinstance(images, torch.Tensor):
            if images.dim() != 4:
                raise _capi.HpsError("detector input: a (B, 3, H, W) tensor or a list of (3, H, W) tensors")
            images = list(images.unbind(0))
        images = list(images)
        if not 1 <= len(images) <= _capi.DET_MAX_IMAGES:
            raise _capi.HpsError("detector input: 1 to %d images per call" % _capi.DET_MAX_IMAGES)
        if self.training:
            raise RuntimeError("the device detector runs in eval mode only")
        out = []
        for im in images:
            if not isinstance(im, torch.Tensor) or im.dim() != 3 or im.shape[0] != 3 or im.shape[1] < 1 or im.shape[2] < 1:
                raise _capi.HpsError("detector input: every image must be a (3, H, W) tensor")
            if im.requires_grad:
                raise RuntimeError("the detector has no backward pass on the device: an input requires grad; detach it")
            _capi.require_device(im, "detector input")
            out.append(_capi.f32c(im.detach()))
        return out

    def _fpn_plan(self, prep, B, FH, FW, taps, device):
        key = (B, FH, FW, _capi.stream().value, tuple(t.data_ptr() for t in taps))
        return self._derived("fpn", key, lambda: self._new_fpn_plan(prep, B, taps, device), limit=4)

    def _new_fpn_plan(self, prep, B, taps, device):
        z = lambda *shape: torch.zeros(*shape, device=device, dtype=torch.float32)
        hw = [(t.shape[1] - 2, t.shape[2] - 2) for t in taps]
        inner = [z(B, h, w, 256) for h, w in hw[:3]]                       # lateral maps of C2..C4 (pad 0)
        t = [z(B, h + 2, w + 2, 256) for h, w in hw]                       # top-down sums (t[3]: the lateral map of C5 itself)
        P = [z(B, h + 2, w + 2, 256) for h, w in hw]
        hp, wp = (hw[3][0] + 1) // 2, (hw[3][1] + 1) // 2
        pool = z(B, hp + 2, wp + 2, 256)
        inner_ops, ws0 = _wide_ops([(prep["inner"][k], taps[k], 1, inner[k] if k < 3 else t[3], 0 if k < 3 else 1, False) for k in range(4)], device)
        ops = []
        for k in (2, 1, 0):
            a = _capi.HrnetFuseArgs(n_terms=2, y=_capi.ptr(t[k]), opad=1, B=B, H=hw[k][0], W=hw[k][1], C=256, relu=0)
            a.term[0], a.shift[0], a.pad[0] = inner[k].data_ptr(), 0, 0
            a.term[1], a.shift[1], a.pad[1] = t[k + 1].data_ptr(), 1, 1
            ops.append(_capi.HrnetOp(kind=_capi.HRNET_FUSE, fuse=a))
        layer_ops, ws1 = _wide_ops([(prep["layer"][k], t[k], 1, P[k], 1, False) for k in range(4)], device)
        # RPN head on P2..P5 and pool
        maps = [(P[k], hw[k][0], hw[k][1]) for k in range(4)] + [(pool, hp, wp)]
        rt = [z(B, h, w, 256) for _, h, w in maps]
        logits = [z(B, h, w, 3) for _, h, w in maps]
        deltas = [z(B, h, w, 12) for _, h, w in maps]
        rpn_wide, ws2 = _wide_ops([(prep["rpn_conv"], m, 1, rt[l], 0, True) for l, (m, _, _) in enumerate(maps)], device)
        rpn = _conv_ops([p for l, (_, h, w) in enumerate(maps) for p in (prep["rpn_cls"].problem(rt[l], B, h, w, 0, logits[l], 0, False),
                                                                          prep["rpn_box"].problem(rt[l], B, h, w, 0, deltas[l], 0, False))])
        ks = [min(self.rpn_pre_nms_top_n, h * w * 3) for _, h, w in maps]
        N = max(ks)
        return {"fpn_ops": (_capi.HrnetOp * len(ops))(*ops), "inner_ops": inner_ops, "layer_ops": layer_ops, "rpn_wide": rpn_wide,
                "scratch": (ws0, ws1, ws2),
                "rpn_ops": (_capi.HrnetOp * len(rpn))(*rpn), "P": P, "pool": pool, "hw": hw,
                "pool_hw": (hp, wp), "maps": maps, "logits": logits, "deltas": deltas, "ks": ks, "N": N,
                "cand_boxes": z(B, 5 * N, 4), "cand_scores": torch.full((B, 5 * N), _NEG_INF, device=device, dtype=torch.float32),
                "keep": (inner, t, rt)}

    @torch.no_grad()
    def features(self, images, frame=None):
        """Stages 1 and 2.  ``frame`` = (FH, FW), multiples of 32: a frame at least this large, as when the images are part of a batch
        with a larger image (the frame's zero region is part of the convolutions' input, so an image's result belongs to its frame).  Returns a dict: ``input`` (the stem's input frame, (B, FH + 6, FW + 6, 4) NHWC with a 3-pixel zero halo),
        ``C`` / ``P`` (C2..C5, P2..P5: zero-haloed NHWC frames (B, h + 2, w + 2, c)), ``pool``, ``sizes`` ([(resized h, w)]),
        ``orig`` ([(H, W)]), ``frame`` ((FH, FW)).  The frames belong to the module: the next call of the same shape overwrites them."""
        ims = self._images(images)
        prep = self._prepared or self.prepare()
        B, dev = len(ims), ims[0].device
        orig = [(int(im.shape[1]), int(im.shape[2])) for im in ims]
        sizes = [resized_size(H, W, self.min_size, self.max_size) for H, W in orig]
        FH, FW = (max(s[0] for s in sizes) + 31) // 32 * 32, (max(s[1] for s in sizes) + 31) // 32 * 32
        if frame is not None:
            if frame[0] % 32 or frame[1] % 32:
                raise _capi.HpsError("detector: frame sizes are multiples of 32, got %s" % (tuple(frame),))
            FH, FW = max(FH, int(frame[0])), max(FW, int(frame[1]))
        held = {}

        def fill(frame):
            if tuple(frame.shape) != (B, FH + 6, FW + 6, 4):
                raise _capi.HpsError("detector: the stem's input frame is %s" % (tuple(frame.shape),))
            a = _capi.DetTransformArgs(struct_bytes=ctypes.sizeof(_capi.DetTransformArgs), B=B, FH=FH, FW=FW, P=3, y=_capi.ptr(frame))
            for c in range(3):
                a.mean[c], a.std[c] = self.image_mean[c], self.image_std[c]
            for b, im in enumerate(ims):
                d = a.image[b]
                d.src, d.H, d.W, d.oh, d.ow = _capi.ptr(im), orig[b][0], orig[b][1], sizes[b][0], sizes[b][1]
            _capi.call("hps_det_transform", ctypes.byref(a), _capi.stream())
            held["input"] = frame

        taps = self.backbone.body.stage_taps((B, 3, FH, FW), dev, fill=fill)
        plan = self._fpn_plan(prep, B, FH, FW, taps, dev)
        _capi.run_enc_ops(plan["inner_ops"], 0, len(plan["inner_ops"]))
        _run(plan["fpn_ops"])
        _capi.run_enc_ops(plan["layer_ops"], 0, len(plan["layer_ops"]))
        h5, w5 = plan["hw"][3]
        _capi.call("hps_det_subsample2", _capi.ptr(plan["P"][3]), _capi.ptr(plan["pool"]), B, h5, w5, 256, 1, 1, _capi.stream())
        return {"input": held["input"], "C": taps, "P": plan["P"], "pool": plan["pool"], "sizes": sizes, "orig": orig, "frame": (FH, FW),
                "plan": plan}

    # ---- stage 3: RPN ----
    @torch.no_grad()
    def proposals(self, feats):
        """Stage 3 on ``features``' output.  Returns ``boxes`` (B, R, 4) in resized-image pixels and ``scores`` (B, R) (objectness
        logits, descending, -inf with a zero box for absent rows), and the intermediate tensors: ``logits`` / ``deltas`` per level (NHWC,
        the module's), ``top`` per level ((values, indices) of the top-k), ``cand_boxes`` (B, 5, N, 4) / ``cand_scores`` (B, 5, N) after
        decode, clip and the small-box filter, ``keep_scores`` (B, 5, N) after the per-level NMS."""
        prep = self._prepared or self.prepare()
        plan, sizes = feats["plan"], feats["sizes"]
        B, (FH, FW) = len(sizes), feats["frame"]
        _capi.run_enc_ops(plan["rpn_wide"], 0, len(plan["rpn_wide"]))
        _run(plan["rpn_ops"])
        N, top = plan["N"], []
        for l, (_, h, w) in enumerate(plan["maps"]):
            k = plan["ks"][l]
            vals, idx = torch.topk(plan["logits"][l].view(B, h * w * 3), k, dim=1)
            vals, idx = vals.contiguous(), idx.contiguous()
            top.append((vals, idx))
            a = _capi.DetRpnDecodeArgs(struct_bytes=ctypes.sizeof(_capi.DetRpnDecodeArgs), B=B, h=h, w=w, A=3, k=k, n_out=5 * N, out_offset=l * N,
                                       stride_h=float(FH // h), stride_w=float(FW // w), min_size=1e-3, deltas=_capi.ptr(plan["deltas"][l]),
                                       index=_capi.ptr(idx, torch.int64), logits=_capi.ptr(vals), boxes=_capi.ptr(plan["cand_boxes"]),
                                       scores=_capi.ptr(plan["cand_scores"]))
            base = prep["anchors"][l]
            for i in range(3):
                for e in range(4):
                    a.base[i][e] = float(base[i, e])
            _set_sizes(a.size, sizes)
            _capi.call("hps_det_rpn_decode", ctypes.byref(a), _capi.stream())
        cb, cs = plan["cand_boxes"], plan["cand_scores"]
        keep = nms_groups(cb.view(B * 5, N, 4), cs.view(B * 5, N), self.rpn_nms_thresh)
        R = min(self.rpn_post_nms_top_n, 5 * N)
        pvals, pidx = torch.topk(keep.view(B, 5 * N), R, dim=1)
        present = pvals > _NEG_INF
        boxes = cb.gather(1, pidx[:, :, None].expand(B, R, 4)) * present[:, :, None]
        return {"boxes": boxes.contiguous(), "scores": pvals.contiguous(), "logits": plan["logits"], "deltas": plan["deltas"], "top": top,
                "cand_boxes": cb.view(B, 5, N, 4), "cand_scores": cs.view(B, 5, N), "keep_scores": keep.view(B, 5, N)}

    # ---- stage 4 + the box head's layers ----
    def _head_plan(self, prep, B, R, device):
        def build():
            z = lambda c: torch.zeros(B, R, c, device=device, dtype=torch.float32)
            NC = self.num_classes
            x6, x7, xo, logits, deltas = z(256 * 49), z(1024), z(1024), z(NC), z(4 * NC)
            M = B * R
            fc_ops, ws = _wide_ops([(prep["fc6"], x6.view(1, 1, M, -1), 0, x7.view(1, 1, M, -1), 0, True),
                                    (prep["fc7"], x7.view(1, 1, M, -1), 0, xo.view(1, 1, M, -1), 0, True)], device)
            ops = _conv_ops([prep["cls"].problem(xo, 1, 1, M, 0, logits, 0, False), prep["box"].problem(xo, 1, 1, M, 0, deltas, 0, False)])
            return {"ops": (_capi.HrnetOp * len(ops))(*ops), "fc_ops": fc_ops, "scratch": ws, "x6": x6, "logits": logits, "deltas": deltas, "keep": (x7, xo)}
        return self._derived("head", (B, R, _capi.stream().value), build, limit=4)

    @torch.no_grad()
    def box_head(self, feats, props):
        """Stage 4 and the box head's layers: ``roi`` (B, R, 49 * 256) in (bin, channel) order, ``logits`` (B, R, num_classes),
        ``deltas`` (B, R, 4 num_classes); the module's buffers."""
        prep = self._prepared or self.prepare()
        boxes, scores = props["boxes"], props["scores"]
        B, R, _ = boxes.shape
        plan = self._head_plan(prep, B, R, boxes.device)
        a = _capi.DetRoiAlignArgs(struct_bytes=ctypes.sizeof(_capi.DetRoiAlignArgs), B=B, R=R, C=256, bins=7, n_levels=4,
                                  boxes=_capi.ptr(boxes), scores=_capi.ptr(scores), y=_capi.ptr(plan["x6"]))
        for l, frame in enumerate(feats["P"]):
            lv = a.level[l]
            lv.x, lv.h, lv.w, lv.pad, lv.scale = _capi.ptr(frame), frame.shape[1] - 2, frame.shape[2] - 2, 1, 1.0 / (4 << l)
        _capi.call("hps_det_roi_align", ctypes.byref(a), _capi.stream())
        _capi.run_enc_ops(plan["fc_ops"], 0, len(plan["fc_ops"]))
        _run(plan["ops"])
        return {"roi": plan["x6"], "logits": plan["logits"], "deltas": plan["deltas"]}

    # ---- stage 5 ----
    @torch.no_grad()
    def detections(self, feats, props, head, with_probs=False, with_rois=False):
        """Stage 5: ``boxes`` (B, D, 4) in the input images' pixels, ``labels`` (B, D) int64, ``scores`` (B, D) descending (absent rows
        zero), ``counts`` (B,) int32 on the device; and the intermediate ``cand_boxes`` (B, NC - 1, R, 4) / ``cand_scores`` (B, NC - 1, R)
        after soft-max, decode, clip and the filters (resized-image pixels, proposal order), ``order`` (each class's descending order),
        ``keep_scores`` (B, NC - 1, R) after the per-class NMS in that order, ``probs`` (B, R, NC) with ``with_probs``.  With
        ``with_rois`` (the mask branch's input): ``roi_boxes`` (B, D, 4), the rows of ``cand_boxes`` that hps_det_gather selects, before
        its rescale (resized-image pixels; absent rows zero), and ``roi_scores`` (B, D), the presence mark of the library: the score
        where the row is present, -infinity where it is absent (``scores`` has 0 there).  No synchronisation."""
        sizes, orig = feats["sizes"], feats["orig"]
        B, R, _ = props["boxes"].shape
        NC, dev = self.num_classes, props["boxes"].device
        f = dict(device=dev, dtype=torch.float32)
        cb, cs = torch.empty(B, NC - 1, R, 4, **f), torch.empty(B, NC - 1, R, **f)
        probs = torch.empty(B, R, NC, **f) if with_probs else None
        a = _capi.DetBoxDecodeArgs(struct_bytes=ctypes.sizeof(_capi.DetBoxDecodeArgs), B=B, R=R, NC=NC, score_thresh=self.box_score_thresh,
                                   min_size=1e-2, logits=_capi.ptr(head["logits"]), deltas=_capi.ptr(head["deltas"]),
                                   proposals=_capi.ptr(props["boxes"]), prop_scores=_capi.ptr(props["scores"]), boxes=_capi.ptr(cb),
                                   scores=_capi.ptr(cs), probs=_capi.ptr(probs))
        _set_sizes(a.size, sizes)
        _capi.call("hps_det_box_decode", ctypes.byref(a), _capi.stream())
        ss, order = torch.sort(cs, dim=2, descending=True)
        ss, order = ss.contiguous(), order.contiguous()
        keep = nms_groups(cb.view(B * (NC - 1), R, 4), ss.view(B * (NC - 1), R), self.box_nms_thresh, order.view(B * (NC - 1), R))
        D = min(self.box_detections_per_img, (NC - 1) * R)
        tvals, tidx = torch.topk(keep.view(B, (NC - 1) * R), D, dim=1)
        tvals, tidx = tvals.contiguous(), tidx.contiguous()
        ob, ol, osc = torch.empty(B, D, 4, **f), torch.empty(B, D, device=dev, dtype=torch.int64), torch.empty(B, D, **f)
        counts = torch.empty(B, device=dev, dtype=torch.int32)
        g = _capi.DetGatherArgs(struct_bytes=ctypes.sizeof(_capi.DetGatherArgs), B=B, D=D, R=R, NC=NC, top_scores=_capi.ptr(tvals),
                                top_index=_capi.ptr(tidx, torch.int64), order=_capi.ptr(order, torch.int64), boxes=_capi.ptr(cb),
                                out_boxes=_capi.ptr(ob), out_labels=_capi.ptr(ol, torch.int64), out_scores=_capi.ptr(osc),
                                counts=_capi.ptr(counts, torch.int32))
        _set_sizes(g.size, [s + o for s, o in zip(sizes, orig)])
        _capi.call("hps_det_gather", ctypes.byref(g), _capi.stream())
        out = {"boxes": ob, "labels": ol, "scores": osc, "counts": counts, "cand_boxes": cb, "cand_scores": cs, "order": order,
               "keep_scores": keep.view(B, NC - 1, R), "probs": probs}
        if with_rois:
            # hps_det_gather's own selection: position (c - 1, p) of the top-k is proposal order[b, c - 1, p] of class c
            r = order.view(B, (NC - 1) * R).gather(1, tidx)
            flat = tidx - tidx % R + r
            present = tvals > _NEG_INF
            out["roi_boxes"] = (cb.view(B, (NC - 1) * R, 4).gather(1, flat[:, :, None].expand(B, D, 4)) * present[:, :, None]).contiguous()
            out["roi_scores"] = tvals
        return out

    # ---- the mask branch ----
    def _mask_plan(self, prep, K, device):
        def build():
            F, C = _capi.DET_MASK_BINS + 2, _capi.DET_MASK_CHANNELS
            roi, f1, f2 = (torch.zeros(K, F, F, C, device=device, dtype=torch.float32) for _ in range(3))
            m = prep["mask"]
            ops, ws = _wide_ops([(m[0], roi, 1, f1, 1, True), (m[1], f1, 1, f2, 1, True), (m[2], f2, 1, f1, 1, True), (m[3], f1, 1, f2, 1, True)], device)
            return {"ops": ops, "scratch": ws, "roi": roi, "features": f2, "keep": f1}
        return self._derived("mask", (K, _capi.stream().value), build, limit=4)

    @torch.no_grad()
    def mask_branch(self, feats, dets, with_logits=True):
        """The mask branch on ``features``' and ``detections(..., with_rois=True)``'s output: ``roi`` (B D, 16, 16, 256), the 14 x 14
        RoIAlign of the detections' boxes (resized-image pixels) over P2..P5 inside a zero halo; ``features`` (B D, 16, 16, 256) after
        the four 3x3 + ReLU layers (the wide kernel, K in slices of 256 products); ``probs`` / ``logits`` (B, D, 28, 28) from
        hps_det_mask_predict: the sigmoid of the detection's own class's logit, and the logit (None without ``with_logits``).  Absent
        rows are zero.  ``roi`` and ``features`` are the module's buffers.  No synchronisation."""
        prep = self._prepared or self.prepare()
        if "roi_boxes" not in dets:
            raise _capi.HpsError("mask_branch: the detections carry no roi_boxes; call detections(..., with_rois=True)")
        boxes, scores, labels = dets["roi_boxes"], dets["roi_scores"], dets["labels"]
        B, D, _ = boxes.shape
        plan = self._mask_plan(prep, B * D, boxes.device)
        a = _capi.DetRoiAlignArgs(struct_bytes=ctypes.sizeof(_capi.DetRoiAlignArgs), B=B, R=D, C=_capi.DET_MASK_CHANNELS, bins=_capi.DET_MASK_BINS,
                                  n_levels=4, boxes=_capi.ptr(boxes), scores=_capi.ptr(scores), y=_capi.ptr(plan["roi"]))
        for l, frame in enumerate(feats["P"]):
            lv = a.level[l]
            lv.x, lv.h, lv.w, lv.pad, lv.scale = _capi.ptr(frame), frame.shape[1] - 2, frame.shape[2] - 2, 1, 1.0 / (4 << l)
        _capi.call("hps_det_roi_align_halo", ctypes.byref(a), 1, _capi.stream())
        _capi.run_enc_ops(plan["ops"], 0, len(plan["ops"]))
        probs, logits = mask_predict(plan["features"], prep["mask_wd"], prep["mask_bd"], prep["mask_wl"], prep["mask_bl"], labels.view(B * D),
                                     scores.view(B * D), with_logits=with_logits)
        S = _capi.DET_MASK_SIZE
        return {"roi": plan["roi"], "features": plan["features"], "probs": probs.view(B, D, S, S),
                "logits": logits.view(B, D, S, S) if with_logits else None}

    # ---- the composition ----
    def detect_padded(self, images, frame=None, masks=False):
        """(boxes (B, D, 4), labels (B, D) int64, scores (B, D), counts (B,) int32), D = box_detections_per_img; rows past an image's
        count are zero.  With ``masks`` a fifth tensor, mask_probs (B, D, 28, 28): each detection's mask inside its box, before the
        paste.  Everything stays on the device: no host synchronisation."""
        feats = self.features(images, frame)
        props = self.proposals(feats)
        det = self.detections(feats, props, self.box_head(feats, props), with_rois=bool(masks))
        if not masks:
            return det["boxes"], det["labels"], det["scores"], det["counts"]
        return det["boxes"], det["labels"], det["scores"], det["counts"], self.mask_branch(feats, det, with_logits=False)["probs"]

    def forward(self, images, frame=None, masks=False, mask_threshold=None):
        """[{"boxes": (n, 4), "labels": (n,) int64, "scores": (n,)}] per image, by descending score.  The last step reads the counts on
        the host to size the returned tensors: the call's one synchronisation.  With ``masks`` each dict gains ``"masks"`` (n, 1, H, W):
        float32 probabilities in the input image's pixels as torchvision returns them, or uint8 ``probability > mask_threshold`` with a
        ``mask_threshold`` in (0, 1); the paste (hps_det_paste_masks, one launch per image, only the n masks allocated) follows the
        synchronisation."""
        mask_threshold = _check_threshold(mask_threshold)
        if not masks:
            boxes, labels, scores, counts = self.detect_padded(images, frame)
            return [{"boxes": boxes[b, :n], "labels": labels[b, :n], "scores": scores[b, :n]} for b, n in enumerate(counts.tolist())]
        boxes, labels, scores, counts, probs = self.detect_padded(images, frame, masks=True)
        sizes = [tuple(im.shape[-2:]) for im in images]
        return [{"boxes": boxes[b, :n], "labels": labels[b, :n], "scores": scores[b, :n],
                 "masks": paste_masks(probs[b, :n], boxes[b, :n], sizes[b], mask_threshold)} for b, n in enumerate(counts.tolist())]


def maskrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=91, pretrained_backbone=False, **kwargs):
    """torchvision.models.detection.maskrcnn_resnet50_fpn's box path (run_predict.py:43); weights come from ``load_state_dict``."""
    if pretrained or pretrained_backbone:
        raise NotImplementedError("no network access: pretrained weights are not available")
    return MaskRCNNBoxDetector(num_classes=num_classes, **kwargs)
