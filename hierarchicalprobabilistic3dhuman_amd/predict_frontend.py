"""The predict front end for a BATCH of photographs of different sizes, on the device (csrc/predict_frontend.hip): what
predict/predict_poseMF_shapeGaussian_net.py:61-100 does per image -- person box, crop to the HRNet input, key points, crop to the
proxy-representation size, Canny edges and heat maps -- with one HRNet forward per batch and no host synchronisation of its own.

    front = DevicePredictFrontEnd(pose_shape_cfg, hrnet_model, hrnet_cfg, edge_detect_model)
    out = front([photo_a, photo_b, ...])          # (H,W,3) uint8 arrays / tensors or (3,H,W) float device tensors, any sizes
    out["proxy_rep"]                               # (B,18,D,D): the network's input

Launches per batch: hps_predict_boxes, hps_crop_bilinear, the HRNet forward, hps_hrnet_keypoints, hps_crop_bilinear for the proxy size
(its static box records are formed once and kept), hps_canny_edge_map and hps_proxy_rep.  The person detector is an injected
per-image callable (its synchronisation is its own); ``detection.maskrcnn_resnet50_fpn()`` is the device implementation.  The functions ``predict_boxes`` / ``crop_bilinear`` / ``hrnet_keypoints`` are
the three kernels on their own.
"""
import ctypes

import numpy as np
import torch

from . import _capi

IMAGENET_MEAN = (0.485, 0.456, 0.406)                 # predict/predict_hrnet.py:101-102
IMAGENET_STD = (0.229, 0.224, 0.225)
ALWAYS_VISIBLE = (0, 1, 2, 3, 4, 5, 6, 11, 12)        # predict/predict_poseMF_shapeGaussian_net.py:98
MAX_IMAGES, REC = _capi.FRONTEND_MAX_IMAGES, _capi.FRONTEND_RECORD_FLOATS


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def predict_boxes(sizes, detections, out_wh, threshold, scale_factor, hrnet_aspect_fix=True, out=None):
    """hps_predict_boxes: ``sizes`` = [(H, W)], ``detections`` = None or, per image, None or the detector's dict / (boxes, labels,
    scores) on the device -> records (B, 12) float32 (include/hps.h).  Batches above 64 images are split."""
    B = len(sizes)
    if out is None:
        out = torch.empty(B, REC, device=_device(), dtype=torch.float32)
    if tuple(out.shape) != (B, REC):
        raise _capi.HpsError("predict_boxes: out must be (%d, %d)" % (B, REC))
    keep = []
    for b0 in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - b0)
        a = _capi.PredictBoxesArgs(struct_bytes=ctypes.sizeof(_capi.PredictBoxesArgs), B=n, out_w=int(out_wh[0]), out_h=int(out_wh[1]),
                                   hrnet_aspect_fix=1 if hrnet_aspect_fix else 0, threshold=float(threshold),
                                   scale_factor=float(scale_factor), records=_capi.ptr(out[b0:b0 + n], what="records"))
        for i in range(n):
            im = a.image[i]
            im.H, im.W = int(sizes[b0 + i][0]), int(sizes[b0 + i][1])
            det = detections[b0 + i] if detections is not None else None
            if det is not None:
                boxes, labels, scores = (det["boxes"], det["labels"], det["scores"]) if isinstance(det, dict) else det
                boxes = _capi.f32c(boxes).reshape(-1, 4)
                labels, scores = labels.to(torch.int64).contiguous(), _capi.f32c(scores)
                if labels.shape[0] != boxes.shape[0] or scores.shape[0] != boxes.shape[0]:
                    raise _capi.HpsError("predict_boxes: boxes, labels and scores of image %d differ in length" % (b0 + i))
                keep.append((boxes, labels, scores))
                # an EMPTY detector output still says "a detector ran": a non-null pointer of its own (never read: n = 0)
                im.boxes = _capi.ptr(boxes, what="boxes").value or out.data_ptr()
                im.labels = _capi.ptr(labels, torch.int64, "labels").value or out.data_ptr()
                im.scores = _capi.ptr(scores, what="scores").value or out.data_ptr()
                im.n = boxes.shape[0]
        _capi.call("hps_predict_boxes", ctypes.byref(a), _capi.stream())
    return out


def _source(t):
    """(pointer, H, W, kind) of a device image: (H,W,3) uint8 or (3,H,W) float32, contiguous."""
    _capi.require_device(t, "image")
    if t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3:
        return _capi.ptr(t, torch.uint8, "image"), t.shape[0], t.shape[1], _capi.FRONTEND_SRC_HWC_U8
    if t.dtype == torch.float32 and t.dim() == 3 and t.shape[0] == 3:
        return _capi.ptr(t, torch.float32, "image"), t.shape[1], t.shape[2], _capi.FRONTEND_SRC_CHW_F32
    raise _capi.HpsError("an image must be (H,W,3) uint8 or (3,H,W) float32, got %s %s" % (tuple(t.shape), t.dtype))


def crop_bilinear(sources, records, out_wh, normalise=None, raw=None, normalised=None):
    """hps_crop_bilinear: ``sources`` = B device images ((H,W,3) uint8 or (3,H,W) float32, contiguous) and their records (B, 12) ->
    raw (B, 3, out_h, out_w); with ``normalise`` = (mean, std) also normalised = (raw - mean) / std.  Returns (raw, normalised or None)."""
    B = len(sources)
    ow, oh = int(out_wh[0]), int(out_wh[1])
    dev = _device()
    if raw is None:
        raw = torch.empty(B, 3, oh, ow, device=dev, dtype=torch.float32)
    if normalise is not None and normalised is None:
        normalised = torch.empty(B, 3, oh, ow, device=dev, dtype=torch.float32)
    if tuple(raw.shape) != (B, 3, oh, ow) or (normalised is not None and tuple(normalised.shape) != (B, 3, oh, ow)) or tuple(records.shape) != (B, REC):
        raise _capi.HpsError("crop_bilinear: raw / normalised must be (%d, 3, %d, %d) and records (%d, %d)" % (B, oh, ow, B, REC))
    for b0 in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - b0)
        a = _capi.CropBilinearArgs(struct_bytes=ctypes.sizeof(_capi.CropBilinearArgs), B=n, out_w=ow, out_h=oh,
                                   records=_capi.ptr(records[b0:b0 + n], what="records"), raw=_capi.ptr(raw[b0:b0 + n], what="raw"),
                                   normalised=_capi.ptr(normalised[b0:b0 + n], what="normalised") if normalised is not None else None)
        if normalise is not None:
            for c in range(3):
                a.mean[c], a.std[c] = float(normalise[0][c]), float(normalise[1][c])
        for i in range(n):
            im = a.image[i]
            im.src, im.H, im.W, im.kind = _source(sources[b0 + i])
        _capi.call("hps_crop_bilinear", ctypes.byref(a), _capi.stream())
    return raw, normalised


def hrnet_keypoints(heatmaps, factor, records=None, vis_threshold=0.75, always_visible=ALWAYS_VISIBLE):
    """hps_hrnet_keypoints: heatmaps (B,K,h,w) -> joints2D in HRNet-input pixels (B,K,2), confidences (B,K), joints2D in the pixels of
    the crop described by ``records`` (B,12) (None without), visibility (B,K) float 0/1."""
    _capi.require_device(heatmaps, "heatmaps")
    hm = _capi.f32c(heatmaps)
    B, K, h, w = hm.shape
    f = dict(device=hm.device, dtype=torch.float32)
    joints, confs, visib = torch.empty(B, K, 2, **f), torch.empty(B, K, **f), torch.empty(B, K, **f)
    crop = torch.empty(B, K, 2, **f) if records is not None else None
    if records is not None and tuple(records.shape) != (B, REC):
        raise _capi.HpsError("hrnet_keypoints: records must be (%d, %d)" % (B, REC))
    mask = 0
    for k in always_visible:
        mask |= 1 << int(k)
    a = _capi.HrnetKeypointsArgs(struct_bytes=ctypes.sizeof(_capi.HrnetKeypointsArgs), B=B, K=K, h=h, w=w, factor=float(factor),
                                 vis_threshold=float(vis_threshold), always_visible=mask & 0xFFFFFFFF, heatmaps=_capi.ptr(hm),
                                 records=_capi.ptr(records, what="records") if records is not None else None,
                                 joints_hrnet=_capi.ptr(joints), confs=_capi.ptr(confs),
                                 joints_crop=_capi.ptr(crop) if crop is not None else None, visib=_capi.ptr(visib))
    _capi.call("hps_hrnet_keypoints", ctypes.byref(a), _capi.stream())
    return joints, confs, crop, visib


class DevicePredictFrontEnd:
    """predict/predict_poseMF_shapeGaussian_net.py:61-100 for a list of images; see the module docstring.

    ``hrnet_model``: any callable (B,3,h,w) -> (B,K,h',w') heat maps on the device (pose2D_hrnet.PoseHighResolutionNet is the intended
    one); ``object_detect_model``: None or the reference's per-image detector interface; ``edge_detect_model``: a
    canny_edge_detector.CannyEdgeDetector."""

    def __init__(self, pose_shape_cfg, hrnet_model, hrnet_cfg, edge_detect_model, object_detect_model=None,
                 joints2Dvisib_threshold=0.75, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _capi.HpsError("DevicePredictFrontEnd runs on a HIP device only; there is no CPU path")
        if not hasattr(edge_detect_model, "edge_map_into"):
            raise _capi.HpsError("DevicePredictFrontEnd needs an edge detector with edge_map_into (canny_edge_detector.CannyEdgeDetector)")
        self.cfg, self.hrnet, self.hrnet_cfg = pose_shape_cfg, hrnet_model, hrnet_cfg
        self.edge, self.detector = edge_detect_model, object_detect_model
        self.vis_threshold = float(joints2Dvisib_threshold)
        self.in_wh = (int(hrnet_cfg.MODEL.IMAGE_SIZE[0]), int(hrnet_cfg.MODEL.IMAGE_SIZE[1]))
        self.factor = hrnet_cfg.MODEL.IMAGE_SIZE[0] / hrnet_cfg.MODEL.HEATMAP_SIZE[0]      # predict_hrnet.py:107: ONE factor for both
        self.D = int(pose_shape_cfg.DATA.PROXY_REP_SIZE)
        for m in (hrnet_model, object_detect_model):
            if hasattr(m, "eval"):
                m.eval()
        self._proxy_records = None                    # the static records of the second crop, MAX_IMAGES rows, formed once
        self._staging = {"host": [None, None], "dev": [None, None], "event": [None, None], "k": 0}

    # -- inputs -------------------------------------------------------------------------------------------------------------------
    def _upload(self, host):
        """[(index, (H,W,3) uint8 numpy array)] -> {index: device view}: the images packed into one of two reused page-locked
        buffers and sent up as uint8 by ONE non-blocking copy -- a quarter of a float upload's bytes, no host transpose."""
        st = self._staging
        k = st["k"] % 2
        st["k"] += 1
        total = sum(a.size for _, a in host)
        if st["host"][k] is None or st["host"][k].numel() < total:
            st["host"][k] = torch.empty(total, dtype=torch.uint8).pin_memory()
            st["dev"][k] = torch.empty(total, dtype=torch.uint8, device=self.device)
        if st["event"][k] is not None:
            st["event"][k].synchronize()               # the copy that last used this pair (two calls ago) has finished
        views, off = {}, 0
        flat = st["host"][k].numpy()
        for i, a in host:
            flat[off:off + a.size] = np.ascontiguousarray(a).reshape(-1)
            views[i] = (off, a.shape)
            off += a.size
        st["dev"][k][:total].copy_(st["host"][k][:total], non_blocking=True)
        st["event"][k] = torch.cuda.Event()
        st["event"][k].record()
        return {i: st["dev"][k][o:o + s[0] * s[1] * 3].view(s) for i, (o, s) in views.items()}

    def _sources(self, images):
        srcs, host = [None] * len(images), []
        for i, im in enumerate(images):
            if isinstance(im, np.ndarray):
                if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                    raise _capi.HpsError("a host image must be (H,W,3) uint8, got %s %s" % (im.shape, im.dtype))
                host.append((i, im))
            elif torch.is_tensor(im) and not im.is_cuda:
                if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
                    raise _capi.HpsError("a host image must be (H,W,3) uint8, got %s %s" % (tuple(im.shape), im.dtype))
                host.append((i, im.numpy()))
            elif torch.is_tensor(im):
                srcs[i] = im.contiguous()
            else:
                raise _capi.HpsError("an image must be a numpy array or a tensor, got %s" % type(im).__name__)
        if host:
            for i, view in self._upload(host).items():
                srcs[i] = view
        return srcs

    @staticmethod
    def as_float_image(src):
        """(3,H,W) float in [0,1] of a source (the detector's input, the uncropped picture's photograph)."""
        return src if src.dtype == torch.float32 else src.permute(2, 0, 1).float() / 255.0

    # -- the call -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, images, with_image=False):
        B = len(images)
        if B == 0:
            raise _capi.HpsError("DevicePredictFrontEnd: no images")
        srcs = self._sources(images)
        geo = [_source(s) for s in srcs]
        sizes = [(g[1], g[2]) for g in geo]
        floats = [None] * B
        dets = None
        if self.detector is not None:                                                               # predict_hrnet.py:52
            floats = [self.as_float_image(s) for s in srcs]
            dets = [self.detector(f[None])[0] for f in floats]
        data = self.cfg.DATA
        records = predict_boxes(sizes, dets, self.in_wh, data.BBOX_THRESHOLD, data.BBOX_SCALE_FACTOR, hrnet_aspect_fix=True)
        raw, hrnet_input = crop_bilinear(srcs, records, self.in_wh, normalise=(IMAGENET_MEAN, IMAGENET_STD))      # :90-102
        heatmaps = self.hrnet(hrnet_input)                                                          # :103
        if self._proxy_records is None:                                                             # predict/...:73-89: static
            in_w, in_h = self.in_wh
            self._proxy_records = predict_boxes([(in_h, in_w)] * MAX_IMAGES, None, (self.D, self.D), 0.0, 1.0, hrnet_aspect_fix=False)
        chunks = [(b0, min(MAX_IMAGES, B - b0)) for b0 in range(0, B, MAX_IMAGES)]
        if B <= MAX_IMAGES:
            proxy_records = self._proxy_records[:B]
        else:
            proxy_records = self._proxy_records[:1].expand(B, REC).contiguous()
        joints_hrnet, confs, joints, visib = hrnet_keypoints(heatmaps, self.factor, proxy_records, self.vis_threshold, ALWAYS_VISIBLE)
        cropped = torch.empty(B, 3, self.D, self.D, device=raw.device, dtype=torch.float32)
        for b0, n in chunks:                                                                        # predict/...:80-89
            crop_bilinear([raw[b] for b in range(b0, b0 + n)], proxy_records[b0:b0 + n], (self.D, self.D), raw=cropped[b0:b0 + n])
        from .predict_poseMF_shapeGaussian_net import proxy_representation
        proxy = proxy_representation(cropped, joints, visib, self.edge, self.cfg)                   # :91-100
        out = {"proxy_rep": proxy, "cropped_rgb": cropped, "joints2D": joints, "joints2D_hrnet": joints_hrnet, "joints2Dconfs": confs,
               "visib": visib, "hrnet_input": hrnet_input, "hrnet_crop": raw, "bbox_centre": records[:, 0:2], "bbox_height": records[:, 2],
               "bbox_width": records[:, 3], "bbox_wh": records[:, 11], "records": records}
        if with_image:
            out["image"] = [f if f is not None else self.as_float_image(s) for f, s in zip(floats, srcs)]
        return out
