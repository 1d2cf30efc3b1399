"""Device-side batch preparation for the datasets (csrc/data_layer.hip): the pixel work the reference's dataset classes do on the host,
per item, in NumPy and OpenCV -- uint8 -> float32, cv2.resize, the bounding-box crop of cv2.warpAffine, joint heat maps -- done per
BATCH on the device from the decoded uint8 data.

    on_the_fly_smpl_train_dataset.OnTheFlySMPLTrainDataset / ssp3d_eval_dataset.SSP3DEvalDataset / pw3d_eval_dataset.PW3DEvalDataset
        __getitem__(index)    host IO and random draws only: a raw item (runs in a DataLoader worker, never touches the GPU)
        prepare_batch(items)  main process: one pinned staging buffer, one host-to-device copy, a fixed number of launches
                              -> the reference's batch dict as device tensors ('fname', 'gender': lists)

``passthrough_collate`` is the DataLoader collate for such datasets and ``preparer`` finds ``prepare_batch`` on a dataset or on the
dataset inside a ``Subset``; the training and evaluation loops use both.  The functions ``texture_gather`` / ``resize_bilinear_u8`` /
``eval_crop_u8`` / ``keypoints_scale_round`` / ``eval_heatmaps`` are the kernels on their own.

Images are decoded with PIL (OpenCV is not a dependency).  PNG decoding is exact; a JPEG may differ from ``cv2.imread`` in the last bit
of some pixels (different IDCT / upsampling defaults of the two libjpeg builds).  The resize and the warp restate OpenCV's integer
arithmetic from its sources and have not been run against OpenCV itself.

With ``decode="device"`` a dataset leaves baseline JPEG files undecoded in ``__getitem__`` (``encode_or_decode_rgb``: the file's bytes
and parsed header) and ``prepare_batch`` decodes them in one call on the device (jpeg.DeviceJpegDecoder, ``DeviceImages``), to the
bytes PIL gives; every other file is decoded by PIL as before.
"""
import ctypes

import numpy as np
import torch

from . import _capi

MAX_IMAGES = _capi.FRONTEND_MAX_IMAGES
ALWAYS_VISIBLE = (0, 1, 2, 3, 4, 5, 6, 11, 12)        # data/ssp3d_eval_dataset.py:66, data/pw3d_eval_dataset.py:58


def current_device():
    return torch.device("cuda", torch.cuda.current_device())


def require_gpu(what):
    if not torch.cuda.is_available():
        raise _capi.HpsError("%s runs on a HIP (MI355X) device only: the pixel work of a batch is done by libhps kernels. "
                             "There is no CPU fallback for this path." % what)


def passthrough_collate(items):
    """DataLoader collate for a dataset with ``prepare_batch``: the list of raw items as it is."""
    return items


def preparer(dataset):
    """``dataset.prepare_batch``, looking through ``torch.utils.data.Subset`` (sharding.shard_dataset); None for any other dataset."""
    while dataset is not None:
        fn = getattr(dataset, "prepare_batch", None)
        if fn is not None:
            return fn
        dataset = getattr(dataset, "dataset", None)
    return None


def check_decoded(dataset):
    """``dataset.check_decoded()``, looking through ``torch.utils.data.Subset``: raises HpsError naming every JPEG file that a
    decode="device" dataset found corrupt or truncated since the last check.  It waits for the batches prepared so far, so the loops
    call it where the host waits anyway (the epoch's read-back, the end of an evaluation); a dataset without it is left alone."""
    while dataset is not None:
        fn = getattr(dataset, "check_decoded", None)
        if fn is not None:
            return fn()
        dataset = getattr(dataset, "dataset", None)


def decode_rgb(path):
    """(H, W, 3) uint8 tensor, what cv2.cvtColor(cv2.imread(path), cv2.COLOR_BGR2RGB) holds (module docstring: JPEG)."""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.array(im.convert("RGB"), dtype=np.uint8))


def check_decode_arg(decode):
    """The datasets' ``decode`` argument: "host" (PIL, in ``__getitem__``) or "device" (jpeg.DeviceJpegDecoder, in ``prepare_batch``)."""
    if decode not in ("host", "device"):
        raise ValueError("decode is 'host' or 'device', not %r" % (decode,))
    return decode


def encode_or_decode_rgb(path):
    """What ``__getitem__`` returns for an image under decode="device": the file as a jpeg.EncodedJpeg (bytes and parsed header, no
    pixels) when it is a JPEG the device decodes, else ``decode_rgb(path)`` as before (PNG, progressive, CMYK, ...).  Host only."""
    from . import jpeg
    encoded = jpeg.encode_file(path, "rgb")
    return encoded if encoded is not None else decode_rgb(path)


class DeviceImages:
    """The images of a batch under decode="device": the decoded ones are staged with the batch's other host data as before, the
    encoded ones go up as file bytes and are decoded in ONE DeviceJpegDecoder call.  ``host_arrays(images)`` is what to add to the
    batch's staging upload, ``resolve(images, staged)`` the (H,W,3) uint8 device tensor of every image, in order; the decoder's status
    words of earlier batches are looked at on the way, without waiting (``check`` waits)."""

    def __init__(self):
        self.decoder = None

    @staticmethod
    def is_encoded(image):
        from . import jpeg
        return isinstance(image, jpeg.EncodedJpeg)

    def host_arrays(self, images):
        return [as_numpy(im) for im in images if not self.is_encoded(im)]

    def resolve(self, images, staged):
        encoded = [im for im in images if self.is_encoded(im)]
        decoded = []
        if encoded:
            if self.decoder is None:
                from . import jpeg
                self.decoder = jpeg.DeviceJpegDecoder()
            self.decoder.check(wait=False)
            decoded = self.decoder.decode(encoded, mode="rgb")
        staged, decoded = iter(staged), iter(decoded)
        return [next(decoded) if self.is_encoded(im) else next(staged) for im in images]

    def check(self):
        if self.decoder is not None:
            self.decoder.check()


def decode_grey(path):
    """(H, W) uint8 tensor, cv2.imread(path, 0) of a single-channel file (a colour file goes through PIL's luma weights, which round
    differently from OpenCV's)."""
    from PIL import Image
    with Image.open(path) as im:
        return torch.from_numpy(np.array(im if im.mode == "L" else im.convert("L"), dtype=np.uint8))


class BatchStaging:
    """The raw data of a batch in ONE reused page-locked buffer and ONE host-to-device copy.  Two host slots alternate: a slot is
    written again only after the copy out of it has finished (an event recorded two batches ago -- the wait does not block in steady
    state).  The device side is one buffer: the copy into it is ordered on the stream behind the previous batch's kernels.  Both grow
    to the largest batch seen and are then reused; the views returned by ``upload`` are valid until the next ``upload``."""

    ALIGN = 16

    def __init__(self):
        self.host, self.events, self.slot, self.dev = [None, None], [None, None], 1, None

    def upload(self, arrays):
        """arrays: C-contiguous numpy arrays of any dtype -> device views of the same shapes and dtypes (16-byte aligned)."""
        offs, total = [], 0
        for a in arrays:
            offs.append(total)
            total += -(-a.nbytes // self.ALIGN) * self.ALIGN
        total = max(total, self.ALIGN)
        self.slot ^= 1
        if self.events[self.slot] is not None:
            self.events[self.slot].synchronize()
        host = self.host[self.slot]
        if host is None or host.numel() < total:
            host = self.host[self.slot] = torch.empty(total + total // 4, dtype=torch.uint8, pin_memory=True)
        if self.dev is None or self.dev.numel() < total:
            self.dev = torch.empty(total + total // 4, dtype=torch.uint8, device=current_device())
        flat = host.numpy()
        for a, o in zip(arrays, offs):
            flat[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        self.dev[:total].copy_(host[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[self.slot] = ev
        return [self.dev[o:o + a.nbytes].view(torch.from_numpy(np.empty(0, a.dtype)).dtype).reshape(a.shape) for a, o in zip(arrays, offs)]


def as_numpy(t):
    return t.numpy() if torch.is_tensor(t) else np.asarray(t)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels on their own
# ---------------------------------------------------------------------------------------------------------------------------------
def texture_gather(grey, nongrey, choices):
    """hps_texture_gather: device banks (n, Ht, Wt, 3) uint8 (either may be None / empty) and host ``choices`` = [(is_grey, idx)] ->
    (B, Ht, Wt, 3) float32 = bank[idx] / 255.  Batches above 64 are split."""
    bank = grey if grey is not None and grey.shape[0] else nongrey
    if bank is None or bank.dim() != 4 or bank.shape[3] != 3:
        raise _capi.HpsError("texture_gather: a bank must be (n, Ht, Wt, 3) uint8")
    Ht, Wt = int(bank.shape[1]), int(bank.shape[2])
    for t in (grey, nongrey):
        if t is not None and t.shape[0] and tuple(t.shape[1:]) != (Ht, Wt, 3):
            raise _capi.HpsError("texture_gather: the two banks differ in texture size")
    B = len(choices)
    out = torch.empty(B, Ht, Wt, 3, device=current_device(), dtype=torch.float32)
    n_grey = int(grey.shape[0]) if grey is not None else 0
    n_nongrey = int(nongrey.shape[0]) if nongrey is not None else 0
    for b0 in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - b0)
        a = _capi.TextureGatherArgs(struct_bytes=ctypes.sizeof(_capi.TextureGatherArgs), B=n, Ht=Ht, Wt=Wt, n_grey=n_grey, n_nongrey=n_nongrey,
                                    grey=_capi.ptr(grey, torch.uint8, "grey bank") if n_grey else None,
                                    nongrey=_capi.ptr(nongrey, torch.uint8, "non-grey bank") if n_nongrey else None,
                                    out=_capi.ptr(out[b0:b0 + n], what="out"))
        for i in range(n):
            a.is_grey[i], a.idx[i] = (1 if choices[b0 + i][0] else 0), int(choices[b0 + i][1])
        _capi.call("hps_texture_gather", ctypes.byref(a), _capi.stream())
    return out


def _u8(t, dims, what):
    _capi.require_device(t, what)
    if t.dtype != torch.uint8 or t.dim() != dims or (dims == 3 and t.shape[2] != 3):
        raise _capi.HpsError("%s must be %s uint8, got %s %s" % (what, "(H,W,3)" if dims == 3 else "(H,W)", tuple(t.shape), t.dtype))
    return _capi.ptr(t, torch.uint8, what)


def resize_bilinear_u8(sources, out_wh):
    """hps_resize_bilinear_u8: B device images (H,W,3) uint8 of any sizes -> (B, 3, out_h, out_w) float32 = cv2.resize(INTER_LINEAR)'s
    uint8 level / 255; ``out_wh`` = (width, height).  Batches above 64 are split."""
    B, ow, oh = len(sources), int(out_wh[0]), int(out_wh[1])
    out = torch.empty(B, 3, oh, ow, device=current_device(), dtype=torch.float32)
    for b0 in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - b0)
        a = _capi.ResizeBilinearU8Args(struct_bytes=ctypes.sizeof(_capi.ResizeBilinearU8Args), B=n, out_w=ow, out_h=oh,
                                       out=_capi.ptr(out[b0:b0 + n], what="out"))
        for i in range(n):
            s = sources[b0 + i]
            a.image[i].src, a.image[i].H, a.image[i].W = _u8(s, 3, "image"), s.shape[0], s.shape[1]
        _capi.call("hps_resize_bilinear_u8", ctypes.byref(a), _capi.stream())
    return out


def eval_crop_u8(images, boxes, scale_factor, out_wh, segs=None, keypoints=None):
    """hps_eval_crop_u8: B device images (H,W,3) uint8, host ``boxes`` = [(centre_vertical, centre_horizontal, side)], optional device
    silhouettes (H,W) uint8 and device keypoints (B,K,3) float64 -> dict(rgb (B,3,wh,wh) float32, seg (B,wh,wh) float32 or None,
    joints (B,K,2) float64 and positions (B,K,2) int32 or None).  Batches above 64 are split."""
    B, wh, dev = len(images), int(out_wh), current_device()
    rgb = torch.empty(B, 3, wh, wh, device=dev, dtype=torch.float32)
    seg = torch.empty(B, wh, wh, device=dev, dtype=torch.float32) if segs is not None else None
    joints = positions = None
    K = 0
    if keypoints is not None:
        if keypoints.dim() != 3 or keypoints.shape[0] != B or keypoints.shape[2] != 3:
            raise _capi.HpsError("eval_crop_u8: keypoints must be (%d, K, 3) float64" % B)
        K = int(keypoints.shape[1])
        joints = torch.empty(B, K, 2, device=dev, dtype=torch.float64)
        positions = torch.empty(B, K, 2, device=dev, dtype=torch.int32)
    for b0 in range(0, B, MAX_IMAGES):
        n = min(MAX_IMAGES, B - b0)
        a = _capi.EvalCropU8Args(struct_bytes=ctypes.sizeof(_capi.EvalCropU8Args), B=n, out_wh=wh, K=K, scale_factor=float(scale_factor),
                                 rgb=_capi.ptr(rgb[b0:b0 + n], what="rgb"), seg=_capi.ptr(seg[b0:b0 + n], what="seg") if seg is not None else None)
        if keypoints is not None:
            a.keypoints = _capi.ptr(keypoints[b0:b0 + n], torch.float64, "keypoints")
            a.joints = _capi.ptr(joints[b0:b0 + n], torch.float64, "joints")
            a.positions = _capi.ptr(positions[b0:b0 + n], torch.int32, "positions")
        for i in range(n):
            im, s = a.image[i], images[b0 + i]
            im.rgb, im.H, im.W = _u8(s, 3, "image"), s.shape[0], s.shape[1]
            if segs is not None:
                g = segs[b0 + i]
                if tuple(g.shape) != (s.shape[0], s.shape[1]):
                    raise _capi.HpsError("eval_crop_u8: silhouette %d is %s, its image %s" % (b0 + i, tuple(g.shape), tuple(s.shape[:2])))
                im.seg = _u8(g, 2, "silhouette")
            im.centre_v, im.centre_h, im.side = (float(v) for v in boxes[b0 + i])
        _capi.call("hps_eval_crop_u8", ctypes.byref(a), _capi.stream())
    return dict(rgb=rgb, seg=seg, joints=joints, positions=positions)


def keypoints_scale_round(keypoints, scale):
    """hps_keypoints_scale_round: device keypoints (B,K,3) float64 and scale (B,2) float64 -> joints (B,K,2) float64 = columns 0, 1
    times the scale, positions (B,K,2) int32 = joints rounded half to even."""
    B, K = int(keypoints.shape[0]), int(keypoints.shape[1])
    if keypoints.dim() != 3 or keypoints.shape[2] != 3 or tuple(scale.shape) != (B, 2):
        raise _capi.HpsError("keypoints_scale_round: keypoints (B, K, 3) and scale (B, 2), float64")
    joints = torch.empty(B, K, 2, device=keypoints.device, dtype=torch.float64)
    positions = torch.empty(B, K, 2, device=keypoints.device, dtype=torch.int32)
    _capi.call("hps_keypoints_scale_round", _capi.ptr(keypoints, torch.float64, "keypoints"), _capi.ptr(scale, torch.float64, "scale"),
               _capi.ptr(joints, torch.float64), _capi.ptr(positions, torch.int32), B, K, _capi.stream())
    return joints, positions


def eval_heatmaps(positions, wh, std, keypoints=None, threshold=None, always_visible=ALWAYS_VISIBLE):
    """hps_eval_heatmaps: device positions (B,K,2) int32 -> (B,K,wh,wh) float32 Gaussians; with ``threshold`` joint k of an image is
    zeroed unless keypoints[b,k,2] > threshold or k is in ``always_visible``."""
    B, K = int(positions.shape[0]), int(positions.shape[1])
    if threshold is not None and (keypoints is None or tuple(keypoints.shape) != (B, K, 3)):
        raise _capi.HpsError("eval_heatmaps: a threshold needs keypoints (%d, %d, 3) float64" % (B, K))
    out = torch.empty(B, K, int(wh), int(wh), device=positions.device, dtype=torch.float32)
    mask = 0
    for k in always_visible:
        mask |= 1 << int(k)
    a = _capi.EvalHeatmapsArgs(struct_bytes=ctypes.sizeof(_capi.EvalHeatmapsArgs), B=B, K=K, wh=int(wh), use_threshold=0 if threshold is None else 1,
                               std=float(std), always_visible=mask & 0xFFFFFFFF, threshold=0.0 if threshold is None else float(threshold),
                               positions=_capi.ptr(positions, torch.int32, "positions"),
                               keypoints=_capi.ptr(keypoints, torch.float64, "keypoints") if threshold is not None else None,
                               out=_capi.ptr(out))
    _capi.call("hps_eval_heatmaps", ctypes.byref(a), _capi.stream())
    return out
