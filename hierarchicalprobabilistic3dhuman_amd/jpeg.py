"""Baseline JPEG files decoded on the device (csrc/jpeg.hip, include/hps.h: hps_jpeg_parse / hps_jpeg_decode) to the bytes PIL gives.

    parse(data)               host: the header of a file in the device profile; JpegUnsupported for a well-formed file outside it
                              (progressive, CMYK, other samplings, ...: decode those with PIL), ValueError for a malformed one
    EncodedJpeg               the file's bytes and its header: what a DataLoader worker returns instead of pixels (picklable, never
                              touches the GPU)
    DeviceJpegDecoder.decode  main process: one page-locked staging copy for the batch, five launches per 64 files, no host
                              synchronisation; ``check()`` reads the status words where the host waits anyway

Opt-in: the datasets take ``decode="device"``, the predict loop ``image_decoder="device"``.  There is no CPU fallback behind ``decode``.

The other direction (csrc/jpeg_encode.hip, include/hps.h: hps_jpeg_encode): finished pictures to the bytes PIL would save.

    encode_bound(H, W, C, s)  host: a capacity no file exceeds
    DeviceJpegEncoder.encode  device tensors in, (out, length) device tensors back; four launches per eight pictures, no host
                              synchronisation (visualise.DeviceJpegWriter goes on to files; the predict loop takes
                              ``picture_format="jpeg"``)
"""
import ctypes

import numpy as np
import torch

from . import _capi
from .data_layer import MAX_IMAGES, BatchStaging, current_device, require_gpu

MODES = {"rgb": _capi.JPEG_RGB, "native": _capi.JPEG_NATIVE, "grey": _capi.JPEG_GREY}
MAX_DIM = _capi.JPEG_MAX_DIM
STATUS_NAMES = ((_capi.JPEG_ST_MARKERS, "restart markers out of place"), (_capi.JPEG_ST_CODE, "an invalid Huffman code or zero run"),
                (_capi.JPEG_ST_OVERRUN, "a symbol past the end of its restart interval"), (_capi.JPEG_ST_SHORT, "the entropy-coded data ends early"))


class JpegUnsupported(Exception):
    """A well-formed JPEG file outside the device profile (include/hps.h); decode it on the host."""


def _last_error():
    msg = _capi.load(dev=_capi._use_dev).hps_last_error()
    return msg.decode() if msg else ""


def parse(data):
    """bytes -> _capi.JpegHeader (a host call; needs libhps.so, not a GPU)."""
    data = bytes(data)
    header = _capi.JpegHeader()
    rc = _capi.load(dev=_capi._use_dev).hps_jpeg_parse(data, len(data), ctypes.byref(header))
    if rc == _capi.JPEG_NOT_FOR_DEVICE:
        raise JpegUnsupported(_last_error())
    if rc != 0:
        raise ValueError(_last_error())
    return header


class EncodedJpeg:
    """A JPEG file in the device profile: ``data`` (bytes), ``header`` (_capi.JpegHeader), ``name`` (for error messages)."""

    __slots__ = ("data", "header", "name")

    def __init__(self, data, header=None, name=None):
        self.data = bytes(data)
        self.header = header if header is not None else parse(self.data)
        self.name = name

    @property
    def width(self):
        return int(self.header.width)

    @property
    def height(self):
        return int(self.header.height)

    @property
    def ncomp(self):
        return int(self.header.ncomp)

    @property
    def shape(self):
        """(H, W, 3): the shape of the decoded RGB image, so that code which only asks an image's size takes either form."""
        return (self.height, self.width, 3)

    def __getstate__(self):
        return (self.data, bytes(self.header), self.name)

    def __setstate__(self, state):
        self.data, header, self.name = state
        self.header = _capi.JpegHeader.from_buffer_copy(header)

    def __repr__(self):
        return "EncodedJpeg(%r, %dx%d, %d component%s, %d bytes)" % (self.name, self.width, self.height, self.ncomp,
                                                                   "" if self.ncomp == 1 else "s", len(self.data))


def encode_file(path, mode="rgb"):
    """The file as an EncodedJpeg where the device can decode it to ``mode``, else None (not a JPEG, outside the profile, or
    greyscale asked of a colour file).  A malformed JPEG raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] != b"\xff\xd8":
        return None
    try:
        header = parse(data)
    except JpegUnsupported:
        return None
    if mode == "grey" and header.ncomp != 1:
        return None
    return EncodedJpeg(data, header, str(path))


class DeviceJpegDecoder:
    """Decodes batches of EncodedJpeg on the current device.  The returned tensors are views of the decoder's own buffers, valid until
    the next ``decode``; staging, workspace and output grow to the largest batch seen and are then reused."""

    GUARD = 0          # bytes kept free behind every output and behind the workspace (the tests set it and look)

    def __init__(self):
        require_gpu("DeviceJpegDecoder")
        self.staging = BatchStaging()
        self.work = self.out = self.status = self.rounds = None
        self._names, self._count, self.layout = [], 0, None
        self._snapshots, self._pending = None, []          # page-locked copies of the status words: (event, slot, count, names)

    @staticmethod
    def _grow(buf, nbytes):
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(nbytes + nbytes // 4, dtype=torch.uint8, device=current_device())
        return buf

    def decode(self, encoded, mode="rgb", subseq_bits=0):
        """[EncodedJpeg] -> [device uint8 tensors]: (H, W, 3) under "rgb", (H, W) under "grey" (one-component files only), the file's
        own form under "native".  Only enqueues -- with one exception: the status words of at most ``SLOTS`` = 8 calls wait unchecked;
        with eight waiting, the oldest is checked first, BEFORE anything of this call is enqueued, which waits for that call and raises
        HpsError naming ITS files if one was corrupt.  A caller that calls ``check`` at least every eight calls never meets this."""
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
        encoded = list(encoded)
        if not encoded:
            return []
        if len(self._pending) == self.SLOTS:
            self._check_one(self._pending.pop(0), True)
        if self._snapshots is None or self._snapshots.shape[1] < len(encoded):
            self.check()
            self._snapshots = torch.empty(self.SLOTS, max(len(encoded), 4 * MAX_IMAGES), dtype=torch.int32, pin_memory=True)
        headers = [e.header for e in encoded]
        channels = [3 if mode == "rgb" else int(h.ncomp) for h in headers]
        if mode == "grey" and any(c != 1 for c in channels):
            raise JpegUnsupported("greyscale output asked of a colour file: decode it on the host")
        up = lambda n: -(-n // 16) * 16
        ws_bytes = [_capi.query_workspace(_capi.WS_JPEG, *_capi.jpeg_ws_dims(h)) for h in headers]
        out_bytes = [int(h.width) * int(h.height) * c for h, c in zip(headers, channels)]
        g = int(self.GUARD)
        ws_off = np.concatenate([[0], np.cumsum([up(b + g) for b in ws_bytes])]).astype(np.int64)
        out_off = np.concatenate([[0], np.cumsum([up(b + g) for b in out_bytes])]).astype(np.int64)
        self.work = self._grow(self.work, int(ws_off[-1]))
        self.out = self._grow(self.out, int(out_off[-1]))
        n = len(encoded)
        if self.status is None or self.status.numel() < n:
            self.status = torch.empty(max(n, MAX_IMAGES), dtype=torch.int32, device=current_device())
            self.rounds = torch.empty(max(n, MAX_IMAGES), dtype=torch.int32, device=current_device())
        arrays = []
        for e in encoded:
            arrays.append(np.frombuffer(bytes(e.header), np.uint8))
            arrays.append(np.frombuffer(e.data, np.uint8))
        dev = self.staging.upload(arrays)
        results = []
        for b0 in range(0, n, MAX_IMAGES):
            m = min(MAX_IMAGES, n - b0)
            a = _capi.JpegDecodeArgs(struct_bytes=ctypes.sizeof(_capi.JpegDecodeArgs), num_images=m, mode=MODES[mode], subseq_bits=int(subseq_bits),
                                     status=_capi.ptr(self.status[b0:], torch.int32, "status"), rounds=_capi.ptr(self.rounds[b0:], torch.int32, "rounds"))
            for i in range(m):
                j = b0 + i
                im = a.image[i]
                im.header = ctypes.addressof(headers[j])
                im.header_dev = dev[2 * j].data_ptr()
                im.data = dev[2 * j + 1].data_ptr()
                im.out = self.out.data_ptr() + int(out_off[j])
                im.workspace = self.work.data_ptr() + int(ws_off[j])
            _capi.call("hps_jpeg_decode", ctypes.byref(a), _capi.stream())
        for j, (h, c) in enumerate(zip(headers, channels)):
            view = self.out[int(out_off[j]):int(out_off[j]) + out_bytes[j]]
            results.append(view.view(int(h.height), int(h.width), 3) if c == 3 else view.view(int(h.height), int(h.width)))
        self._names, self._count = [e.name for e in encoded], n
        self._snapshot()
        self.layout = dict(ws_off=ws_off, ws_bytes=ws_bytes, out_off=out_off, out_bytes=out_bytes)
        return results

    def statuses(self):
        """The last call's status words (host; waits for the stream)."""
        return self.status[:self._count].cpu().tolist() if self._count else []

    def sync_rounds(self):
        """The rounds each file's synchronisation loop took in the last call (host; waits for the stream)."""
        return self.rounds[:self._count].cpu().tolist() if self._count else []

    SLOTS = 8

    def _snapshot(self):
        """The last call's status words on their way to a page-locked slot, with an event behind the copy: ``check`` reads them
        without a device-to-host copy of its own, and ``check(wait=False)`` without waiting at all."""
        n = self._count                                     # decode() has made room: a free slot, wide enough
        used = {p[1] for p in self._pending}
        slot = next(k for k in range(self.SLOTS) if k not in used)
        self._snapshots[slot, :n].copy_(self.status[:n], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((ev, slot, n, self._names))

    def _check_one(self, entry, wait):
        ev, slot, n, names = entry
        if not wait and not ev.query():
            return False
        ev.synchronize()
        bad = [(i, s) for i, s in enumerate(self._snapshots[slot, :n].tolist()) if s]
        if bad:
            what = "; ".join("%s (file %d of the call): %s" % (names[i] or "<bytes>", i, ", ".join(t for bit, t in STATUS_NAMES if s & bit))
                             for i, s in bad)
            raise _capi.HpsError("device JPEG decode: corrupt or truncated entropy-coded data in " + what)
        return True

    def check(self, wait=True):
        """Raise HpsError naming the files whose stream was corrupt or truncated, over every call not yet checked.  ``wait=True``
        waits for those calls (use it where the host waits anyway); ``wait=False`` looks only at calls that have finished."""
        pending, self._pending = self._pending, []
        try:
            while pending:
                if not self._check_one(pending[0], wait):
                    break
                pending.pop(0)
        except _capi.HpsError:
            pending.pop(0)
            raise
        finally:
            self._pending = pending + self._pending


SAMPLINGS = {"444": 0, "422": 1, "420": 2}


def encode_bound(H, W, C, sampling=2):
    """include/hps.h: hps_jpeg_encode_bound -- a capacity no JPEG file of an (H, W, C) picture exceeds (a host call).  ``sampling``:
    0 / "444", 1 / "422", 2 / "420"; ignored for C = 1."""
    sampling = SAMPLINGS.get(sampling, sampling)
    n = _capi.load(dev=_capi._use_dev).hps_jpeg_encode_bound(int(H), int(W), int(C), int(sampling))
    if n < 0:
        raise _capi.HpsError("hps_jpeg_encode_bound(%d, %d, %d, %d): %s" % (H, W, C, sampling, _last_error()))
    return int(n)


class DeviceJpegEncoder:
    """Baseline JPEG files made on the current device (include/hps.h: hps_jpeg_encode), for callers who want the bytes there:
    ``encode`` takes (H, W), (H, W, 1) or (H, W, 3) uint8 device tensors and returns one ``(out, length)`` pair per picture -- ``out``
    a uint8 tensor of ``encode_bound`` bytes whose first ``length[0]`` (a device int64) are the file, equal to PIL's
    ``save(format="JPEG", quality=quality, subsampling=...)`` byte for byte.  Only enqueues: four launches per
    _capi.JPEG_ENC_MAX_IMAGES pictures, no host synchronisation.  The pairs are views of the encoder's own buffers, valid until the
    next ``encode``; buffers are kept per picture shape.  (visualise.DeviceJpegWriter is the route from pictures to files.)"""

    def __init__(self, quality=95, subsampling="420"):
        require_gpu("DeviceJpegEncoder")
        if subsampling not in SAMPLINGS:
            raise ValueError("subsampling is '444', '422' or '420', not %r" % (subsampling,))
        if not 1 <= int(quality) <= 100:
            raise ValueError("quality is 1 .. 100, not %r" % (quality,))
        self.quality, self.sampling = int(quality), SAMPLINGS[subsampling]
        self._buffers = {}

    def _buffer(self, key, index):
        bufs = self._buffers.setdefault(key, [])
        while len(bufs) <= index:
            H, W, C = key
            dev = current_device()
            ws = _capi.query_workspace(_capi.WS_JPEG_ENC, H, W, _capi.jpeg_enc_d2(C, self.sampling))
            bufs.append((torch.empty(encode_bound(H, W, C, self.sampling), dtype=torch.uint8, device=dev),
                         torch.zeros(1, dtype=torch.int64, device=dev), torch.empty(max(16, ws), dtype=torch.uint8, device=dev)))
        return bufs[index]

    def encode(self, images):
        images = list(images)
        results, keep, used = [], [], {}
        for b0 in range(0, len(images), _capi.JPEG_ENC_MAX_IMAGES):
            group = images[b0:b0 + _capi.JPEG_ENC_MAX_IMAGES]
            a = _capi.JpegEncodeArgs()
            a.struct_bytes, a.num_images = ctypes.sizeof(_capi.JpegEncodeArgs), len(group)
            for i, image in enumerate(group):
                _capi.require_device(image, "image")
                if image.dtype != torch.uint8 or image.dim() not in (2, 3) or (image.dim() == 3 and image.shape[2] not in (1, 3)):
                    raise _capi.HpsError("a picture is (H, W), (H, W, 1) or (H, W, 3) uint8")
                image = image.contiguous()
                if image.data_ptr() % 16:
                    image = image.clone()
                keep.append(image)
                key = (int(image.shape[0]), int(image.shape[1]), int(image.shape[2]) if image.dim() == 3 else 1)
                used[key] = used.get(key, -1) + 1
                out, length, ws = self._buffer(key, used[key])
                im = a.image[i]
                im.pixels, (im.H, im.W, im.C) = _capi.ptr(image, torch.uint8, "image"), key
                im.quality, im.sampling = self.quality, self.sampling
                im.out, im.capacity = _capi.ptr(out, torch.uint8), out.numel()
                im.length, im.workspace = _capi.ptr(length, torch.int64), _capi.ptr(ws, torch.uint8)
                results.append((out, length))
            _capi.call("hps_jpeg_encode", ctypes.addressof(a), _capi.stream())
        return results
