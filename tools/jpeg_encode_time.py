"""Time per image of writing the three predict pictures as files, on one MI355X: visualise.DeviceJpegWriter (hps_jpeg_encode on the
device, quality 95, 4:2:0, only the file crosses) against visualise.DevicePngWriter(strategy="dynamic") -- the route it would replace
for speed -- and against PIL's own JPEG encoder on PngWriter's four host threads (bytes to the host, ``save(format="JPEG",
quality=95)``: the honest host alternative, defined here only).

    python tools/jpeg_encode_time.py [--out profiles/jpeg_encode_time.txt] [--commit ID]

tools/png_encode_time.py's pictures and protocol: the eight-panel figure (1024 x 2048), the body over a 720 x 960 photograph, the
3 x 6 sample sheet (1536 x 3072) at visualise_wh = 512, composed once; a round is, per writer, the host clock from the finished device
pictures to drained files in a temporary directory.  The three writers alternate round by round in one process: 3 warm-up rounds, then
``--rounds`` timed ones; median and quartiles.  Also recorded: the library's launches per image, the device time of the library call
alone, the bytes copied to the host, each picture's file sizes, and whether every timed JPEG file equalled PIL's.  The output is
appended to ``--out``."""
import argparse
import ctypes
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from hierarchicalprobabilistic3dhuman_amd import _capi, visualise  # noqa: E402
from png_encode_time import pictures  # noqa: E402

QUALITY = 95


class PilJpegWriter(visualise.PngWriter):
    """PngWriter's route -- the raw picture to a page-locked buffer, PIL on four host threads -- saving JPEG instead of PNG."""

    def _encode(self, host, copied, shape, path):
        from PIL import Image
        try:
            copied.synchronize()
            tmp = path + ".part"
            Image.fromarray(host.numpy().reshape(shape)).save(tmp, format="JPEG", quality=QUALITY)
            os.replace(tmp, path)
        finally:
            self._free.setdefault(host.numel(), []).append(host)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode_time.txt"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--commit", default="working tree")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    from PIL import Image
    dev = torch.device("cuda", torch.cuda.current_device())
    pics = pictures(dev)
    tmp = tempfile.mkdtemp(prefix="jpeg_encode_time_")
    writers = {"jpeg": visualise.DeviceJpegWriter(quality=QUALITY, subsampling="420"), "png": visualise.DevicePngWriter(strategy="dynamic"),
               "pil": PilJpegWriter()}
    ext = {"jpeg": "jpg", "png": "png", "pil": "jpg"}
    path = lambda route, name: os.path.join(tmp, "%s_%s.%s" % (route, name, ext[route]))
    want = {}
    for name, t in pics:
        buf = io.BytesIO()
        Image.fromarray(t.cpu().numpy()).save(buf, "JPEG", quality=QUALITY)
        want[name] = buf.getvalue()
    same = [True]

    def pil():
        for name, t in pics:
            writers["pil"].write(t, path("pil", name))
        writers["pil"].drain()

    def on_device(route):
        def fn():
            writers[route].write_many([t for _, t in pics], [path(route, name) for name, _ in pics])
            writers[route].drain()
        return fn

    routes = {"jpeg": on_device("jpeg"), "png": on_device("png"), "pil": pil}
    seen = []
    original = _capi.call
    _capi.call = lambda entry, *a: (seen.append(entry), original(entry, *a))[1]
    try:
        routes["jpeg"]()
    finally:
        _capi.call = original
    for _ in range(3):
        for fn in routes.values():
            fn()
    t = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
            if k == "jpeg":                                        # outside the clock: every timed file is PIL's file
                same[0] = same[0] and all(open(path("jpeg", name), "rb").read() == want[name] for name, _ in pics)
    # the library calls alone: device events around windows of 20 calls on the writers' own buffers, the two encoders window by window
    jw, pw = writers["jpeg"], writers["png"]
    key = lambda x: (int(x.shape[0]), int(x.shape[1]), int(x.shape[2]))
    ja = _capi.JpegEncodeArgs()
    ja.struct_bytes, ja.num_images = ctypes.sizeof(_capi.JpegEncodeArgs), len(pics)
    pa = _capi.PngEncodeArgs()
    pa.struct_bytes, pa.num_images = ctypes.sizeof(_capi.PngEncodeArgs), len(pics)
    for a, w in ((ja, jw), (pa, pw)):
        for im, (_, tensor) in zip(a.image, pics):
            slot = w._slot(key(tensor), tensor.device)
            im.pixels, (im.H, im.W, im.C) = _capi.ptr(tensor, torch.uint8), slot.key
            w._describe(im)
            im.out, im.capacity = _capi.ptr(slot.out, torch.uint8), slot.bound
            im.length, im.workspace = _capi.ptr(slot.length, torch.int64), _capi.ptr(slot.workspace, torch.uint8)
    calls = {"jpeg": ("hps_jpeg_encode", ja), "png": ("hps_png_encode", pa)}
    kernel_ms = {route: [] for route in calls}
    for _ in range(1 + 9):
        for route, (entry, a) in calls.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(20):
                _capi.call(entry, ctypes.addressof(a), _capi.stream())
            stop.record()
            stop.synchronize()
            kernel_ms[route].append(start.elapsed_time(stop) / 20)
    kernel_ms = {route: np.percentile(v[1:], [0, 50, 100]) for route, v in kernel_ms.items()}
    for w in writers.values():
        w.close()
    q = {k: np.percentile(v, [25, 50, 75]) for k, v in t.items()}
    iqr = {k: q[k][2] - q[k][0] for k in q}
    sizes = []
    for name, tensor in pics:
        sizes.append((name, tuple(tensor.shape), tensor.numel()) + tuple(os.path.getsize(path(route, name)) for route in ("jpeg", "png", "pil")))
    pil_same = all(open(path("pil", name), "rb").read() == want[name] for name, _ in pics)
    raw_total, jpg_total, png_total = sum(s[2] for s in sizes), sum(s[3] for s in sizes), sum(s[4] for s in sizes)
    verdict = lambda a, b: ("lower by more than the sum of the interquartile ranges (%.2f + %.2f ms): yes" if q[a][1] < q[b][1] - (iqr[a] + iqr[b])
                            else "higher by more than it (%.2f + %.2f ms): the route does NOT win here" if q[a][1] > q[b][1] + (iqr[a] + iqr[b])
                            else "within the sum of the interquartile ranges (%.2f + %.2f ms): no real difference") % (iqr[a], iqr[b])
    lines = ["Writing the three predict pictures of one image as files on one MI355X (gfx950), visualise_wh = 512: tools/jpeg_encode_time.py,",
             "commit: %s.  Host clock from the finished device pictures to drained files; %d rounds of each writer, alternating," % (args.commit, args.rounds),
             "after 3 warm-up rounds; median (quartiles).", "",
             "  (a) DeviceJpegWriter  (hps_jpeg_encode, quality %d, 4:2:0, one call per image)          %6.2f ms  (%.2f .. %.2f)" % (QUALITY, q["jpeg"][1], q["jpeg"][0], q["jpeg"][2]),
             "  (b) DevicePngWriter   (hps_png_encode, strategy dynamic, one call per image)            %6.2f ms  (%.2f .. %.2f)" % (q["png"][1], q["png"][0], q["png"][2]),
             "  (c) PIL save(JPEG, quality %d) on PngWriter's four host threads (the raw pictures cross) %6.2f ms  (%.2f .. %.2f)" % (QUALITY, q["pil"][1], q["pil"][0], q["pil"][2]), "",
             "  (b) / (a), medians %6.2f   (a) against (b): %s" % (q["png"][1] / q["jpeg"][1], verdict("jpeg", "png")),
             "  (c) / (a), medians %6.2f   (a) against (c): %s" % (q["pil"][1] / q["jpeg"][1], verdict("jpeg", "pil")), "",
             "libhps calls per image, (a): %s = %d launches" % (", ".join("%d x %s" % (seen.count(e), e) for e in sorted(set(seen))), 4 * seen.count("hps_jpeg_encode")),
             "the library call alone, the three pictures in one call (device events around 20 calls, median of 9 windows, fastest .. slowest; the two",
             "encoders window by window): hps_jpeg_encode %.3f ms (%.3f .. %.3f), hps_png_encode dynamic %.3f ms (%.3f .. %.3f), png / jpeg %.2f"
             % (kernel_ms["jpeg"][1], kernel_ms["jpeg"][0], kernel_ms["jpeg"][2], kernel_ms["png"][1], kernel_ms["png"][0], kernel_ms["png"][2],
                kernel_ms["png"][1] / kernel_ms["jpeg"][1]),
             "bytes copied to the host per image: (a) %d and (b) %d (the files) + %d (their lengths); (c) %d (the raw pictures)"
             % (jpg_total, png_total, 8 * len(sizes), raw_total), "",
             "file sizes in bytes (every timed file of (a) equalled PIL's save(quality=%d) byte for byte: %s; (c)'s files are PIL's: %s):"
             % (QUALITY, "yes" if same[0] else "NO", "yes" if pil_same else "NO"),
             "  %-8s %-16s %10s %12s %12s %12s %12s" % ("picture", "shape", "raw", "(a) JPEG", "(b) PNG", "(c) PIL JPEG", "(a) / (b)")]
    for name, shape, raw, a, b, c in sizes:
        lines.append("  %-8s %-16s %10d %12d %12d %12d %12.3f" % (name, "x".join(map(str, shape)), raw, a, b, c, a / b))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:                                   # appended: the file keeps the records of earlier commits
        f.write(("\n" if os.path.getsize(args.out) else "") + text)


if __name__ == "__main__":
    main()
