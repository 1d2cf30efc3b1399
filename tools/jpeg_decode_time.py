"""Time the device JPEG decoder (jpeg.DeviceJpegDecoder, hps_jpeg_decode) against the host route it replaces: PIL decode in this one
process plus the page-locked staging upload of the decoded pixels (data_layer.BatchStaging).

    python tools/jpeg_decode_time.py [--parent COMMIT] [--out FILE]

Two workloads: the training batch (72 backgrounds of LSUN size, 256 on the short side, quality 75, 4:2:0) and the predict group (16
photographs of 720 x 960, quality 90, 4:2:0).  The pictures are synthetic -- smooth fields, soft edges and a little grain -- so that a
file has a photograph's size (about 0.1 of the raw bytes), not a noise picture's.  The two routes alternate in one process, 3 warm-up
and 20 timed rounds each; wall time is the host clock from the files' bytes to finished device tensors (synchronised), reported as
the median with the quartiles.  Device time comes from events around windows of 10 decode calls.  Every decoded file is compared
with PIL first.
"""
import argparse
import io
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hierarchicalprobabilistic3dhuman_amd import data_layer, jpeg  # noqa: E402

WARMUP, ROUNDS, WINDOW, WINDOWS = 3, 20, 10, 9


def photo_like(h, w, seed):
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 3), np.float32)
    for c in range(3):
        for _ in range(6):
            fx, fy, ph, amp = rs.uniform(0.002, 0.03), rs.uniform(0.002, 0.03), rs.uniform(0, 6.28), rs.uniform(10, 40)
            img[:, :, c] += amp * np.sin(fx * x + fy * y + ph)
    coarse = rs.rand(h // 16 + 2, w // 16 + 2, 3).astype(np.float32)
    img += 60 * np.kron(coarse, np.ones((16, 16, 1), np.float32))[:h, :w]          # soft-edged patches
    img += rs.normal(0, 3.0, (h, w, 3))                                            # grain
    img = 128 + (img - img.mean())
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(pixels, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", quality=quality, subsampling=2)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB"), dtype=np.uint8)


def quartiles(v):
    return tuple(float(np.percentile(v, q)) for q in (50, 25, 75))


def fmt(v):
    m, lo, hi = quartiles(v)
    return "%8.3f ms  (%.3f .. %.3f)" % (m, lo, hi)


def run(title, files, out):
    decoder, staging = jpeg.DeviceJpegDecoder(), data_layer.BatchStaging()

    def host_route():
        staged = staging.upload([pil_decode(d) for d in files])
        torch.cuda.synchronize()
        return staged

    def device_route(subseq_bits=0):
        res = decoder.decode([jpeg.EncodedJpeg(d) for d in files], subseq_bits=subseq_bits)
        torch.cuda.synchronize()
        return res

    got = [t.cpu().numpy() for t in device_route()]
    decoder.check()
    same = all(np.array_equal(g, pil_decode(d)) for g, d in zip(got, files))
    rounds = decoder.sync_rounds()
    wall = {"host": [], "device": [], "pil only": [], "parse only": []}
    for r in range(WARMUP + ROUNDS):
        for name, fn in (("host", host_route), ("device", device_route)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= WARMUP:
                wall[name].append(dt)
        t0 = time.perf_counter()
        for d in files:
            pil_decode(d)
        t1 = time.perf_counter()
        for d in files:
            jpeg.parse(d)
        t2 = time.perf_counter()
        if r >= WARMUP:
            wall["pil only"].append((t1 - t0) * 1e3)
            wall["parse only"].append((t2 - t1) * 1e3)
    encoded = [jpeg.EncodedJpeg(d) for d in files]
    device_ms = {}
    for bits in (128, 256, 512, 1024):
        windows = []
        for _ in range(WINDOWS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(WINDOW):
                decoder.decode(encoded, subseq_bits=bits)
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) / WINDOW)
        device_ms[bits] = windows
        decoder.check()
    raw = sum(g.size for g in got)
    enc = sum(len(d) for d in files) + len(files) * len(bytes(encoded[0].header))
    calls = -(-len(files) // data_layer.MAX_IMAGES)
    h, d = quartiles(wall["host"]), quartiles(wall["device"])
    clear = abs(h[0] - d[0]) > (h[2] - h[1]) + (d[2] - d[1])
    lines = [
        "%s: %d files, %d bytes of JPEG (%.0f per file), %d bytes decoded; every file equals PIL byte for byte: %s" % (
            title, len(files), sum(len(x) for x in files), sum(len(x) for x in files) / len(files), raw, "yes" if same else "NO"),
        "  wall, host route    (PIL decode in one process + staging upload of the pixels)   %s" % fmt(wall["host"]),
        "  wall, device route  (parse + staging upload of the files + hps_jpeg_decode)       %s" % fmt(wall["device"]),
        "    of the host route, PIL decode alone                                             %s" % fmt(wall["pil only"]),
        "    of the device route, hps_jpeg_parse alone                                       %s" % fmt(wall["parse only"]),
        "  host / device, medians   %.2f   (%s by more than the sum of the two interquartile ranges: %s)" % (
            h[0] / d[0], "device lower" if d[0] < h[0] else "DEVICE HIGHER", "yes" if clear else "no"),
        "  sixteen worker processes at perfect scaling would bring PIL decode alone to %.3f ms per batch" % (
            quartiles(wall["pil only"])[0] / 16),
    ]
    for bits, w in device_ms.items():
        lines.append("  device time per call, subseq_bits %4d%s (events around %d calls, median of %d windows, fastest .. slowest)  %.3f ms (%.3f .. %.3f)" % (
            bits, " (the default)" if bits == 512 else "", WINDOW, WINDOWS, float(np.median(w)), min(w), max(w)))
    lines += [
        "  launches per call: %d (5 per hps_jpeg_decode call of up to %d files, %d call%s)" % (5 * calls, data_layer.MAX_IMAGES, calls, "" if calls == 1 else "s"),
        "  bytes across PCIe per batch: host route %d (the pixels), device route %d (the files and their %d-byte headers): 1 / %.1f" % (
            raw, enc, len(bytes(encoded[0].header)), raw / enc),
        "  rounds of the synchronisation loop at the default subseq_bits: at most %d, on average %.2f" % (max(rounds), float(np.mean(rounds))),
        "",
    ]
    for line in lines:
        print(line, flush=True)
        out.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent = args.parent
    if parent is None:
        try:
            parent = subprocess.check_output(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, stderr=subprocess.DEVNULL).decode().strip()
        except (OSError, subprocess.CalledProcessError):
            parent = "unknown"
    out = open(args.out, "w") if args.out else open(os.devnull, "w")
    from PIL import features
    head = ("Decoding baseline JPEG files on one MI355X (gfx950) against PIL %s (libjpeg-turbo: %s) on the host: tools/jpeg_decode_time.py,\n"
            "commit: %s + this change.  Routes alternating in one process, %d warm-up and %d timed rounds; median (quartiles).\n" % (
                __import__("PIL").__version__, features.check_feature("libjpeg_turbo"), parent, WARMUP, ROUNDS))
    print(head, flush=True)
    out.write(head + "\n")
    train = [encode(photo_like(256, 256 + 17 * (i % 9), 500 + i) if i % 3 else photo_like(256 + 17 * (i % 9), 256, 500 + i), 75) for i in range(72)]
    run("training batch (72 backgrounds, 256 on the short side, quality 75, 4:2:0)", train, out)
    predict = [encode(photo_like(720, 960, 900 + i), 90) for i in range(16)]
    run("predict group (16 photographs of 720 x 960, quality 90, 4:2:0)", predict, out)
    out.close()


if __name__ == "__main__":
    main()
