"""Cases and a NumPy restatement for the device JPEG encoder (csrc/jpeg_encode.hip, include/hps.h: hps_jpeg_encode).

The restatement builds the WHOLE file from the rules include/hps.h states -- markers, Annex K tables scaled by the quality, 16.16
colour conversion, the padding rules, 2 x 2 / 2 x 1 down-sampling with alternating bias, libjpeg's accurate integer DCT, quantisation,
dummy blocks, the Huffman code with the Annex K tables, byte stuffing -- and is independent of the library.  It is held to
``PIL.Image.save(format="JPEG", quality=q, subsampling=s)`` byte for byte.  ``restated(name)`` is cached: the tests share one result.
"""
import functools
import io

import numpy as np

from jpeg_scenario import NATURAL, picture, turbo            # noqa: F401  (the zig-zag order and the noise-over-gradient pictures)

SAMPLINGS = ("grey", "444", "422", "420")
SAMPLING_CODE = {"grey": 0, "444": 0, "422": 1, "420": 2}
_FACTORS = {"grey": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}       # (hmax, vmax): luminance's factors; chrominance is 1 x 1

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
    0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
    0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
    0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])


def pil_encode(pixels, quality, sampling):
    from PIL import Image
    kw = dict(quality=quality)
    if pixels.ndim == 3:
        kw["subsampling"] = SAMPLING_CODE[sampling]
    buf = io.BytesIO()
    Image.fromarray(pixels).save(buf, "JPEG", **kw)
    return buf.getvalue()


# -----------------------------------------------------------------------------------------------------------------------------------
# the restatement
# -----------------------------------------------------------------------------------------------------------------------------------
def quant_table(base, quality):
    """Natural order, (64,) int64."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def _codes(table):
    """symbol -> (code, length), canonical."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            out[symbols[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def header(H, W, C, quality, sampling):
    be16 = lambda v: bytes([v >> 8, v & 255])
    out = b"\xff\xd8" + b"\xff\xe0" + be16(16) + b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0])
    tables = [quant_table(BASE_LUMA, quality)] + ([quant_table(BASE_CHROMA, quality)] if C == 3 else [])
    for i, t in enumerate(tables):
        out += b"\xff\xdb" + be16(67) + bytes([i]) + bytes(t[NATURAL].astype(np.uint8).tolist())
    hmax, vmax = _FACTORS[sampling]
    out += b"\xff\xc0" + be16(8 + 3 * C) + bytes([8]) + be16(H) + be16(W) + bytes([C])
    for c in range(C):
        out += bytes([c + 1, (hmax << 4 | vmax) if c == 0 else 0x11, 0 if c == 0 else 1])
    for cls_id, t in ((0x00, DC_LUMA), (0x10, AC_LUMA)) + (((0x01, DC_CHROMA), (0x11, AC_CHROMA)) if C == 3 else ()):
        out += b"\xff\xc4" + be16(19 + len(t[1])) + bytes([cls_id]) + bytes(t[0]) + bytes(t[1])
    out += b"\xff\xda" + be16(6 + 2 * C) + bytes([C])
    for c in range(C):
        out += bytes([c + 1, 0x00 if c == 0 else 0x11])
    return out + bytes([0, 63, 0])


def planes(pixels, sampling):
    """The component planes, padded to whole blocks of each component: [(plane int64 (8 bh, 8 bw), bw, bh, h, v)]."""
    H, W = pixels.shape[:2]
    px = pixels.astype(np.int64)
    if pixels.ndim == 2:
        full = [px]
    else:
        R, G, B = px[:, :, 0], px[:, :, 1], px[:, :, 2]
        full = [(19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
                (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
                (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16]
    hmax, vmax = _FACTORS[sampling]
    out = []
    for c, p in enumerate(full):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        cw, ch = -(-W * h // hmax), -(-H * v // vmax)
        bw, bh = -(-cw // 8), -(-ch // 8)
        fx, fy = hmax // h, vmax // v                                             # the down-sampling factors of this component
        p = np.concatenate([p] + [p[:, -1:]] * (8 * bw * fx - W), 1) if 8 * bw * fx > W else p
        rows = -(-H // vmax) * vmax
        p = np.concatenate([p] + [p[-1:]] * (rows - H), 0) if rows > H else p
        if fx == 2 and fy == 2:
            bias = np.tile([1, 2], 4 * bw)[None]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif fx == 2:
            bias = np.tile([0, 1], 4 * bw)[None]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        p = p[:, :8 * bw]
        p = np.concatenate([p] + [p[-1:]] * (8 * bh - p.shape[0]), 0) if 8 * bh > p.shape[0] else p[:8 * bh]
        out.append((p, bw, bh, h, v))
    return out


def _fdct_1d(d, first):
    d0, d1, d2, d3, d4, d5, d6, d7 = d
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    ds = lambda x: (x + (1 << (n - 1))) >> n
    if first:
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o0, o4 = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o2, o6 = ds(z1 + t13 * 6270), ds(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return [o0, ds(t7 + z1 + z4), o2, ds(t6 + z2 + z3), o4, ds(t5 + z2 + z4), o6, ds(t4 + z1 + z3)]


def fdct(blocks):
    """(n, 8, 8) samples -> (n, 8, 8) coefficients scaled by 8 (jfdctint: rows, then columns)."""
    s = blocks - 128
    rows = np.stack(_fdct_1d([s[:, :, i] for i in range(8)], True), 2)
    return np.stack(_fdct_1d([rows[:, i, :] for i in range(8)], False), 1)


def quantise(coefs, q):
    """(n, 8, 8) scaled coefficients, q (64,) natural -> (n, 64) int64, natural order."""
    c = coefs.reshape(-1, 64)
    d = 8 * q[None]
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def scan_blocks(pixels, quality, sampling):
    """The blocks in scan order: (coefficients (n, 64) int64 in ZIG-ZAG order, component of each block, dummy flags 0 / 1 column / 2 row)."""
    comps = planes(pixels, sampling)
    tables = [quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality), quant_table(BASE_CHROMA, quality)]
    grids = []
    for c, (p, bw, bh, h, v) in enumerate(comps):
        b = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
        grids.append(quantise(fdct(b), tables[c])[:, NATURAL].reshape(bh, bw, 64))
    hmax, vmax = _FACTORS[sampling]
    H, W = pixels.shape[:2]
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    coefs, comp_of, dummy = [], [], []
    for r in range(my):
        for m in range(mx):
            for c, (p, bw, bh, h, v) in enumerate(comps):
                for by in range(v):
                    for bx in range(h):
                        y, x = r * v + by, m * h + bx
                        if y < bh and x < bw:
                            coefs.append(grids[c][y, x])
                            dummy.append(0)
                        else:                                                     # a dummy: the DC of the block before it, no AC
                            z = np.zeros(64, np.int64)
                            z[0] = coefs[-1][0]
                            coefs.append(z)
                            dummy.append(2 if y >= bh else 1)
                        comp_of.append(c)
    return np.stack(coefs), comp_of, dummy


def _magnitude(v):
    """(bits, size) of a DC difference or AC value."""
    s = int(abs(v)).bit_length()
    return (v if v >= 0 else v + (1 << s) - 1), s


def restate(pixels, quality, sampling):
    """dict(data: the file; symbols: [("dc", size, diff) | ("ac", run, size, value) | ("zrl",) | ("eob",)]; blocks_without_eob;
    pad_bits; stuffed; dummy: the set of dummy kinds met)."""
    H, W = pixels.shape[:2]
    C = 3 if pixels.ndim == 3 else 1
    coefs, comp_of, dummy = scan_blocks(pixels, quality, sampling)
    dc_codes, ac_codes = [_codes(DC_LUMA), _codes(DC_CHROMA)], [_codes(AC_LUMA), _codes(AC_CHROMA)]
    acc, nbits, symbols, no_eob = 0, 0, [], 0
    pred = [0, 0, 0]

    def put(v, n):
        nonlocal acc, nbits
        acc = (acc << n) | v
        nbits += n

    for row, c in zip(coefs.tolist(), comp_of):
        t = 0 if c == 0 else 1
        diff = row[0] - pred[c]
        pred[c] = row[0]
        bits, s = _magnitude(diff)
        put(*dc_codes[t][s])
        put(bits, s)
        symbols.append(("dc", s, diff))
        run = 0
        for k in range(1, 64):
            if row[k] == 0:
                run += 1
                continue
            while run > 15:
                put(*ac_codes[t][0xF0])
                symbols.append(("zrl",))
                run -= 16
            bits, s = _magnitude(row[k])
            put(*ac_codes[t][(run << 4) | s])
            put(bits, s)
            symbols.append(("ac", run, s, row[k]))
            run = 0
        if run:
            put(*ac_codes[t][0])
            symbols.append(("eob",))
        else:
            no_eob += 1
    pad = -nbits % 8
    put((1 << pad) - 1, pad)
    raw = acc.to_bytes(nbits // 8, "big") if nbits else b""
    scan = raw.replace(b"\xff", b"\xff\x00")
    data = header(H, W, C, quality, sampling) + scan + b"\xff\xd9"
    return dict(data=data, symbols=symbols, blocks_without_eob=no_eob, pad_bits=pad, stuffed=len(scan) - len(raw), dummy=set(dummy) - {0},
                coefs=coefs)


def noise_bound_bytes(blocks, C):
    """What a scan of ``blocks`` blocks can take at most (include/hps.h: hps_jpeg_encode_bound)."""
    return 2 * (-(-blocks * (22 + 63 * 26) // 8)) + 2 + len(header(1, 1, C, 50, "444" if C == 3 else "grey"))


# -----------------------------------------------------------------------------------------------------------------------------------
# the cases
# -----------------------------------------------------------------------------------------------------------------------------------
def extreme():
    """Greyscale 32 x 24: all-0 and all-255 blocks side by side (a DC step of 2040 at quality 100: 11 bits) and half-step blocks
    (|AC| = 924: 10 bits)."""
    img = np.zeros((24, 32), np.uint8)
    img[0:8, 8:16] = 255
    img[0:8, 24:32] = 255
    img[8:16, 0:8] = 255
    img[8:16, 8:12] = 255                 # a vertical half step
    img[8:12, 16:24] = 255                # a horizontal half step
    img[16:24, 0:4] = 255
    img[16:24, 12:16] = 255
    return img


def stuffing():
    """64 x 64 binary noise: at quality 100 the scan holds hundreds of FF bytes."""
    return (np.random.RandomState(7).randint(0, 2, (64, 64)) * 255).astype(np.uint8)


def sparse():
    """A 16 x 16 picture whose blocks hold one high-frequency term each: zero runs beyond 16 (ZRL)."""
    y, x = np.mgrid[0:16, 0:16]
    return np.clip(128 + 100 * np.cos((2 * x + 1) * 7 * np.pi / 16) * np.cos((2 * y + 1) * 7 * np.pi / 16), 0, 255).astype(np.uint8)


def constant(H, W, C, value=77):
    return np.full((H, W, 3) if C == 3 else (H, W), value, np.uint8)


SHAPES = ((1, 1), (8, 8), (9, 7), (16, 16), (24, 24), (40, 8), (17, 33), (33, 17), (250, 130))          # (width, height)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, pixels, quality, sampling), ...)."""
    out = []
    i = 0
    for (w, h) in SHAPES:
        for sampling in SAMPLINGS:
            for quality in (30, 95) if (w, h) != (250, 130) else (95,):
                out.append(("%dx%d_%s_q%d" % (w, h, sampling, quality), picture(w, h, sampling == "grey", 2000 + i), quality, sampling))
                i += 1
    for sampling in SAMPLINGS:
        out.append(("16x16_%s_q100" % sampling, picture(16, 16, sampling == "grey", 3000 + i), 100, sampling))
        out.append(("17x33_%s_q1" % sampling, picture(17, 33, sampling == "grey", 3100 + i), 1, sampling))
        out.append(("9x7_%s_q75" % sampling, picture(9, 7, sampling == "grey", 3200 + i), 75, sampling))
        i += 1
    out.append(("extreme_grey_q100", extreme(), 100, "grey"))
    out.append(("extreme_420_q100", np.stack([extreme(), extreme().T[:24, :24].repeat(2, 1)[:, :32], 255 - extreme()], -1), 100, "420"))
    out.append(("stuffing_grey_q100", stuffing(), 100, "grey"))
    out.append(("stuffing_444_q100", np.stack([stuffing(), stuffing()[::-1], stuffing()[:, ::-1]], -1), 100, "444"))
    out.append(("sparse_grey_q95", sparse(), 95, "grey"))
    out.append(("sparse_grey_q30", sparse(), 30, "grey"))
    out.append(("constant_grey_q95", constant(24, 40, 1), 95, "grey"))
    out.append(("constant_420_q95", constant(24, 40, 3), 95, "420"))
    for w in range(1, 9):                                                         # final paddings of every length
        out.append(("pad_%d_grey_q95" % w, picture(8 + w, 8, True, 4000 + w), 95, "grey"))
    for p in out:
        p[1].setflags(write=False)
    return tuple(out)


def case(name):
    return {c[0]: c for c in cases()}[name]


@functools.lru_cache(maxsize=None)
def restated(name):
    _, pixels, quality, sampling = case(name)
    return restate(pixels, quality, sampling)
