"""Cases and a NumPy restatement for the device JPEG decoder (csrc/jpeg.hip, include/hps.h: hps_jpeg_decode).

``cases()``: files written by PIL's encoder from seeded noise-over-gradient pictures -- noise makes the stream span many subsequences,
quality 100 long codes and large coefficients, quality 30 streams of EOB and ZRL.

The restatement is independent of the library: its own marker walk, a sequential Huffman decode, libjpeg's islow IDCT, fancy
upsampling and colour conversion as include/hps.h states them.  ``restated(name)`` is cached, so the tests share one result.
"""
import functools
import io

import numpy as np

SIZES = ((1, 1), (7, 5), (8, 8), (16, 16), (17, 33), (37, 29), (50, 9), (64, 48), (131, 67))          # (width, height)
SAMPLINGS = ("grey", "444", "422", "420")
QUALITIES = (30, 75, 100)
RESTARTS = ("none", "blocks3", "rows1")
_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def picture(width, height, grey, seed):
    """Noise over a gradient, (H, W) or (H, W, 3) uint8."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:height, 0:width]
    base = (x * 200.0 / max(width - 1, 1) + y * 55.0 / max(height - 1, 1))
    if grey:
        img = base + rng.normal(0, 40, (height, width))
    else:
        img = np.stack([base, 255 - base, (x + y) % 256], -1) + rng.normal(0, 40, (height, width, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(pixels, quality=75, sampling="420", optimize=False, restart="none", progressive=False):
    from PIL import Image
    im = Image.fromarray(pixels)
    kw = dict(quality=quality, optimize=optimize)
    if pixels.ndim == 3:
        kw["subsampling"] = _SUBSAMPLING[sampling]
    if restart == "blocks3":
        kw["restart_marker_blocks"] = 3
    elif restart == "rows1":
        kw["restart_marker_rows"] = 1
    if progressive:
        kw["progressive"] = True
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def cases():
    """((name, file bytes), ...): every size x sampling x quality x table kind x restart placement, 648 files."""
    out = []
    i = 0
    for (w, h) in SIZES:
        for sampling in SAMPLINGS:
            for quality in QUALITIES:
                for optimize in (False, True):
                    for restart in RESTARTS:
                        name = "%dx%d_%s_q%d_%s_%s" % (w, h, sampling, quality, "opt" if optimize else "std", restart)
                        out.append((name, encode(picture(w, h, sampling == "grey", 1000 + i), quality, sampling, optimize, restart)))
                        i += 1
    return tuple(out)


def case_bytes(name):
    return dict(cases())[name]


def pil_pixels(data, rgb=False):
    from PIL import Image
    with Image.open(io.BytesIO(data)) as im:
        return np.array(im.convert("RGB") if rgb else im, dtype=np.uint8)


def turbo():
    from PIL import features
    return bool(features.check_feature("libjpeg_turbo"))


# -----------------------------------------------------------------------------------------------------------------------------------
# the restatement
# -----------------------------------------------------------------------------------------------------------------------------------
def walk(data):
    """The marker walk of a baseline file written by PIL: dict(width, height, comps [(h, v, quant (64,) natural, dc, ac)], ri,
    scan bytes); a Huffman table is (counts[16], symbols)."""
    assert data[:2] == b"\xff\xd8"
    pos, qt, huff, ri, frame = 2, {}, {}, 0, None
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        L = (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4:pos + 2 + L]
        if m == 0xDB:
            q = 0
            while q < len(seg):
                assert seg[q] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[NATURAL] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[seg[q] & 15] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                n = sum(counts)
                huff[(seg[q] >> 4, seg[q] & 15)] = (counts, list(seg[q + 17:q + 17 + n]))
                q += 17 + n
        elif m == 0xDD:
            ri = (seg[0] << 8) | seg[1]
        elif m in (0xC0, 0xC1):
            assert seg[0] == 8
            frame = dict(height=(seg[1] << 8) | seg[2], width=(seg[3] << 8) | seg[4],
                         comps=[(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(seg[5])])
        elif m == 0xDA:
            ns = seg[0]
            assert frame is not None and ns == len(frame["comps"])
            comps = []
            for c in range(ns):
                cid, h, v, tq = frame["comps"][c]
                assert seg[1 + 2 * c] == cid
                comps.append((h, v, qt[tq], huff[(0, seg[2 + 2 * c] >> 4)], huff[(1, seg[2 + 2 * c] & 15)]))
            if ns == 1:
                comps = [(1, 1) + comps[0][2:]]
            start = pos + 2 + L
            end = start
            while end < len(data):
                if data[end] == 0xFF and end + 1 < len(data) and data[end + 1] != 0 and not (0xD0 <= data[end + 1] <= 0xD7):
                    break
                end += 1
            return dict(width=frame["width"], height=frame["height"], comps=comps, ri=ri, scan=data[start:end])
        pos += 2 + L


def _lookup16(table):
    """(65536,) int32: (length << 8) | symbol for the 16 bits at the head of the stream, canonical codes."""
    counts, symbols = table
    look = np.zeros(65536, np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(counts[l - 1]):
            look[code << (16 - l):(code + 1) << (16 - l)] = (l << 8) | symbols[k]
            code += 1
            k += 1
        code <<= 1
    return look.tolist()


def intervals(scan):
    """The scan's restart intervals with the byte stuffing removed."""
    out, cur, i = [], bytearray(), 0
    while i < len(scan):
        b = scan[i]
        if b == 0xFF and i + 1 < len(scan):
            if scan[i + 1] == 0:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= scan[i + 1] <= 0xD7:
                out.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
        cur.append(b)
        i += 1
    out.append(bytes(cur))
    return out


def coefficients(info):
    """Sequential Huffman decode: (blocks, 64) int32 in scan order, natural coefficient order, DC values absolute."""
    comps = info["comps"]
    hs, vs = comps[0][0], comps[0][1]
    mcus = -(-info["width"] // (8 * hs)) * -(-info["height"] // (8 * vs))
    blocks_of = [0] * (hs * vs) + list(range(1, len(comps)))                  # component of each block of an MCU
    dc = [_lookup16(c[3]) for c in comps]
    ac = [_lookup16(c[4]) for c in comps]
    coefs = np.zeros((mcus * len(blocks_of), 64), np.int32)
    per = info["ri"] if info["ri"] else mcus
    parts = intervals(info["scan"])
    assert len(parts) == -(-mcus // per)
    nat = NATURAL.tolist()
    blk = 0
    for k, part in enumerate(parts):
        raw = np.frombuffer(part + b"\0" * 8, np.uint8).astype(np.int64)
        win = ((raw[:-3] << 24) | (raw[1:-2] << 16) | (raw[2:-1] << 8) | raw[3:]).tolist()      # 32 bits from every byte
        p, nbits = 0, 8 * len(part)
        pred = [0] * len(comps)
        for _ in range(min(per, mcus - k * per)):
            for c in blocks_of:
                row = coefs[blk]
                kk, look = 0, dc[c]
                while kk < 64:
                    e = look[(win[p >> 3] >> (16 - (p & 7))) & 0xFFFF]
                    assert e, "no such code"
                    p += e >> 8
                    sym = e & 255
                    s, r = sym & 15, sym >> 4
                    v = 0
                    if s:
                        v = (win[p >> 3] >> (32 - (p & 7) - s)) & ((1 << s) - 1)
                        if v < (1 << (s - 1)):
                            v -= (1 << s) - 1
                        p += s
                    if kk == 0:
                        pred[c] += v
                        row[0] = pred[c]
                        kk, look = 1, ac[c]
                    elif s == 0:
                        kk = kk + 16 if r == 15 else 64
                    else:
                        kk += r
                        row[nat[kk]] = v
                        kk += 1
                blk += 1
        assert p <= nbits, "the decode ran past its interval"
    return coefs


def coefficient_checksum(coefs):
    """sum of value * weight(index) modulo 2^64, the stand-alone host check's figure."""
    flat = coefs.reshape(-1).astype(np.int64).astype(np.uint64)
    idx = np.arange(flat.size, dtype=np.uint64)
    weight = ((idx * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) | np.uint64(1)
    with np.errstate(over="ignore"):
        return int((flat * weight).sum(dtype=np.uint64))


def _idct_1d(c):
    c0, c1, c2, c3, c4, c5, c6, c7 = c
    z1 = (c2 + c6) * 4433
    t2, t3 = z1 - c6 * 15137, z1 + c2 * 6270
    t0, t1 = (c0 + c4) << 13, (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    z1, z2, z3, z4 = c7 + c1, c5 + c3, c7 + c3, c5 + c1
    z5 = (z3 + z4) * 9633
    a, b, d, e = c7 * 2446, c5 * 16819, c3 * 25172, c1 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = a + z1 + z3, b + z2 + z4, d + z2 + z3, e + z1 + z4
    return [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]


def idct(blocks, quant):
    """(n, 64) coefficients -> (n, 8, 8) samples."""
    c = (blocks.astype(np.int64) * quant[None]).reshape(-1, 8, 8)
    cols = np.stack([(x + (1 << 10)) >> 11 for x in _idct_1d([c[:, r, :] for r in range(8)])], 1)          # (n, row, col)
    rows = np.stack([((x + (1 << 17)) >> 18) + 128 for x in _idct_1d([cols[:, :, i] for i in range(8)])], 2)
    return np.clip(rows, 0, 255)


def _h_fancy(t, lo, hi, shift):
    left = np.concatenate([t[:, :1], t[:, :-1]], 1)
    right = np.concatenate([t[:, 1:], t[:, -1:]], 1)
    out = np.empty((t.shape[0], 2 * t.shape[1]), np.int64)
    out[:, 0::2] = (3 * t + left + lo) >> shift
    out[:, 1::2] = (3 * t + right + hi) >> shift
    return out


def upsample(s, hs, vs):
    """Real samples (ch, cw) -> (vs ch, hs cw), libjpeg's fancy upsampling."""
    s = s.astype(np.int64)
    if hs == 1:
        return s
    if vs == 1:
        return _h_fancy(s, 1, 2, 2)
    up = np.concatenate([s[:1], s[:-1]], 0)
    down = np.concatenate([s[1:], s[-1:]], 0)
    out = np.empty((2 * s.shape[0], 2 * s.shape[1]), np.int64)
    out[0::2] = _h_fancy(3 * s + up, 8, 7, 4)
    out[1::2] = _h_fancy(3 * s + down, 8, 7, 4)
    return out


def pixels(info, coefs, rgb=False):
    """(H, W) for a one-component file (``rgb``: the value repeated), else (H, W, 3) RGB."""
    W, H, comps = info["width"], info["height"], info["comps"]
    hs, vs = comps[0][0], comps[0][1]
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    bpm = hs * vs + len(comps) - 1
    per_mcu = coefs.reshape(my, mx, bpm, 64)
    planes = []
    for c, comp in enumerate(comps):
        if c == 0:
            b = idct(per_mcu[:, :, :hs * vs].reshape(-1, 64), comp[2]).reshape(my, mx, vs, hs, 8, 8)
            planes.append(b.transpose(0, 2, 4, 1, 3, 5).reshape(my * vs * 8, mx * hs * 8))
        else:
            b = idct(per_mcu[:, :, hs * vs + c - 1].reshape(-1, 64), comp[2]).reshape(my, mx, 8, 8)
            planes.append(b.transpose(0, 2, 1, 3).reshape(my * 8, mx * 8))
    Y = planes[0][:H, :W]
    if len(comps) == 1:
        Y = Y.astype(np.uint8)
        return np.repeat(Y[:, :, None], 3, 2) if rgb else Y
    cw, ch = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1][:ch, :cw], hs, vs)[:H, :W] - 128
    cr = upsample(planes[2][:ch, :cw], hs, vs)[:H, :W] - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], -1), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def restated(name):
    """dict(info, coefs, pixels (native), checksum) of a case; computed once."""
    info = walk(case_bytes(name))
    coefs = coefficients(info)
    px = pixels(info, coefs)
    px.setflags(write=False)
    return dict(info=info, coefs=coefs, pixels=px, checksum=coefficient_checksum(coefs))


def as_rgb(px):
    return px if px.ndim == 3 else np.repeat(px[:, :, None], 3, 2)
