"""The PNG encoder's yardsticks (csrc/png.hip, include/hps.h: hps_png_encode), none of which goes through PIL:

  read_png            an independent reader: splits the chunks, checks every CRC with zlib.crc32, requires IHDR -> IDAT ... -> IEND,
                      zlib.decompress'es the concatenated IDAT data (which verifies the Adler-32) and undoes all five filter types;
  idat_payloads,
  fixed_block_tokens  the IDAT payloads of a file and the tokens of one fixed-Huffman segment with the bit at which its end-of-block
                      code ends: what the tests aim at the bit-packing edges with;
  reference_encode    the stream include/hps.h documents, restated on the host byte for byte (filter rule, run tokeniser, fixed
                      Huffman coding, stored fallback, one IDAT chunk per segment);
  the seeded picture makers and the case list of tests/test_gpu_png.py.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
SEG_BYTES, MAX_SEG_ROWS, MAX_ROW_BYTES, MAX_H = 16384, 64, 12288, 32768


class PngError(ValueError):
    pass


# ---- the reader --------------------------------------------------------------------------------------------------------------------
def chunks(data):
    """[(type, payload)] of a PNG file; every CRC is checked."""
    data = bytes(data)
    if data[:8] != SIGNATURE:
        raise PngError("not a PNG signature")
    out, pos = [], 8
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("a truncated chunk")
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, payload = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if pos + 12 + n > len(data):
            raise PngError("a chunk runs past the end of the file")
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if zlib.crc32(kind + payload) & 0xFFFFFFFF != crc:
            raise PngError("chunk %r: CRC mismatch" % kind)
        out.append((kind, payload))
        pos += 12 + n
        if kind == b"IEND":
            break
    if pos != len(data):
        raise PngError("bytes after IEND")
    return out


def idat_payloads(data):
    return [p for k, p in chunks(data) if k == b"IDAT"]


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def read_png(data):
    """The pixels of an 8-bit greyscale or RGB, non-interlaced PNG: (H, W) or (H, W, 3) uint8."""
    cs = chunks(data)
    kinds = [k for k, _ in cs]
    if len(kinds) < 3 or kinds[0] != b"IHDR" or kinds[-1] != b"IEND" or kinds.count(b"IHDR") != 1 or kinds.count(b"IEND") != 1:
        raise PngError("chunk order must be IHDR, IDAT ..., IEND")
    idat = [i for i, k in enumerate(kinds) if k == b"IDAT"]
    if not idat or idat != list(range(idat[0], idat[0] + len(idat))):
        raise PngError("IDAT chunks must exist and be consecutive")
    if cs[-1][1] != b"" or len(cs[0][1]) != 13:
        raise PngError("IHDR holds 13 bytes, IEND none")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    if depth != 8 or colour not in (0, 2) or comp != 0 or filt != 0 or interlace != 0 or W < 1 or H < 1:
        raise PngError("only 8-bit greyscale / RGB without interlace")
    C = 3 if colour == 2 else 1
    try:
        raw = zlib.decompress(b"".join(cs[i][1] for i in idat))
    except zlib.error as e:
        raise PngError("IDAT data: %s" % e)
    rb = W * C
    if len(raw) != H * (rb + 1):
        raise PngError("IDAT data holds %d bytes, the picture needs %d" % (len(raw), H * (rb + 1)))
    out = np.zeros((H, rb), dtype=np.uint8)
    prev = np.zeros(rb, dtype=np.int64)
    for y in range(H):
        ft, line = raw[y * (rb + 1)], np.frombuffer(raw, dtype=np.uint8, count=rb, offset=y * (rb + 1) + 1).astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(rb, dtype=np.int64)
            for x in range(rb):
                a = cur[x - C] if x >= C else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + prev[x]) >> 1
                else:
                    pred = _paeth(int(a), int(prev[x]), int(prev[x - C]) if x >= C else 0)
                cur[x] = (line[x] + pred) & 255
        else:
            raise PngError("row %d: unknown filter type %d" % (y, ft))
        out[y] = cur
        prev = cur
    return out.reshape(H, W, 3) if C == 3 else out.reshape(H, W)


# ---- deflate's fixed code, read and written ------------------------------------------------------------------------------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_block_tokens(segment):
    """One segment's deflate bytes -> (tokens, end_bit) when it opens with a fixed-Huffman block: tokens are ("lit", v) and
    ("match", length, distance), end_bit the bit position (from the segment's start) just after the end-of-block code.  A segment that
    opens with a stored block gives (None, None)."""
    pos = [0]

    def bit():
        b = (segment[pos[0] >> 3] >> (pos[0] & 7)) & 1
        pos[0] += 1
        return b

    def lsb(n):
        return sum(bit() << i for i in range(n))

    def msb(n, v=0):
        for _ in range(n):
            v = (v << 1) | bit()
        return v

    bit()
    if lsb(2) != 1:
        return None, None
    tokens = []
    while True:
        c = msb(7)
        if c <= 0x17:
            sym = 256 + c
        else:
            c = msb(1, c)
            if 0x30 <= c <= 0xBF:
                sym = c - 0x30
            elif 0xC0 <= c <= 0xC7:
                sym = 280 + c - 0xC0
            else:
                sym = 144 + msb(1, c) - 0x190
        if sym < 256:
            tokens.append(("lit", sym))
        elif sym == 256:
            return tokens, pos[0]
        else:
            if sym > 285:
                raise PngError("length symbol %d" % sym)
            length = _LEN_BASE[sym - 257] + lsb(_LEN_EXTRA[sym - 257])
            d = msb(5)
            tokens.append(("match", length, _DIST_BASE[d] + lsb(_DIST_EXTRA[d])))


def segment_end_bits(data):
    """end_bit % 8 of every fixed-Huffman segment of a file made by hps_png_encode (its first and last IDAT chunks are the zlib header
    and the trailer; stored segments are left out)."""
    ends = [fixed_block_tokens(p)[1] for p in idat_payloads(data)[1:-1]]
    return [e % 8 for e in ends if e is not None]


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, nb):
        self.acc |= v << self.n
        self.n += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, nb):
        self.put(int(format(code, "0%db" % nb)[::-1], 2), nb)

    def finish(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc = self.n = 0
        return bytes(self.out)


def segment_rows(H, W, C):
    """hps_png_segment_rows, restated."""
    return max(1, min(MAX_SEG_ROWS, SEG_BYTES // (1 + W * C)))


def bound(H, W, C):
    """hps_png_bound, restated."""
    return 77 + H * (1 + W * C) + 17 * -(-H // segment_rows(H, W, C))


def filtered_rows(img):
    """(H, 1 + W C) uint8: every row behind its filter byte; Sub (1) where sum |Sub residual| < sum |Up residual|, residuals read as signed
    bytes, else Up (2)."""
    H = img.shape[0]
    flat = img.reshape(H, -1).astype(np.int64)
    C = 3 if img.ndim == 3 else 1
    left = np.zeros_like(flat)
    left[:, C:] = flat[:, :-C]
    up = np.concatenate([np.zeros((1, flat.shape[1]), dtype=np.int64), flat[:-1]], axis=0)
    sub, upr = (flat - left) & 255, (flat - up) & 255
    mag = lambda r: np.where(r < 128, r, 256 - r).sum(axis=1)
    use_sub = mag(sub) < mag(upr)
    out = np.empty((H, flat.shape[1] + 1), dtype=np.uint8)
    out[:, 0] = np.where(use_sub, 1, 2)
    out[:, 1:] = np.where(use_sub[:, None], sub, upr)
    return out


def segment_tokens(f):
    """The documented tokeniser on one segment's filtered bytes."""
    f = np.asarray(f, dtype=np.uint8)
    flag = np.concatenate([[False], f[1:] == f[:-1]])
    zeros = np.flatnonzero(~flag)                                   # the unflagged positions; position 0 is one
    ends = np.concatenate([zeros[1:], [len(f)]])
    tokens = []
    for p, e in zip(zeros.tolist(), ends.tolist()):
        tokens.append(("lit", int(f[p])))
        L = e - p - 1
        while L > 0:
            piece = min(258, L)
            tokens += [("match", piece, 1)] if piece >= 3 else [("lit", int(f[p]))] * piece
            L -= piece
    return tokens


def _length_symbol(L):
    i = max(k for k in range(29) if _LEN_BASE[k] <= L) if L < 258 else 28
    return 257 + i, _LEN_EXTRA[i], L - _LEN_BASE[i]


def encode_segment(f):
    """One segment's deflate bytes and end_bit (None when it is a stored block)."""
    f = bytes(bytearray(np.asarray(f, dtype=np.uint8)))
    w = _Bits()
    w.put(0, 1)
    w.put(1, 2)
    for t in segment_tokens(np.frombuffer(f, dtype=np.uint8)):
        if t[0] == "lit":
            v = t[1]
            w.huff(0x30 + v, 8) if v < 144 else w.huff(0x190 + v - 144, 9)
        else:
            sym, eb, extra = _length_symbol(t[1])
            w.huff(sym - 256, 7) if sym < 280 else w.huff(0xC0 + sym - 280, 8)
            w.put(extra, eb)
            w.huff(0, 5)
    w.huff(0, 7)
    end_bit = 8 * len(w.out) + w.n
    w.put(0, 3)
    fixed = w.finish() + b"\x00\x00\xff\xff"
    if len(fixed) > len(f) + 5:
        return b"\x00" + struct.pack("<HH", len(f), len(f) ^ 0xFFFF) + f, None
    return fixed, end_bit


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def reference_encode(img, with_end_bits=False):
    """The file hps_png_encode documents for ``img`` ((H, W) or (H, W, 1) or (H, W, 3) uint8), built on the host."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    H, W = img.shape[:2]
    C = 3 if img.ndim == 3 else 1
    rows = filtered_rows(img)
    R = segment_rows(H, W, C)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)), _chunk(b"IDAT", b"\x78\x01")]
    end_bits = []
    for r0 in range(0, H, R):
        seg, end = encode_segment(rows[r0:r0 + R].reshape(-1))
        out.append(_chunk(b"IDAT", seg))
        end_bits.append(end)
    out += [_chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", zlib.adler32(rows.tobytes()) & 0xFFFFFFFF)), _chunk(b"IEND", b"")]
    data = b"".join(out)
    return (data, end_bits) if with_end_bits else data


def segmented_zlib_png(img, rows_per_segment, level=6):
    """A multi-IDAT file built from the host's zlib: a 78 01 chunk, one sync-flushed raw-deflate segment per IDAT chunk (filter None),
    a closing 03 00 + Adler-32 chunk -- the container hps_png_encode uses, with another compressor inside."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    C = 3 if img.ndim == 3 else 1
    rows = np.concatenate([np.zeros((H, 1), dtype=np.uint8), img.reshape(H, -1)], axis=1)
    out = [SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)), _chunk(b"IDAT", b"\x78\x01")]
    for r0 in range(0, H, rows_per_segment):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        out.append(_chunk(b"IDAT", co.compress(rows[r0:r0 + rows_per_segment].tobytes()) + co.flush(zlib.Z_SYNC_FLUSH)))
    out += [_chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", zlib.adler32(rows.tobytes()) & 0xFFFFFFFF)), _chunk(b"IEND", b"")]
    return b"".join(out)


# ---- the pictures ----------------------------------------------------------------------------------------------------------------------
def _shape(H, W, C):
    return (H, W) if C == 1 else (H, W, 3)


def constant(H, W, C, value=93):
    return np.full(_shape(H, W, C), value, dtype=np.uint8)


def two_valued(H, W, C, seed):
    """Two values: every row is one of two constant rows, so both filters leave long zero runs with single bytes between them."""
    rs = np.random.RandomState(seed)
    rows = np.where(rs.rand(H) < 0.5, 40, 200).astype(np.uint8)
    return np.broadcast_to(rows.reshape((H,) + (1,) * (len(_shape(H, W, C)) - 1)), _shape(H, W, C)).copy()


def broken_runs(H, W, C, period):
    """Constant, but every ``period``-th byte of a row differs: the filtered runs are broken every 2 or every 3 bytes."""
    flat = np.full((H, W * C), 17, dtype=np.uint8)
    flat[:, period - 1::period] = 16
    flat[1::2] = 255 - flat[1::2]                                    # odd rows differ from the rows above everywhere
    return flat.reshape(_shape(H, W, C))


def all_bytes(H, C, seed):
    """Every byte value in every row, in a seeded order of its own: no filter flattens it."""
    rs = np.random.RandomState(seed)
    flat = np.stack([rs.permutation(256 * C) % 256 for _ in range(H)]).astype(np.uint8)
    return flat.reshape(_shape(H, 256, C))


def noise(H, W, C, seed):
    return np.random.RandomState(seed).randint(0, 256, _shape(H, W, C)).astype(np.uint8)


def ramp(H, W, C, horizontal):
    """horizontal: the value steps along the row by 3 and from row to row by 90 (Sub leaves 3, Up 90: Sub wins); vertical: it steps
    from row to row by 5 and along the row irregularly, so Up wins."""
    y, x = np.mgrid[0:H, 0:W]
    if horizontal:
        v = 3 * x + 90 * y
    else:
        v = 5 * y + (x * x * 31) % 97
    v = (v % 256).astype(np.uint8)
    return v if C == 1 else np.stack([v, 255 - v, (v.astype(np.int64) * 3 % 256).astype(np.uint8)], axis=-1)


def repeating_rows(H, W, C, seed):
    """One seeded row repeated H times: under Up every row after the first is zeros, so the zero run crosses every segment boundary."""
    row = np.random.RandomState(seed).randint(0, 256, (1,) + _shape(1, W, C)[1:]).astype(np.uint8)
    return np.repeat(row, H, axis=0)


def figure_like(H=64, W=128, seed=3):
    """A flat background and textured ellipses: what the predict pictures look like."""
    rs = np.random.RandomState(seed)
    img = np.full((H, W, 3), 255, dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    for _ in range(5):
        cy, cx, ry, rx = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(4, H / 3), rs.uniform(4, W / 4)
        inside = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
        texture = (rs.randint(60, 200, 3)[None, None, :] + 40 * np.sin(0.7 * x + rs.uniform(0, 3))[:, :, None] + rs.randint(-6, 7, (H, W, 1)))
        img[inside] = np.clip(texture, 0, 255).astype(np.uint8)[inside]
    return img


def end_bit_family():
    """Pictures of one row whose single segment ends on every bit offset: a run of equal bytes (a match, so the fixed block beats the stored
    one) followed by k distinct bytes of 144 and more, each a 9-bit literal under either filter's residuals -- the tests do not trust
    this reasoning: they measure the offsets from the files and assert that all eight occurred."""
    out = []
    for k in range(16):
        row = np.concatenate([np.full(60, 3, dtype=np.uint8), np.array([(150 + 7 * j) if j % 2 == 0 else (5 + 3 * j) for j in range(k)], dtype=np.uint8)])
        out.append(row.reshape(1, -1))
    return out


RUN_WIDTHS = list(range(1, 9)) + list(range(257, 263)) + list(range(515, 521))


def run_length_cases():
    """Run lengths around the match limits: (name, picture)."""
    cases = []
    for W in RUN_WIDTHS:
        cases.append(("const_c1_w%d" % W, constant(3, W, 1)))
        cases.append(("two_c1_w%d" % W, two_valued(3, W, 1, W)))
    for W in sorted(set(max(1, w // 3) for w in RUN_WIDTHS) | {86, 87, 172, 173, 174}):
        cases.append(("const_c3_w%d" % W, constant(3, W, 3)))
        cases.append(("two_c3_w%d" % W, two_valued(3, W, 3, W)))
    for period in (2, 3):
        cases.append(("broken%d_c1" % period, broken_runs(3, 262, 1, period)))
        cases.append(("broken%d_c3" % period, broken_runs(3, 87, 3, period)))
    return cases


def symbol_cases():
    return [("all_bytes_c1", all_bytes(8, 1, 1)), ("all_bytes_c3", all_bytes(4, 3, 2)), ("noise_c1", noise(9, 37, 1, 3)), ("noise_c3", noise(7, 21, 3, 4)),
            ("ramp_h_c1", ramp(9, 301, 1, True)), ("ramp_v_c1", ramp(9, 301, 1, False)), ("ramp_h_c3", ramp(5, 100, 3, True)),
            ("ramp_v_c3", ramp(5, 100, 3, False))]


def boundary_cases(W=5, C=1):
    """H around the segment boundaries of a narrow picture (R rows are few bytes), with a row pattern that repeats across them."""
    R = segment_rows(1, W, C)
    cases = []
    for H in (1, R - 1, R, R + 1, 2 * R + 1):
        cases.append(("repeat_h%d" % H, repeating_rows(H, W, C, H)))
        cases.append(("const_h%d" % H, constant(H, W, C)))
        cases.append(("noise_h%d" % H, noise(H, W, C, H)))
    return R, cases


def mixed_cases():
    return [("widest_rgb", noise(2, 4096, 3, 5) // 64 * 64), ("widest_grey", repeating_rows(2, 12288, 1, 6)), ("figure", figure_like()),
            ("narrow_grey", noise(70, 1, 1, 7)), ("one_pixel", constant(1, 1, 3))]
