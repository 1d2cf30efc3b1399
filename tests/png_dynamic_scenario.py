"""The yardsticks of hps_png_encode's strategy 1 (csrc/png.hip, include/hps.h: one dynamic Huffman block per segment, all five filters),
beside tests/png_scenario.py, whose reader, container helpers and case lists are used as they are:

  filtered_rows5            the five-filter rule: the type with the smallest sum of |residual|, ties to the lowest type;
  huffman_depths            an UNLIMITED Huffman code's depths on given counts (what the limiting pictures are held against);
  limited_lengths           the documented length-limited construction, restated;
  reference_encode_dynamic  the documented strategy-1 stream, byte for byte (filters, tokens, code construction, header, fallback);
  dynamic_block_info        a small dynamic-block reader: header fields, both sets of code lengths, the tokens, the end bit;
  rle_yardstick             the same container with the host's zlib per segment under Z_RLE (dynamic Huffman, distance-1 matches);
  the new pictures: five_filters, fibonacci_literals, code_length_limit, photo_like.
"""
import struct
import zlib

import numpy as np

import png_scenario as S

MAX_LL_BITS, MAX_CL_BITS = 15, 7
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


# ---- filters -----------------------------------------------------------------------------------------------------------------------------
def filtered_rows5(img):
    """(H, 1 + W C) uint8: every row behind its filter byte.  A row takes the type among None 0, Sub 1, Up 2, Average 3, Paeth 4 with the
    smallest sum of |residual| (residuals read as signed bytes); ties go to the lowest type."""
    H = img.shape[0]
    flat = img.reshape(H, -1).astype(np.int64)
    C = 3 if img.ndim == 3 else 1
    a = np.zeros_like(flat)
    a[:, C:] = flat[:, :-C]
    b = np.concatenate([np.zeros((1, flat.shape[1]), dtype=np.int64), flat[:-1]], axis=0)
    c = np.zeros_like(flat)
    c[:, C:] = b[:, :-C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([(flat - pred) & 255 for pred in (np.zeros_like(flat), a, b, (a + b) >> 1, paeth)])          # (5, H, W C)
    mag = np.where(res < 128, res, 256 - res).sum(axis=2)                                                       # (5, H)
    ft = np.argmin(mag, axis=0)                                                                                 # the first minimum
    out = np.empty((H, flat.shape[1] + 1), dtype=np.uint8)
    out[:, 0] = ft
    out[:, 1:] = res[ft, np.arange(H)]
    return out


# ---- code construction -------------------------------------------------------------------------------------------------------------------
def huffman_depths(weights):
    """Leaf depths of a Huffman tree on ``weights`` (ascending, at least two), by the two-queue method: leaves in the given order,
    internal nodes in the order of their creation; each step takes the two smallest heads, a leaf before an internal node of equal weight."""
    n = len(weights)
    assert n >= 2 and all(weights[i] <= weights[i + 1] for i in range(n - 1))
    iw, pl, pi = [0] * (n - 1), [0] * n, [0] * (n - 1)
    li = ii = 0
    for k in range(n - 1):
        w2 = 0
        for _ in range(2):
            if li < n and (ii >= k or weights[li] <= iw[ii]):
                w2 += weights[li]
                pl[li] = k
                li += 1
            else:
                w2 += iw[ii]
                pi[ii] = k
                ii += 1
        iw[k] = w2
    di = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        di[k] = di[pi[k]] + 1
    return [di[pl[i]] + 1 for i in range(n)]


def limited_lengths(counts, max_bits):
    """The documented code lengths of an alphabet with the given counts (0 = unused), none above ``max_bits``:
    1. the used symbols in descending order of count, ties in ascending order of symbol index;
    2. the number of leaves at each depth of the two-queue Huffman tree on their counts; depths above max_bits count as max_bits;
    3. while the Kraft sum exceeds 1: one code of max_bits leaves, and one code of the greatest length below max_bits that has any
       becomes two codes one bit longer (the sum falls by 2^-max_bits);
    4. the first symbols in the order of 1 take the shortest lengths.
    A single used symbol takes length 1."""
    used = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (-counts[s], s))
    lens = [0] * len(counts)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    bl = [0] * (max_bits + 1)
    for d in huffman_depths([counts[s] for s in reversed(used)]):
        bl[min(d, max_bits)] += 1
    total = sum(bl[d] << (max_bits - d) for d in range(1, max_bits + 1))
    while total > 1 << max_bits:
        bl[max_bits] -= 1
        for i in range(max_bits - 1, 0, -1):
            if bl[i]:
                bl[i] -= 1
                bl[i + 1] += 2
                break
        total -= 1
    j = 0
    for d in range(1, max_bits + 1):
        for _ in range(bl[d]):
            lens[used[j]] = d
            j += 1
    assert j == len(used)
    return lens


def canonical_codes(lens):
    """deflate's canonical codes of a set of lengths (RFC 1951, 3.2.2)."""
    top = max(lens)
    bl = [0] * (top + 2)
    for v in lens:
        if v:
            bl[v] += 1
    nxt, code = [0] * (top + 2), 0
    for d in range(1, top + 1):
        code = (code + bl[d - 1]) << 1
        nxt[d] = code
    codes = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            codes[s] = nxt[v]
            nxt[v] += 1
    return codes


def kraft(lens):
    """sum 2^-len over the used symbols, as a fraction of 2^15: (numerator, 2^15)."""
    return sum(1 << (15 - v) for v in lens if v), 1 << 15


def code_length_tokens(seq):
    """The code-length sequence (the literal/length lengths up to the last used symbol, then the one distance length) as code-length
    symbols, maximal run of equal values by maximal run.  A run of z zeros is cut into pieces of 138 from its start: a piece of 11..138 is
    symbol 18 (7 extra bits: piece - 11), a piece of 3..10 symbol 17 (3 extra bits: piece - 3), a piece of 1 or 2 that many symbols 0.
    A run of r equal lengths v > 0 is v once, then the r - 1 others cut into pieces of 6 from their start: a piece of 3..6 is symbol 16
    (2 extra bits: piece - 3), a piece of 1 or 2 that many symbols v.  -> [(symbol, extra bits, extra value)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        i += r
        if v:
            out.append((v, 0, 0))
            r -= 1
        while r > 0:
            piece = min(138 if v == 0 else 6, r)
            if piece < 3:
                out += [(v, 0, 0)] * piece
            elif v:
                out.append((16, 2, piece - 3))
            elif piece >= 11:
                out.append((18, 7, piece - 11))
            else:
                out.append((17, 3, piece - 3))
            r -= piece
    return out


def segment_histogram(tokens):
    counts = [0] * 286
    for t in tokens:
        counts[t[1] if t[0] == "lit" else S._length_symbol(t[1])[0]] += 1
    counts[256] += 1
    return counts


def dynamic_block(f):
    """One segment's filtered bytes as ONE dynamic block closed by an empty stored block -> (bytes, end_bit, parts); parts holds the
    counts and lengths for the tests."""
    tokens = S.segment_tokens(np.frombuffer(bytes(bytearray(f)), dtype=np.uint8))
    counts = segment_histogram(tokens)
    ll = limited_lengths(counts, MAX_LL_BITS)
    hlit = max(s for s in range(286) if ll[s]) + 1
    cl_tokens = code_length_tokens(ll[:hlit] + [1])
    cl_counts = [0] * 19
    for sym, _, _ in cl_tokens:
        cl_counts[sym] += 1
    cl = limited_lengths(cl_counts, MAX_CL_BITS)
    hclen = max(4, max(k for k in range(19) if cl[CL_ORDER[k]]) + 1)
    ll_codes, cl_codes = canonical_codes(ll), canonical_codes(cl)
    w = S._Bits()
    w.put(0, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(0, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl[CL_ORDER[k]], 3)
    for sym, eb, extra in cl_tokens:
        w.huff(cl_codes[sym], cl[sym])
        w.put(extra, eb)
    for t in tokens:
        if t[0] == "lit":
            w.huff(ll_codes[t[1]], ll[t[1]])
        else:
            sym, eb, extra = S._length_symbol(t[1])
            w.huff(ll_codes[sym], ll[sym])
            w.put(extra, eb)
            w.put(0, 1)                                             # the one distance code: a single bit 0 is distance 1
    w.huff(ll_codes[256], ll[256])
    end_bit = 8 * len(w.out) + w.n
    w.put(0, 3)
    return w.finish() + b"\x00\x00\xff\xff", end_bit, {"counts": counts, "ll": ll, "cl_counts": cl_counts, "cl": cl}


def encode_segment_dynamic(f):
    """Strategy 1 on one segment: the dynamic block unless the strategy-0 form of the segment (its fixed block, or one stored block where
    that is shorter) is strictly shorter.  -> (bytes, kind, end_bit)"""
    dyn, end, _ = dynamic_block(f)
    other, other_end = S.encode_segment(f)
    if len(dyn) <= len(other):
        return dyn, "dynamic", end
    return other, ("stored" if other_end is None else "fixed"), other_end


def _container(img, rows, segments):
    H, W = img.shape[:2]
    C = 3 if img.ndim == 3 else 1
    out = [S.SIGNATURE, S._chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)), S._chunk(b"IDAT", b"\x78\x01")]
    out += [S._chunk(b"IDAT", seg) for seg in segments]
    out += [S._chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", zlib.adler32(rows.tobytes()) & 0xFFFFFFFF)), S._chunk(b"IEND", b"")]
    return b"".join(out)


def _picture(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    return img


def reference_encode_dynamic(img, with_kinds=False):
    """The file hps_png_encode documents for a picture of strategy 1, built on the host."""
    img = _picture(img)
    rows = filtered_rows5(img)
    R = S.segment_rows(img.shape[0], img.shape[1], 3 if img.ndim == 3 else 1)
    coded = [encode_segment_dynamic(rows[r0:r0 + R].reshape(-1)) for r0 in range(0, img.shape[0], R)]
    data = _container(img, rows, [c[0] for c in coded])
    return (data, [c[1:] for c in coded]) if with_kinds else data


def rle_yardstick(filtered, R, img):
    """The container of hps_png_encode around the host's zlib, one sync-flushed raw-deflate stream per segment of R rows of the given
    filtered rows, with strategy Z_RLE: dynamic Huffman codes, matches of distance 1 only."""
    segments = []
    for r0 in range(0, filtered.shape[0], R):
        co = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        segments.append(co.compress(filtered[r0:r0 + R].tobytes()) + co.flush(zlib.Z_SYNC_FLUSH))
    return _container(_picture(img), filtered, segments)


# ---- the dynamic-block reader ------------------------------------------------------------------------------------------------------------
def _decoder(lens):
    codes = canonical_codes(lens)
    return {(lens[s], codes[s]): s for s in range(len(lens)) if lens[s]}


def dynamic_block_info(segment):
    """One segment's deflate bytes -> None when it does not open with a dynamic block, else a dict: hlit, hdist, hclen, cl (19 code-length
    code lengths), ll (hlit literal/length lengths), dist (hdist distance lengths), cl_symbols (the symbols the lengths were coded with),
    tokens, end_bit (the bit just after the end-of-block code)."""
    pos = [0]

    def bit():
        b = (segment[pos[0] >> 3] >> (pos[0] & 7)) & 1
        pos[0] += 1
        return b

    def lsb(n):
        return sum(bit() << i for i in range(n))

    def symbol(table):
        code = 0
        for n in range(1, 16):
            code = (code << 1) | bit()
            if (n, code) in table:
                return table[(n, code)]
        raise S.PngError("no such code")

    bit()
    if lsb(2) != 2:
        return None
    hlit, hdist, hclen = 257 + lsb(5), 1 + lsb(5), 4 + lsb(4)
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = lsb(3)
    table, lens, cl_symbols = _decoder(cl), [], []
    while len(lens) < hlit + hdist:
        s = symbol(table)
        cl_symbols.append(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + lsb(2))
        else:
            lens += [0] * ((3 + lsb(3)) if s == 17 else (11 + lsb(7)))
    if len(lens) != hlit + hdist:
        raise S.PngError("a repeat runs past the lengths")
    ll, dist = lens[:hlit], lens[hlit:]
    lt, dt, tokens = _decoder(ll), _decoder(dist), []
    while True:
        s = symbol(lt)
        if s < 256:
            tokens.append(("lit", s))
        elif s == 256:
            break
        else:
            length = S._LEN_BASE[s - 257] + lsb(S._LEN_EXTRA[s - 257])
            d = symbol(dt)
            tokens.append(("match", length, S._DIST_BASE[d] + lsb(S._DIST_EXTRA[d])))
    return {"hlit": hlit, "hdist": hdist, "hclen": hclen, "cl": cl, "ll": ll, "dist": dist, "cl_symbols": cl_symbols, "tokens": tokens,
            "end_bit": pos[0]}


def segment_infos(data):
    """dynamic_block_info of every segment of a file made by hps_png_encode (None for fixed and stored segments)."""
    return [dynamic_block_info(p) for p in S.idat_payloads(data)[1:-1]]


# ---- the new pictures ----------------------------------------------------------------------------------------------------------------------
def five_filters(W=96, seed=1):
    """Six grey rows, each built from its own predictor plus a residual of +-1, so that each filter type wins at least one row: small
    values (None), a walk of small steps far from the row above (Sub), the row above plus noise under large steps (Up), the mean of left
    and above plus noise (Average), Paeth's choice plus noise over rows with edges in both directions (Paeth).  The tests measure the
    filter bytes; they do not trust this."""
    rs = np.random.RandomState(seed)
    e = lambda: rs.randint(-1, 2, W)
    rows = [np.where(rs.rand(W) < 0.5, 3, 253)]                                                                 # None
    rows.append((128 + np.cumsum(rs.randint(-2, 3, W))) & 255)                                                    # Sub
    rows.append((rows[1] + 40 * (rs.rand(W) < 0.3)) & 255)                                                        # an edge row for the next
    rows.append((rows[2] + e()) & 255)                                                                            # Up
    avg, noise = np.zeros(W, dtype=np.int64), 7 * e()
    for x in range(W):
        avg[x] = (((avg[x - 1] if x else 0) + rows[3][x]) // 2 + noise[x]) & 255
    rows.append(avg)                                                                                              # Average
    edge = (rows[4] + 60 * (np.arange(W) // 7 % 2)) & 255
    rows.append(edge)
    pae, noise = np.zeros(W, dtype=np.int64), e()
    for x in range(W):
        a, b, c = (int(pae[x - 1]) if x else 0), int(edge[x]), (int(edge[x - 1]) if x else 0)
        pae[x] = (S._paeth(a, b, c) + (25 if x % 11 == 0 else 0) + noise[x]) & 255
    rows.append(pae)                                                                                              # Paeth
    return np.stack(rows).astype(np.uint8)


def _interleaved_row(counts):
    """One grey row holding value v counts[v] times (no count above half the total): the bytes sorted by descending count of their value,
    the first half of them on the even places and the second half on the odd ones.  No byte equals its neighbour, so every byte is a
    literal; where the frequent values are the smallest, the large steps between neighbours make filter None the row's choice."""
    order = sorted(range(len(counts)), key=lambda v: (-counts[v], v))
    values = np.concatenate([np.full(counts[v], v, dtype=np.uint8) for v in order])
    row = np.empty(len(values), dtype=np.uint8)
    half = (len(values) + 1) // 2
    row[0::2], row[1::2] = values[:half], values[half:]
    return row.reshape(1, -1)


def fibonacci_literals(n=17):
    """n literal values with the counts 1, 2, 3, 5, 8, ... (6 764 bytes for n = 17; the end-of-block symbol supplies the second 1 of
    Fibonacci's sequence).  Every count exceeds the sum of all counts two and more places below it, so an unlimited Huffman code is a
    chain n bits deep whatever the tie rule."""
    fib = [1, 2]
    while len(fib) < n:
        fib.append(fib[-1] + fib[-2])
    return _interleaved_row(fib[::-1])


def code_length_limit():
    """One segment whose literal/length counts are dyadic -- 2, 3, 5, 8, 13, 21 and 81 values with the counts 256, 64, 16, 8, 4, 2 and 1,
    and the end-of-block symbol's 1: 1 024 in all -- so that the code has exactly 2, 3, 5, 8, 13, 21 and 82 symbols of the lengths 2, 4, 6,
    7, 8, 9 and 10.  The values 2 .. 132 take their counts in an order that leaves no four equal lengths in a row, so no repeat symbol
    is used, and with the one distance length and the one zero run the code-length alphabet's counts are 1, 1, 2, 3, 5, 8, 13, 21, 82: an
    unlimited Huffman code on them is a chain 8 bits deep, one more than the code-length code may have."""
    left = {4: 3, 6: 5, 7: 8, 8: 13, 9: 21, 10: 81}
    lengths = [2, 2]
    while any(left.values()):
        allowed = [L for L in left if left[L] and lengths[-3:] != [L] * 3]
        L = max(allowed, key=lambda L: (left[L], -L))
        lengths.append(L)
        left[L] -= 1
    counts = [1 << (10 - L) for L in lengths]
    counts[0] -= 1                                                   # the row's filter byte, 0, is the last 0
    return _interleaved_row(counts)


def photo_like(H=96, W=160, seed=4, factor=8):
    """Low-frequency seeded noise, (H / factor, W / factor, 3), enlarged bilinearly (pixel centres aligned, edges clamped)."""
    rs = np.random.RandomState(seed)
    small = rs.rand(H // factor, W // factor, 3) * 255.0

    def axis(n, m):
        t = np.clip((np.arange(n) + 0.5) / factor - 0.5, 0, m - 1)
        i0 = np.minimum(np.floor(t).astype(np.int64), m - 2)
        return i0, t - i0

    y0, fy = axis(H, small.shape[0])
    x0, fx = axis(W, small.shape[1])
    top = small[y0] * (1 - fy)[:, None, None] + small[y0 + 1] * fy[:, None, None]
    out = top[:, x0] * (1 - fx)[None, :, None] + top[:, x0 + 1] * fx[None, :, None]
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def new_pictures():
    return [("five_filters", five_filters()), ("fibonacci_literals", fibonacci_literals()), ("code_length_limit", code_length_limit()),
            ("photo_like", photo_like())]


def all_cases():
    """Every picture the strategy-1 tests run: the case lists of png_scenario and the new pictures, (name, picture)."""
    family = [("end_bits_%d" % i, img) for i, img in enumerate(S.end_bit_family())]
    return S.run_length_cases() + S.symbol_cases() + S.boundary_cases()[1] + S.mixed_cases() + family + new_pictures()
