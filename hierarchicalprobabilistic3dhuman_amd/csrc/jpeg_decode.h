// Baseline JPEG: the marker parser (host) and the entropy decoder's bit reader, symbol decode and block step (host and device).
// One source for csrc/jpeg.hip's kernels, hps_jpeg_parse and the stand-alone host check (tests/jpeg_host_check.cpp), which runs
// exactly these functions on the CPU under the sanitizers.  No allocation, no global state; every table index is masked or bounded
// here, so a garbage table or stream can give wrong symbols but never an address outside the tables and the stream.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "hps.h"

#if defined(__HIPCC__)
#define JPG_HD __host__ __device__ inline
#else
#define JPG_HD inline
#endif

#define JPG_LOOK_BITS 10

// zigzag position -> natural (row-major) position
#define JPG_NATURAL_ORDER                                                                                                          \
    {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// One Huffman table in decode form (libjpeg's maxcode / valoffset scheme behind a 10-bit lookahead).
struct JpgTable {
    uint16_t look[1 << JPG_LOOK_BITS];     // (length << 8) | symbol for a code of up to 10 bits at the top of the index, 0: longer
    int32_t maxcode[17];                   // [l]: the largest code of length l, -1: none
    int32_t valoff[17];                    // [l]: index into vals of the first code of length l, minus that code
    uint8_t vals[256];
};

// the per-length part (one thread on the device)
JPG_HD void jpg_table_lengths(const hps_jpeg_huff* h, JpgTable* t) {
    int32_t code = 0, k = 0;
    t->maxcode[0] = -1;
    t->valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        const int32_t n = h->bits[l - 1];
        t->valoff[l] = k - code;
        t->maxcode[l] = n ? code + n - 1 : -1;
        k += n;
        code = (code + n) << 1;
    }
}

// lookahead entry idx (any thread on the device; needs jpg_table_lengths and vals)
JPG_HD uint16_t jpg_look_entry(const JpgTable* t, int idx) {
    for (int l = 1; l <= JPG_LOOK_BITS; ++l) {
        const int32_t code = idx >> (JPG_LOOK_BITS - l);
        if (code <= t->maxcode[l]) return (uint16_t)((l << 8) | t->vals[(t->valoff[l] + code) & 255]);
    }
    return 0;
}

// The destuffed entropy-coded bytes as big-endian bit stream behind 32-bit words.
struct JpgStream {
    const uint32_t* words;
    uint32_t nwords;
};

JPG_HD uint32_t jpg_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }

JPG_HD uint32_t jpg_word(const JpgStream& s, uint32_t i) { return i < s.nwords ? jpg_bswap(s.words[i]) : 0u; }

// A reader at bit p of the stream: the next 32 .. 64 bits wait in `win` (from its top), and the word behind them is already loaded
// (`ahead`), so that a symbol costs no memory access of its own and the one load per 32 bits has a window's worth of symbols to
// arrive in.  Bits at and behind `end`, and words behind the buffer, read as zero.
struct JpgReader {
    JpgStream s;
    uint32_t end, p, next, have, ahead;
    uint64_t win;
};

JPG_HD void jpg_reader_init(JpgReader* r, const JpgStream& s, uint32_t p, uint32_t end) {
    const uint32_t wi = p >> 5, sh = p & 31;
    r->s = s;
    r->end = end;
    r->p = p;
    r->win = (((uint64_t)jpg_word(s, wi) << 32) | jpg_word(s, wi + 1)) << sh;
    r->have = 64 - sh;
    r->next = wi + 3;
    r->ahead = jpg_word(s, wi + 2);
}

// the 32 bits at p
JPG_HD uint32_t jpg_reader_peek(const JpgReader* r) {
    if (r->p >= r->end) return 0;
    uint32_t v = (uint32_t)(r->win >> 32);
    const uint32_t avail = r->end - r->p;
    if (avail < 32) v &= ~(0xffffffffu >> avail);
    return v;
}

// n in [1, 31]
JPG_HD void jpg_reader_skip(JpgReader* r, uint32_t n) {
    r->win <<= n;
    r->have -= n;
    r->p += n;
    if (r->have < 32) {                                              // have in [1, 31]
        r->win |= (uint64_t)r->ahead << (32 - r->have);
        r->have += 32;
        r->ahead = jpg_word(r->s, r->next);
        r->next += 1;
    }
}

// Decoder position: bit p, block `blk` of the MCU, next coefficient k (zigzag; 0: the block's DC symbol comes next), blocks completed.
struct JpgState {
    uint32_t p, blk, k, nblk;
};

#define JPG_STEP_VALUE 1   /* a coefficient came out: zigzag position *kout, value *val (a DC value is the difference) */
#define JPG_STEP_BLOCK 2   /* the block is complete */
#define JPG_STEP_ERROR 4   /* no such code, or a run past coefficient 63 */

// One Huffman symbol with its extra bits.  tabs: DC tables of components 0..2, then AC tables of components 0..2.  nluma: the luma
// blocks of an MCU (1 for a single-component scan), bpm: all its blocks; r: a reader at st->p.  Always consumes at least one bit.
JPG_HD int jpg_step(const JpgTable* tabs, uint32_t nluma, uint32_t bpm, JpgReader* r, JpgState* st, int* kout, int* val) {
    const uint32_t comp = st->blk < nluma ? 0u : (st->blk - nluma + 1u) & 3u;
    const JpgTable* t = tabs + (st->k == 0 ? comp : 3u + comp);
    const uint32_t w = jpg_reader_peek(r);
    const uint32_t e = t->look[w >> (32 - JPG_LOOK_BITS)];
    int flags = 0;
    uint32_t len, sym;
    if (e) {
        len = e >> 8;
        sym = e & 255u;
    } else {
        int32_t code = 0;
        for (len = JPG_LOOK_BITS + 1; len <= 16; ++len) {
            code = (int32_t)(w >> (32 - len));
            if (code <= t->maxcode[len]) break;
        }
        if (len > 16) {
            len = 16;
            sym = 0;
            flags |= JPG_STEP_ERROR;
        } else {
            sym = t->vals[(t->valoff[len] + code) & 255];
        }
    }
    const uint32_t sbits = sym & 15u, run = sym >> 4;
    int value = 0;
    if (sbits) {
        const uint32_t ext = (w << len) >> (32 - sbits);             // len + sbits <= 31
        value = ext < (1u << (sbits - 1)) ? (int)ext - (int)(1u << sbits) + 1 : (int)ext;
    }
    jpg_reader_skip(r, len + sbits);
    st->p = r->p;
    if (st->k == 0) {
        *kout = 0;
        *val = value;
        flags |= JPG_STEP_VALUE;
        st->k = 1;
    } else if (sbits == 0) {
        st->k = run == 15 ? st->k + 16 : 64;                         // ZRL, else end of block
    } else {
        const uint32_t kk = st->k + run;
        if (kk > 63) {
            flags |= JPG_STEP_ERROR;
            st->k = 64;
        } else {
            *kout = (int)kk;
            *val = value;
            flags |= JPG_STEP_VALUE;
            st->k = kk + 1;
        }
    }
    if (st->k >= 64) {
        st->k = 0;
        st->blk = st->blk + 1 >= bpm ? 0 : st->blk + 1;
        st->nblk += 1;
        flags |= JPG_STEP_BLOCK;
    }
    return flags;
}

// Geometry that follows from the header's fields.
struct JpgGeometry {
    int mcus_x, mcus_y, nluma, bpm, num_blocks, num_intervals, mcus_per_interval;
};

JPG_HD JpgGeometry jpg_geometry(int width, int height, int ncomp, int hs, int vs, int ri) {
    JpgGeometry g;
    if (ncomp == 1) hs = vs = 1;
    g.mcus_x = (width + 8 * hs - 1) / (8 * hs);
    g.mcus_y = (height + 8 * vs - 1) / (8 * vs);
    g.nluma = hs * vs;
    g.bpm = ncomp == 1 ? 1 : g.nluma + 2;
    const int mcus = g.mcus_x * g.mcus_y;
    g.num_blocks = mcus * g.bpm;
    g.mcus_per_interval = ri > 0 ? ri : mcus;
    g.num_intervals = (mcus + g.mcus_per_interval - 1) / g.mcus_per_interval;
    return g;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The marker parser.  0: *H is filled and the file is in the device profile; 1: a well-formed file outside it (msg says why);
// -1: malformed (msg says where).  Reads d[0 .. n) only.
// ---------------------------------------------------------------------------------------------------------------------------------
#define JPG_FAIL(code, ...)                      \
    do {                                         \
        snprintf(msg, msg_bytes, __VA_ARGS__);   \
        return code;                             \
    } while (0)

inline int jpg_parse(const uint8_t* d, int64_t n, hps_jpeg_header* H, char* msg, size_t msg_bytes) {
    static const uint8_t natural[64] = JPG_NATURAL_ORDER;
    if (n < 4 || d[0] != 0xff || d[1] != 0xd8) JPG_FAIL(-1, "not a JPEG file (no SOI marker)");
    if (n >= (1ll << 28)) JPG_FAIL(1, "file of %lld bytes (the device takes files below 2^28 bytes)", (long long)n);
    uint8_t qt[4][64], qt_state[4] = {0, 0, 0, 0};                   // 0: undefined, 1: 8 bit, 2: 16 bit
    hps_jpeg_huff huff[2][4];
    bool huff_set[2][4] = {{false, false, false, false}, {false, false, false, false}};
    bool jfif = false, adobe = false, have_frame = false;
    int adobe_transform = -1, ri = 0, unsupported_frame = 0;
    int width = 0, height = 0, nc = 0, precision = 0, cid[4] = {0, 0, 0, 0}, ch[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0}, ctq[4] = {0, 0, 0, 0};
    int64_t pos = 2;
    for (;;) {
        if (pos >= n) JPG_FAIL(-1, "the file ends at byte %lld before any scan", (long long)pos);
        if (d[pos] != 0xff) JPG_FAIL(-1, "byte %lld: 0x%02x where a marker should start", (long long)pos, d[pos]);
        while (pos < n && d[pos] == 0xff) ++pos;                     // fill bytes
        if (pos >= n) JPG_FAIL(-1, "the file ends inside a marker at byte %lld", (long long)pos);
        const int m = d[pos++];
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;         // TEM, stray RSTn: no payload
        if (m == 0xd8) JPG_FAIL(-1, "a second SOI marker at byte %lld", (long long)pos - 2);
        if (m == 0xd9) JPG_FAIL(-1, "EOI at byte %lld before any scan", (long long)pos - 2);
        if (m == 0x00) JPG_FAIL(-1, "marker FF 00 at byte %lld outside a scan", (long long)pos - 2);
        if (pos + 2 > n) JPG_FAIL(-1, "marker 0x%02x at byte %lld: its length runs past the file", m, (long long)pos - 2);
        const int64_t L = (d[pos] << 8) | d[pos + 1], seg = pos + 2, seg_end = pos + L;
        if (L < 2 || seg_end > n) JPG_FAIL(-1, "marker 0x%02x at byte %lld: length %lld runs past the file", m, (long long)pos - 2, (long long)L);
        if (m == 0xc0 || m == 0xc1) {
            if (have_frame) JPG_FAIL(-1, "a second frame header at byte %lld", (long long)pos - 2);
            if (L < 8) JPG_FAIL(-1, "frame header at byte %lld is too short", (long long)pos - 2);
            precision = d[seg];
            height = (d[seg + 1] << 8) | d[seg + 2];
            width = (d[seg + 3] << 8) | d[seg + 4];
            nc = d[seg + 5];
            if (L != 8 + 3 * nc) JPG_FAIL(-1, "frame header at byte %lld: length %lld for %d components", (long long)pos - 2, (long long)L, nc);
            if (nc < 1 || nc > 4) {
                unsupported_frame = 1;
            } else {
                for (int c = 0; c < nc; ++c) {
                    cid[c] = d[seg + 6 + 3 * c];
                    ch[c] = d[seg + 7 + 3 * c] >> 4;
                    cv[c] = d[seg + 7 + 3 * c] & 15;
                    ctq[c] = d[seg + 8 + 3 * c];
                    if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4 || ctq[c] > 3)
                        JPG_FAIL(-1, "frame header at byte %lld: component %d has sampling %dx%d, table %d", (long long)pos - 2, c, ch[c], cv[c], ctq[c]);
                }
            }
            have_frame = true;
        } else if (m == 0xc4) {
            int64_t q = seg;
            while (q < seg_end) {
                if (q + 17 > seg_end) JPG_FAIL(-1, "DHT at byte %lld: a table runs past the segment", (long long)pos - 2);
                const int tc = d[q] >> 4, th = d[q] & 15;
                if (tc > 1 || th > 3) JPG_FAIL(-1, "DHT at byte %lld: class %d, slot %d", (long long)pos - 2, tc, th);
                int total = 0, code = 0;
                for (int l = 1; l <= 16; ++l) {
                    const int cnt = d[q + l];
                    total += cnt;
                    code += cnt;
                    if (code > (1 << l)) JPG_FAIL(-1, "DHT at byte %lld: the counts of table %d/%d overflow the code space at length %d", (long long)pos - 2, tc, th, l);
                    code <<= 1;
                }
                if (total > 256 || q + 17 + total > seg_end) JPG_FAIL(-1, "DHT at byte %lld: %d symbols run past the segment", (long long)pos - 2, total);
                hps_jpeg_huff* h = &huff[tc][th];
                memset(h, 0, sizeof(*h));
                memcpy(h->bits, d + q + 1, 16);
                memcpy(h->vals, d + q + 17, (size_t)total);
                if (tc == 0)
                    for (int i = 0; i < total; ++i)
                        if (h->vals[i] > 15) JPG_FAIL(-1, "DHT at byte %lld: DC symbol %d", (long long)pos - 2, h->vals[i]);
                huff_set[tc][th] = true;
                q += 17 + total;
            }
        } else if (m == 0xdb) {
            int64_t q = seg;
            while (q < seg_end) {
                const int pq = d[q] >> 4, tq = d[q] & 15;
                if (pq > 1 || tq > 3) JPG_FAIL(-1, "DQT at byte %lld: precision %d, slot %d", (long long)pos - 2, pq, tq);
                const int bytes = pq ? 128 : 64;
                if (q + 1 + bytes > seg_end) JPG_FAIL(-1, "DQT at byte %lld: a table runs past the segment", (long long)pos - 2);
                if (pq == 0)
                    for (int i = 0; i < 64; ++i) qt[tq][natural[i]] = d[q + 1 + i];
                qt_state[tq] = pq ? 2 : 1;
                q += 1 + bytes;
            }
        } else if (m == 0xdd) {
            if (L != 4) JPG_FAIL(-1, "DRI at byte %lld: length %lld", (long long)pos - 2, (long long)L);
            ri = (d[seg] << 8) | d[seg + 1];
        } else if (m == 0xe0) {
            if (L >= 7 && memcmp(d + seg, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xee) {
            if (L >= 14 && memcmp(d + seg, "Adobe", 5) == 0) {
                adobe = true;
                adobe_transform = d[seg + 11];
            }
        } else if (m == 0xda) {
            if (!have_frame) JPG_FAIL(-1, "SOS at byte %lld before a frame header", (long long)pos - 2);
            if (unsupported_frame) JPG_FAIL(1, "%d components", nc);
            if (precision != 8) JPG_FAIL(1, "%d-bit samples", precision);
            if (L < 3) JPG_FAIL(-1, "SOS at byte %lld is too short", (long long)pos - 2);
            const int ns = d[seg];
            if (ns < 1 || ns > 4 || L != 6 + 2 * ns) JPG_FAIL(-1, "SOS at byte %lld: length %lld for %d components", (long long)pos - 2, (long long)L, ns);
            if (nc != 1 && nc != 3) JPG_FAIL(1, "%d components (CMYK / YCCK)", nc);
            if (ns != nc) JPG_FAIL(1, "a scan of %d of %d components (several scans)", ns, nc);
            if (d[seg + 1 + 2 * ns] != 0 || d[seg + 2 + 2 * ns] != 63 || d[seg + 3 + 2 * ns] != 0)
                JPG_FAIL(1, "a scan with Ss %d, Se %d, Ah/Al 0x%02x", d[seg + 1 + 2 * ns], d[seg + 2 + 2 * ns], d[seg + 3 + 2 * ns]);
            if (width < 1 || height < 1) JPG_FAIL(1, "size %d x %d in the frame header", width, height);
            if (width > HPS_JPEG_MAX_DIM || height > HPS_JPEG_MAX_DIM) JPG_FAIL(1, "size %d x %d (limit %d)", width, height, HPS_JPEG_MAX_DIM);
            memset(H, 0, sizeof(*H));
            for (int c = 0; c < ns; ++c) {
                const int sel = d[seg + 1 + 2 * c], td = d[seg + 2 + 2 * c] >> 4, ta = d[seg + 2 + 2 * c] & 15;
                bool found = false;
                for (int f = 0; f < nc; ++f) found = found || cid[f] == sel;
                if (!found) JPG_FAIL(-1, "SOS at byte %lld selects component %d, which the frame does not have", (long long)pos - 2, sel);
                if (sel != cid[c]) JPG_FAIL(1, "scan components in another order than the frame's");
                if (td > 3 || ta > 3 || !huff_set[0][td] || !huff_set[1][ta])
                    JPG_FAIL(-1, "SOS at byte %lld selects Huffman tables %d/%d, which are not defined", (long long)pos - 2, td, ta);
                if (qt_state[ctq[c]] == 0) JPG_FAIL(-1, "component %d selects quantisation table %d, which is not defined", c, ctq[c]);
                if (qt_state[ctq[c]] == 2) JPG_FAIL(1, "a 16-bit quantisation table");
                H->dc[c] = huff[0][td];
                H->ac[c] = huff[1][ta];
                for (int i = 0; i < 64; ++i) H->quant[c][i] = qt[ctq[c]][i];
            }
            if (nc == 3) {
                if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || !((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2)))
                    JPG_FAIL(1, "sampling %dx%d, %dx%d, %dx%d", ch[0], cv[0], ch[1], cv[1], ch[2], cv[2]);
                if (!jfif) {
                    if (adobe) {
                        if (adobe_transform != 1) JPG_FAIL(1, "Adobe transform %d", adobe_transform);
                    } else if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') {
                        JPG_FAIL(1, "component ids R, G, B (an RGB file)");
                    }
                }
            }
            // the entropy-coded bytes: up to the first marker that is neither stuffing nor RSTn, or the end of the file
            int64_t q = seg_end;
            const int64_t scan_offset = q;
            int end_marker = -1;
            while (q < n) {
                const uint8_t* f = (const uint8_t*)memchr(d + q, 0xff, (size_t)(n - q));
                if (!f) {
                    q = n;
                    break;
                }
                q = f - d;
                if (q + 1 >= n) {
                    q = n;
                    break;
                }
                const int x = d[q + 1];
                if (x == 0 || (x >= 0xd0 && x <= 0xd7)) {
                    q += 2;
                    continue;
                }
                if (x == 0xff) JPG_FAIL(1, "fill bytes inside the scan");
                end_marker = x;
                break;
            }
            if (end_marker != -1 && end_marker != 0xd9) JPG_FAIL(1, "marker 0x%02x after the scan (several scans)", end_marker);
            if (q - scan_offset > HPS_JPEG_MAX_SCAN_BYTES)
                JPG_FAIL(1, "%lld bytes of entropy-coded data (the device takes %d)", (long long)(q - scan_offset), HPS_JPEG_MAX_SCAN_BYTES);
            H->struct_bytes = (int)sizeof(*H);
            H->width = width;
            H->height = height;
            H->ncomp = nc;
            H->hs = nc == 1 ? 1 : ch[0];
            H->vs = nc == 1 ? 1 : cv[0];
            H->restart_interval = ri;
            H->scan_offset = (int)scan_offset;
            H->scan_length = (int)(q - scan_offset);
            const JpgGeometry g = jpg_geometry(width, height, nc, H->hs, H->vs, ri);
            H->num_blocks = g.num_blocks;
            H->num_intervals = g.num_intervals;
            H->file_bytes = (int)n;
            return 0;
        } else if ((m >= 0xc2 && m <= 0xcf) && m != 0xc8) {
            JPG_FAIL(1, "%s (SOF marker 0x%02x)", m == 0xc2 ? "progressive" : m == 0xc3 ? "lossless" : m == 0xcc || m >= 0xc9 ? "arithmetic coding" : "differential", m);
        }
        pos = seg_end;                                               // APPn, COM and everything else: skipped
    }
}
#undef JPG_FAIL
