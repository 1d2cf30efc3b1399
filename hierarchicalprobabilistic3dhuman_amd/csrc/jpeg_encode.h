// Baseline JPEG encoding, block by block (host and device): where a block lies in the scan, its samples with the padding rules, colour
// conversion and down-sampling, libjpeg's accurate integer forward DCT, quantisation, a block's bit count and bits with the Annex K
// Huffman tables, the file's header and byte stuffing.  One source for csrc/jpeg_encode.hip's kernels and the stand-alone host check
// (tests/jpeg_encode_host_check.cpp), which builds whole files from exactly these functions on the CPU under the sanitizers.
// include/hps.h (hps_jpeg_encode) states the file these functions make.  No allocation, no global state.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPE_HD __host__ __device__ inline
#else
#define JPE_HD inline
#endif

// A block before stuffing: a DC code of at most 11 bits (the chrominance table's category 11) and 11 magnitude bits, 63 AC codes of at
// most 16 bits with 10 magnitude bits each.
#define JPE_MAX_BLOCK_BITS (22 + 63 * 26)
#define JPE_MAX_HEADER 640

struct JpeTables {
    uint8_t natural[64];                   // zig-zag position -> natural (row-major) position
    uint8_t zigzag[64];                    // natural position -> zig-zag position
    uint8_t base[2][64];                   // Annex K quantisation tables, natural order: luminance, chrominance
    uint8_t dc_bits[2][16], ac_bits[2][16];
    uint8_t dc_vals[2][12], ac_vals[2][162];
    uint16_t dc_code[2][12], ac_code[2][256];      // by symbol
    uint8_t dc_len[2][12], ac_len[2][256];
};

constexpr JpeTables jpe_make_tables() {
    JpeTables t{};
    constexpr uint8_t natural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                     41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                     30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    constexpr uint8_t luma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                  69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                  81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    constexpr uint8_t chroma[16] = {17, 18, 24, 47, 18, 21, 26, 66, 24, 26, 56, 99, 47, 66, 99, 99};      // the top-left 4 x 4; 99 elsewhere
    constexpr uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    constexpr uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
    constexpr uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1,
         0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26,
         0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56,
         0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85,
         0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA,
         0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
         0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
         0xFA},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
         0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19,
         0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55,
         0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8,
         0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4,
         0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9,
         0xFA}};
    for (int i = 0; i < 64; ++i) {
        t.natural[i] = natural[i];
        t.zigzag[natural[i]] = (uint8_t)i;
        t.base[0][i] = luma[i];
        t.base[1][i] = (i / 8 < 4 && i % 8 < 4) ? chroma[(i / 8) * 4 + i % 8] : 99;
    }
    for (int k = 0; k < 2; ++k) {
        for (int i = 0; i < 16; ++i) {
            t.dc_bits[k][i] = dc_bits[k][i];
            t.ac_bits[k][i] = ac_bits[k][i];
        }
        for (int i = 0; i < 12; ++i) t.dc_vals[k][i] = (uint8_t)i;
        for (int i = 0; i < 162; ++i) t.ac_vals[k][i] = ac_vals[k][i];
        // canonical codes: the symbols of each length in the order listed, codes counting up, doubled from length to length
        int code = 0, n = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int j = 0; j < dc_bits[k][l - 1]; ++j, ++n, ++code) {
                t.dc_code[k][n] = (uint16_t)code;
                t.dc_len[k][n] = (uint8_t)l;
            }
            code <<= 1;
        }
        code = 0;
        n = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int j = 0; j < ac_bits[k][l - 1]; ++j, ++n, ++code) {
                t.ac_code[k][ac_vals[k][n]] = (uint16_t)code;
                t.ac_len[k][ac_vals[k][n]] = (uint8_t)l;
            }
            code <<= 1;
        }
    }
    return t;
}

// ---- where things are -----------------------------------------------------------------------------------------------------------
struct JpeGeometry {
    int H, W, C;
    int hmax, vmax;                        // luminance's sampling factors; chrominance is 1 x 1
    int mx, my;                            // MCUs across and down
    int bpm;                               // blocks per MCU
    int bw[2], bh[2];                      // the block grid of luminance and of a chrominance component
    int nblk;                              // blocks in the scan, dummies included
};

JPE_HD JpeGeometry jpe_geometry(int H, int W, int C, int sampling) {
    JpeGeometry g;
    g.H = H; g.W = W; g.C = C;
    g.hmax = (C == 3 && sampling >= 1) ? 2 : 1;
    g.vmax = (C == 3 && sampling == 2) ? 2 : 1;
    g.mx = (W + 8 * g.hmax - 1) / (8 * g.hmax);
    g.my = (H + 8 * g.vmax - 1) / (8 * g.vmax);
    g.bpm = C == 3 ? g.hmax * g.vmax + 2 : 1;
    g.bw[0] = (W + 7) / 8;
    g.bh[0] = (H + 7) / 8;
    g.bw[1] = ((W + g.hmax - 1) / g.hmax + 7) / 8;
    g.bh[1] = ((H + g.vmax - 1) / g.vmax + 7) / 8;
    g.nblk = g.mx * g.my * g.bpm;
    return g;
}

struct JpeBlock {
    int comp;                              // 0 luminance, 1 Cb, 2 Cr
    int bx, by;                            // the block in its component's grid
    int source;                            // a real block: its own scan index; a dummy: the real block whose DC it repeats
    int pred;                              // the block before it of the same component in scan order, -1: none
};

JPE_HD bool jpe_luma_is_real(const JpeGeometry& g, int mcol, int mrow, int k) {
    return mcol * g.hmax + k % g.hmax < g.bw[0] && mrow * g.vmax + k / g.hmax < g.bh[0];
}

// block i of the scan: MCUs in raster order; in an MCU luminance's blocks row by row, then Cb, then Cr
JPE_HD JpeBlock jpe_block(const JpeGeometry& g, int i) {
    JpeBlock b;
    const int mcu = i / g.bpm, k = i - mcu * g.bpm, nl = g.C == 3 ? g.bpm - 2 : 1;
    const int mrow = mcu / g.mx, mcol = mcu - mrow * g.mx;
    if (k < nl) {
        b.comp = 0;
        b.bx = mcol * g.hmax + k % g.hmax;
        b.by = mrow * g.vmax + k / g.hmax;
        int s = k;                                                           // block 0 of an MCU is always real
        for (int step = 0; step < 3 && !jpe_luma_is_real(g, mcol, mrow, s); ++step) --s;
        b.source = i - k + s;
        b.pred = k > 0 ? i - 1 : (mcu > 0 ? i - g.bpm + nl - 1 : -1);
    } else {
        b.comp = 1 + k - nl;
        b.bx = mcol;
        b.by = mrow;
        b.source = i;
        b.pred = mcu > 0 ? i - g.bpm : -1;
    }
    return b;
}

// ---- samples --------------------------------------------------------------------------------------------------------------------
// component comp of pixel (x, y), both inside the picture; 16.16 fixed point
JPE_HD int jpe_component(const uint8_t* px, int W, int C, int comp, int x, int y) {
    const uint8_t* p = px + ((int64_t)y * W + x) * C;
    if (C == 1) return p[0];
    const int R = p[0], G = p[1], B = p[2];
    if (comp == 0) return (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    if (comp == 1) return (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    return (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
}

// Sample (x, y) of a component's padded plane (x, y in block-grid samples).  The full-resolution plane repeats its last column to the
// right and its last row down to a multiple of vmax rows; the down-sampled plane then repeats ITS last row.
JPE_HD int jpe_sample(const uint8_t* px, const JpeGeometry& g, int comp, int x, int y) {
    const int fx = comp == 0 ? 1 : g.hmax, fy = comp == 0 ? 1 : g.vmax;
    const int rows = (g.H + fy - 1) / fy;                                    // the component's real rows
    if (y > rows - 1) y = rows - 1;
    const int W1 = g.W - 1, H1 = g.H - 1;
    if (fx == 1) return jpe_component(px, g.W, g.C, comp, x < W1 ? x : W1, y < H1 ? y : H1);
    const int x0 = 2 * x < W1 ? 2 * x : W1, x1 = 2 * x + 1 < W1 ? 2 * x + 1 : W1;
    if (fy == 1) return (jpe_component(px, g.W, g.C, comp, x0, y) + jpe_component(px, g.W, g.C, comp, x1, y) + (x & 1)) >> 1;
    const int y0 = 2 * y, y1 = 2 * y + 1 < H1 ? 2 * y + 1 : H1;             // 2 y <= H - 1 by the clamp above
    return (jpe_component(px, g.W, g.C, comp, x0, y0) + jpe_component(px, g.W, g.C, comp, x1, y0) +
            jpe_component(px, g.W, g.C, comp, x0, y1) + jpe_component(px, g.W, g.C, comp, x1, y1) + 1 + (x & 1)) >> 2;
}

// ---- the forward DCT (libjpeg's jfdctint: 13-bit constants, two pass-1 bits, rows then columns, the result scaled by 8) ------------
JPE_HD void jpe_fdct_1d(int* d, int stride, bool first) {
    const int n = first ? 11 : 15, half = 1 << (n - 1);
    const int d0 = d[0], d1 = d[stride], d2 = d[2 * stride], d3 = d[3 * stride], d4 = d[4 * stride], d5 = d[5 * stride], d6 = d[6 * stride],
              d7 = d[7 * stride];
    int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = first ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
    d[4 * stride] = first ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
    int z1 = (t12 + t13) * 4433;
    d[2 * stride] = (z1 + t13 * 6270 + half) >> n;
    d[6 * stride] = (z1 - t12 * 15137 + half) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * stride] = (t4 + z1 + z3 + half) >> n;
    d[5 * stride] = (t5 + z2 + z4 + half) >> n;
    d[3 * stride] = (t6 + z2 + z3 + half) >> n;
    d[stride] = (t7 + z1 + z4 + half) >> n;
}

// d: 64 samples minus 128, row-major, in place
JPE_HD void jpe_fdct(int* d) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 8; ++r) jpe_fdct_1d(d + 8 * r, 1, true);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; ++c) jpe_fdct_1d(d + c, 8, false);
}

// quantisation table entry: the Annex K value scaled by the quality
JPE_HD int jpe_quant(int base, int quality) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : (q > 255 ? 255 : q);
}

// a coefficient scaled by 8 to its quantised value
JPE_HD int jpe_quantise(int c, int q) {
    const int d = 8 * q, a = c < 0 ? -c : c;
    const int v = (a + (d >> 1)) / d;
    return c < 0 ? -v : v;
}

// ---- the entropy code -----------------------------------------------------------------------------------------------------------
JPE_HD int jpe_size(int v) {               // bits of |v|
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

// the AC part's bit count; zz: the block in zig-zag order
JPE_HD int jpe_ac_bits(const JpeTables& T, int table, const int16_t* zz) {
    int bits = 0, run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { bits += T.ac_len[table][0xF0]; run -= 16; }
        const int s = jpe_size(v);
        bits += T.ac_len[table][((run << 4) | s) & 255] + s;
        run = 0;
    }
    if (run) bits += T.ac_len[table][0];
    return bits;
}

JPE_HD int jpe_dc_bits(const JpeTables& T, int table, int diff) {
    const int s = jpe_size(diff);
    return T.dc_len[table][s < 12 ? s : 11] + s;
}

// A block's bits into a sink: put(value, count), count <= 27, most significant bit first.
template <class Sink>
JPE_HD void jpe_block_bits(const JpeTables& T, int table, const int16_t* zz, int diff, Sink& sink) {
    int s = jpe_size(diff);
    if (s > 11) s = 11;
    uint32_t m = (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1);
    sink.put(((uint32_t)T.dc_code[table][s] << s) | m, T.dc_len[table][s] + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { sink.put(T.ac_code[table][0xF0], T.ac_len[table][0xF0]); run -= 16; }
        s = jpe_size(v);
        const int sym = ((run << 4) | s) & 255;
        m = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1);
        sink.put(((uint32_t)T.ac_code[table][sym] << s) | m, T.ac_len[table][sym] + s);
        run = 0;
    }
    if (run) sink.put(T.ac_code[table][0], T.ac_len[table][0]);
}

// Bits into 32-bit words, bit p of the stream at bit 31 - (p & 31) of word p >> 5: byte j of the stream is byte 3 - (j & 3) of word
// j >> 2.  The words start zeroed; or(word index, bits) is a plain OR on the host and an atomic OR in LDS on the device.
template <class Or>
struct JpeWordSink {
    Or o;
    uint32_t pos;
    JPE_HD void put(uint32_t v, int nb) {
        const uint64_t x = (uint64_t)v << (64 - (pos & 31) - nb);
        o((pos >> 5), (uint32_t)(x >> 32));
        if ((uint32_t)x) o((pos >> 5) + 1, (uint32_t)x);
        pos += nb;
    }
};

// ---- the file -------------------------------------------------------------------------------------------------------------------
JPE_HD int jpe_header_bytes(int C) { return C == 3 ? 623 : 328; }

// SOI, APP0, DQT ..., SOF0, DHT ..., SOS into dst (JPE_MAX_HEADER bytes); returns the length
JPE_HD int jpe_header(const JpeTables& T, uint8_t* dst, int H, int W, int C, int quality, int sampling) {
    const JpeGeometry g = jpe_geometry(H, W, C, sampling);
    int n = 0;
    const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; ++i) dst[n++] = app0[i];
    for (int t = 0; t < (C == 3 ? 2 : 1); ++t) {
        dst[n++] = 0xFF; dst[n++] = 0xDB; dst[n++] = 0; dst[n++] = 67; dst[n++] = (uint8_t)t;
        for (int k = 0; k < 64; ++k) dst[n++] = (uint8_t)jpe_quant(T.base[t][T.natural[k]], quality);
    }
    dst[n++] = 0xFF; dst[n++] = 0xC0; dst[n++] = 0; dst[n++] = (uint8_t)(8 + 3 * C); dst[n++] = 8;
    dst[n++] = (uint8_t)(H >> 8); dst[n++] = (uint8_t)H; dst[n++] = (uint8_t)(W >> 8); dst[n++] = (uint8_t)W; dst[n++] = (uint8_t)C;
    for (int c = 0; c < C; ++c) {
        dst[n++] = (uint8_t)(c + 1);
        dst[n++] = c == 0 ? (uint8_t)((g.hmax << 4) | g.vmax) : 0x11;
        dst[n++] = c == 0 ? 0 : 1;
    }
    for (int t = 0; t < (C == 3 ? 2 : 1); ++t)
        for (int ac = 0; ac < 2; ++ac) {
            const int count = ac ? 162 : 12;
            dst[n++] = 0xFF; dst[n++] = 0xC4; dst[n++] = 0; dst[n++] = (uint8_t)(19 + count); dst[n++] = (uint8_t)((ac << 4) | t);
            for (int i = 0; i < 16; ++i) dst[n++] = ac ? T.ac_bits[t][i] : T.dc_bits[t][i];
            for (int i = 0; i < count; ++i) dst[n++] = ac ? T.ac_vals[t][i] : T.dc_vals[t][i];
        }
    dst[n++] = 0xFF; dst[n++] = 0xDA; dst[n++] = 0; dst[n++] = (uint8_t)(6 + 2 * C); dst[n++] = (uint8_t)C;
    for (int c = 0; c < C; ++c) {
        dst[n++] = (uint8_t)(c + 1);
        dst[n++] = c == 0 ? 0x00 : 0x11;
    }
    dst[n++] = 0; dst[n++] = 63; dst[n++] = 0;
    return n;
}

// raw[0 .. n) with 00 behind every FF; returns the bytes written (at most 2 n)
JPE_HD int64_t jpe_stuff(const uint8_t* raw, int64_t n, uint8_t* dst) {
    int64_t m = 0;
    for (int64_t i = 0; i < n; ++i) {
        dst[m++] = raw[i];
        if (raw[i] == 0xFF) dst[m++] = 0;
    }
    return m;
}

// A capacity no file exceeds: the header, every block at JPE_MAX_BLOCK_BITS and the final padding, every byte of that doubled by
// stuffing, EOI.
JPE_HD int64_t jpe_bound(int H, int W, int C, int sampling) {
    const JpeGeometry g = jpe_geometry(H, W, C, sampling);
    return jpe_header_bytes(C) + 2 * (((int64_t)g.nblk * JPE_MAX_BLOCK_BITS + 7) / 8) + 2;
}
