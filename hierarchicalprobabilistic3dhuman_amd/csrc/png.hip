// PNG files made on the device (no reference counterpart: the reference hands its pictures to cv2.imwrite on the host).  A finished
// (H, W, C) uint8 picture becomes the bytes of a complete file -- signature, IHDR, IDAT ..., IEND, every chunk CRC and the zlib
// Adler-32 formed here -- so that only the compressed file crosses to the host.  Two launches per call, whatever the number of
// pictures (hps_png_encode, include/hps.h):
//   png_segment_kernel   one workgroup per SEGMENT of whole rows (at most PNG_SEG_BYTES filtered bytes, at most PNG_MAX_SEG_ROWS
//                        rows).  It filters the rows (Sub or Up per row, by the smaller sum of absolute values; the row above comes
//                        from global memory, so segments are independent), tokenises the filtered bytes without a sequential parse
//                        (runs of "equals the byte before" become distance-1 matches), codes them with deflate's fixed Huffman
//                        tables into an LDS bit buffer, closes the segment with an empty stored block (a sync flush: it ends on a
//                        byte boundary), falls back to one stored block when that is shorter, and leaves the segment as a complete
//                        IDAT chunk -- length, type, data, CRC -- in its slot of the workspace, with its Adler-32 sums.
//   png_assemble_kernel  one workgroup per segment again: the exclusive sum of the chunk lengths before it places the chunk in the
//                        file; the first also writes signature, IHDR and the two-byte zlib header chunk, the last the closing chunk
//                        (final empty fixed block + Adler-32), IEND and the file length.
// No global atomics; the LDS atomics are integer OR / XOR / ADD, whose results do not depend on arrival order.  Every loop bound is a
// function of the sizes.
#include "hps_common.h"

namespace {

constexpr int PNG_THREADS = 256;
constexpr int PNG_SEG_BYTES = 16384;      // filtered bytes of one segment at most (filter bytes included)
constexpr int PNG_MAX_SEG_ROWS = 64;      // rows of one segment at most (the per-row filter sums live in LDS)
constexpr int PNG_MAX_ROW = 12288;        // W C at most: 4096 RGB pixels
constexpr int PNG_MAX_H = 32768;
// raw bytes staged per segment: its rows and the row above, from the 16-byte boundary below to the one above.  One row per segment:
// 2 PNG_MAX_ROW; two or more: the row is at most PNG_SEG_BYTES / 2, so (R + 1) W C <= 1.5 PNG_SEG_BYTES -- both 24 576.
constexpr int PNG_RAW_LDS = 24576 + 32;
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;
constexpr uint32_t ADLER_MOD = 65521u;
constexpr int PNG_PROLOGUE = 8 + 25 + 14; // signature, IHDR chunk, the IDAT chunk holding the zlib header 78 01
constexpr int PNG_EPILOGUE = 18 + 12;     // the IDAT chunk holding 03 00 + Adler-32, IEND

struct PngPic {
    const uint8_t* px;
    uint8_t* ws;
    uint8_t* out;
    long long* length;
    int H, W, C, R, nseg, seg0;           // R rows per segment, nseg segments, seg0 = segments of the pictures before this one
};
struct PngParams {
    PngPic pic[HPS_PNG_MAX_IMAGES];
    int n;
};

inline int seg_rows(int W, int C) {
    const int r = PNG_SEG_BYTES / (1 + W * C);
    return r < 1 ? 1 : (r > PNG_MAX_SEG_ROWS ? PNG_MAX_SEG_ROWS : r);
}
inline bool supported(int H, int W, int C) {
    return (C == 1 || C == 3) && H >= 1 && H <= PNG_MAX_H && W >= 1 && W <= PNG_MAX_ROW && W * C <= PNG_MAX_ROW;
}
__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// workspace of one picture: len / sum-a / sum-b (uint32 each) per segment, then one slot per segment
__host__ __device__ inline int64_t ws_meta_bytes(int nseg) { return align16((int64_t)nseg * 12); }
__host__ __device__ inline int64_t ws_slot_bytes(int R, int rb) { return align16((int64_t)R * rb + 17); }

// ---- CRC-32 arithmetic in the reflected representation (bit 31 is x^0) ---------------------------------------------------------
__host__ __device__ constexpr uint32_t multmodp(uint32_t a, uint32_t b) {      // a b mod P
    uint32_t p = 0;
    for (int j = 0; j < 32; ++j) {
        if (a & (0x80000000u >> j)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1;
    }
    return p;
}
struct X2N {
    uint32_t v[32];                                                              // x^(2^k) mod P
};
constexpr X2N make_x2n() {
    X2N t{};
    uint32_t p = 0x40000000u;                                                    // x^1
    t.v[0] = p;
    for (int k = 1; k < 32; ++k) t.v[k] = p = multmodp(p, p);
    return t;
}
__constant__ X2N c_x2n = make_x2n();

__device__ inline uint32_t x8n_modp(uint32_t nbytes) {                          // x^(8 nbytes) mod P; nbytes < 2^20
    uint32_t p = 0x80000000u;
    for (int k = 0; k < 20; ++k)
        if ((nbytes >> k) & 1) p = multmodp(c_x2n.v[k + 3], p);
    return p;
}
__device__ inline uint32_t crc_table_entry(uint32_t i) {
    for (int k = 0; k < 8; ++k) i = (i & 1) ? (i >> 1) ^ PNG_CRC_POLY : i >> 1;
    return i;
}
__device__ inline uint32_t crc_bitwise(const uint8_t* p, int n) {               // the finished CRC-32 of a few bytes, by one lane
    uint32_t c = 0xFFFFFFFFu;
    for (int i = 0; i < n; ++i) c = crc_table_entry((c ^ p[i]) & 0xFF) ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}
__device__ inline void put_be32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// ---- workgroup scans over one value per lane (Hillis-Steele in LDS; 256 lanes) ---------------------------------------------------
struct OpAdd { __device__ static int f(int a, int b) { return a + b; } };
struct OpMax { __device__ static int f(int a, int b) { return a > b ? a : b; } };
struct OpMin { __device__ static int f(int a, int b) { return a < b ? a : b; } };
// exclusive scan in lane order (reverse: from the last lane down); *total, if wanted, receives the reduction over all lanes
template <class Op>
__device__ int block_scan_excl(int v, int identity, int* s, bool reverse, int* total) {
    const int idx = reverse ? PNG_THREADS - 1 - (int)threadIdx.x : (int)threadIdx.x;
    s[idx] = v;
    for (int off = 1; off < PNG_THREADS; off <<= 1) {
        __syncthreads();
        const int t = idx >= off ? s[idx - off] : identity;
        __syncthreads();
        s[idx] = Op::f(s[idx], t);
    }
    __syncthreads();
    const int r = idx > 0 ? s[idx - 1] : identity;
    if (total) *total = s[PNG_THREADS - 1];
    __syncthreads();
    return r;
}

// ---- deflate's fixed Huffman code -------------------------------------------------------------------------------------------------
__device__ inline int literal_bits(uint32_t v) { return v < 144 ? 8 : 9; }
__device__ inline void length_symbol(int L, int& sym, int& eb, int& extra) {    // L in [3, 258]
    const int l = L - 3;
    if (L == 258) { sym = 285; eb = 0; extra = 0; }
    else if (l < 8) { sym = 257 + l; eb = 0; extra = 0; }
    else {
        eb = (31 - __clz(l)) - 2;
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        extra = l & ((1 << eb) - 1);
    }
}
__device__ inline int match_bits(int L) {
    int sym, eb, extra;
    length_symbol(L, sym, eb, extra);
    return (sym < 280 ? 7 : 8) + eb + 5;                                         // + the 5-bit code of distance 1
}

struct CountSink {
    int bits = 0;
    __device__ void literal(uint32_t v) { bits += literal_bits(v); }
    __device__ void match(int L) { bits += match_bits(L); }
};
struct EmitSink {
    uint32_t* w;
    uint32_t pos;
    __device__ void put(uint32_t v, int nb) {                                   // nb <= 18 bits, already in stream order (LSB first)
        const uint64_t x = (uint64_t)v << (pos & 31);
        atomicOr(&w[pos >> 5], (uint32_t)x);
        const uint32_t hi = (uint32_t)(x >> 32);
        if (hi) atomicOr(&w[(pos >> 5) + 1], hi);
        pos += nb;
    }
    __device__ void literal(uint32_t v) {                                       // Huffman codes go in most significant bit first
        if (v < 144) put(__brev(0x30u + v) >> 24, 8);
        else put(__brev(0x190u + (v - 144)) >> 23, 9);
    }
    __device__ void match(int L) {
        int sym, eb, extra;
        length_symbol(L, sym, eb, extra);
        const int cb = sym < 280 ? 7 : 8;
        const uint32_t code = sym < 280 ? __brev((uint32_t)(sym - 256)) >> 25 : __brev(0xC0u + (sym - 280)) >> 24;
        put(code | ((uint32_t)extra << cb), cb + eb + 5);                        // extra bits LSB first; distance 1 is code 00000
    }
};

// The tokens of filtered bytes [b0, b1) of a segment of S bytes.  flag(i) = byte i equals byte i - 1 (never at i = 0, so no match
// reaches before the segment).  A maximal run of L flagged bytes after an unflagged byte p is cut into pieces of 258 from its start;
// a piece of at least 3 is one match (length, distance 1) emitted by its first byte, a shorter last piece is literals; every
// unflagged byte is a literal.  prevz = the last unflagged position before b0, nextz = the first unflagged position at or after b1
// (S if none).
template <class Sink>
__device__ void walk_tokens(const uint8_t* filt, int b0, int b1, int prevz, int nextz, Sink& sink) {
    int p = prevz, e = -1;
    for (int i = b0; i < b1; ++i) {
        const uint32_t v = filt[i];
        if (i == 0 || v != filt[i - 1]) { p = i; sink.literal(v); continue; }
        if (e <= i) {                                                            // the end of this run: each run is searched once
            e = nextz;
            for (int j = i + 1; j < b1; ++j)
                if (filt[j] != filt[j - 1]) { e = j; break; }
        }
        const int L = e - p - 1, k = i - p - 1;
        const int q = k / 258, off = k - q * 258;
        const int piece = min(258, L - q * 258);
        if (piece < 3) sink.literal(v);
        else if (off == 0) sink.match(piece);
    }
}

__device__ inline const PngPic& find_picture(const PngParams& P, int block) {
    int p = 0;
    for (int i = 1; i < HPS_PNG_MAX_IMAGES; ++i)
        if (i < P.n && block >= P.pic[i].seg0) p = i;
    return P.pic[p];
}

__global__ void __launch_bounds__(PNG_THREADS) png_segment_kernel(const PngParams P) {
    __shared__ uint4 s_img4[PNG_RAW_LDS / 16];             // first the raw rows, then the finished chunk
    __shared__ __attribute__((aligned(16))) uint8_t s_filt[PNG_SEG_BYTES];
    __shared__ uint32_t s_crc[256];
    __shared__ int s_scan[PNG_THREADS];
    __shared__ uint32_t s_rowsum[PNG_MAX_SEG_ROWS][2];
    __shared__ uint32_t s_red[3];                          // Adler sum a, sum b, the chunk's CRC register
    uint8_t* const s_img = reinterpret_cast<uint8_t*>(s_img4);
    uint32_t* const s_words = reinterpret_cast<uint32_t*>(s_img4);

    const PngPic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x;
    const int seg = blockIdx.x - pic.seg0;
    const int WC = pic.W * pic.C, rb = WC + 1, C = pic.C;
    const int row0 = seg * pic.R, rows = min(pic.R, pic.H - row0);
    const int S = rows * rb;
    const uint8_t* px = pic.px;

    // stage the raw rows and the row above with 16-byte loads (px is 16-byte aligned)
    const int total = pic.H * WC;
    const int gstart = (row0 > 0 ? row0 - 1 : 0) * WC, gend = (row0 + rows) * WC;
    const int a0 = gstart & ~15;
    for (int u = tid; a0 + 16 * u < gend; u += PNG_THREADS) {
        const int addr = a0 + 16 * u;
        if (addr + 16 <= total) s_img4[u] = *reinterpret_cast<const uint4*>(px + addr);
        else
            for (int b = 0; b < 16; ++b) s_img[16 * u + b] = addr + b < total ? px[addr + b] : 0;
    }
    s_crc[tid] = crc_table_entry(tid);
    if (tid < PNG_MAX_SEG_ROWS) s_rowsum[tid][0] = s_rowsum[tid][1] = 0;
    if (tid < 3) s_red[tid] = 0;
    __syncthreads();

    const int K = hps::ceil_div(S, PNG_THREADS);
    const int b0 = min(S, tid * K), b1 = min(S, b0 + K);
    const uint8_t* raw = s_img - a0;                       // raw[g] = byte g of the picture

    // the filter of every row: sums of |Sub| and |Up| residuals, read as signed bytes
    {
        int r = b0 / rb, c = b0 - r * rb;
        uint32_t asub = 0, aup = 0;
        for (int i = b0; i < b1; ++i) {
            if (c > 0) {
                const int x = c - 1, g = (row0 + r) * WC + x;
                const int cur = raw[g], left = x >= C ? raw[g - C] : 0, up = row0 + r > 0 ? raw[g - WC] : 0;
                const int ds = (cur - left) & 255, du = (cur - up) & 255;
                asub += ds < 128 ? ds : 256 - ds;
                aup += du < 128 ? du : 256 - du;
            }
            if (++c == rb || i + 1 == b1) {
                atomicAdd(&s_rowsum[r][0], asub);
                atomicAdd(&s_rowsum[r][1], aup);
                asub = aup = 0;
                if (c == rb) { c = 0; ++r; }
            }
        }
    }
    __syncthreads();
    // the filtered bytes and their Adler-32 sums: a = sum v, b = sum (S - i) v
    {
        int r = b0 / rb, c = b0 - r * rb;
        uint32_t sa = 0, sb = 0;
        for (int i = b0; i < b1; ++i) {
            const bool sub = s_rowsum[r][0] < s_rowsum[r][1];
            uint32_t v;
            if (c == 0) v = sub ? 1 : 2;
            else {
                const int x = c - 1, g = (row0 + r) * WC + x;
                const int cur = raw[g];
                const int ref = sub ? (x >= C ? raw[g - C] : 0) : (row0 + r > 0 ? raw[g - WC] : 0);
                v = (cur - ref) & 255;
            }
            s_filt[i] = (uint8_t)v;
            sa += v;
            sb += (uint32_t)(S - i) * v;                   // <= 64 bytes per lane: below 2^32
            if (++c == rb) { c = 0; ++r; }
        }
        atomicAdd(&s_red[0], sa % ADLER_MOD);
        atomicAdd(&s_red[1], sb % ADLER_MOD);
    }
    __syncthreads();

    // tokens: where the unflagged bytes are, bits per lane, bit positions
    int lastz = -1, firstz = S;
    for (int i = b0; i < b1; ++i)
        if (i == 0 || s_filt[i] != s_filt[i - 1]) {
            lastz = i;
            if (firstz == S) firstz = i;
        }
    const int prevz = block_scan_excl<OpMax>(lastz, -1, s_scan, false, nullptr);
    const int nextz = block_scan_excl<OpMin>(firstz, S, s_scan, true, nullptr);
    CountSink count;
    walk_tokens(s_filt, b0, b1, prevz, nextz, count);
    int token_bits = 0;
    const int pos = block_scan_excl<OpAdd>(count.bits, 0, s_scan, false, &token_bits);

    // fixed block: 3 header bits, the tokens, end of block (7), an empty stored block (3 bits, pad, 00 00 FF FF); or one stored block
    const int nfixed = (3 + token_bits + 7 + 3 + 7) / 8 + 4;
    const bool stored = nfixed > S + 5;
    const int n = stored ? S + 5 : nfixed;
    const int units = (12 + n + 15) / 16;
    for (int u = tid; u < units; u += PNG_THREADS) s_img4[u] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    if (stored) {
        for (int i = tid; i < S; i += PNG_THREADS) s_img[13 + i] = s_filt[i];
        if (tid == 0) {
            s_img[8] = 0;                                  // BFINAL = 0, BTYPE = 00
            s_img[9] = (uint8_t)S; s_img[10] = (uint8_t)(S >> 8);
            s_img[11] = (uint8_t)~S; s_img[12] = (uint8_t)(~S >> 8);
        }
    } else {
        EmitSink emit{s_words, (uint32_t)(64 + 3 + pos)};
        walk_tokens(s_filt, b0, b1, prevz, nextz, emit);
        if (tid == 0) atomicOr(&s_words[2], 2u);           // BFINAL = 0, BTYPE = 01, as the stream's first three bits
    }
    __syncthreads();
    if (tid == 0) {
        if (!stored) s_img[8 + n - 2] = s_img[8 + n - 1] = 0xFF;
        put_be32(s_img, (uint32_t)n);
        s_img[4] = 'I'; s_img[5] = 'D'; s_img[6] = 'A'; s_img[7] = 'T';
    }
    __syncthreads();
    // CRC-32 over type and data: lanes run the table over sub-ranges, a register r followed by m more bytes is r x^(8 m) mod P
    {
        const int m = n + 4, Kc = hps::ceil_div(m, PNG_THREADS);
        const int c0 = min(m, tid * Kc), c1 = min(m, c0 + Kc);
        uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
        for (int i = c0; i < c1; ++i) c = s_crc[(c ^ s_img[4 + i]) & 0xFF] ^ (c >> 8);
        if (c != 0) atomicXor(&s_red[2], multmodp(x8n_modp((uint32_t)(m - c1)), c));
    }
    __syncthreads();
    if (tid == 0) put_be32(s_img + 8 + n, s_red[2] ^ 0xFFFFFFFFu);
    __syncthreads();
    uint8_t* slot = pic.ws + ws_meta_bytes(pic.nseg) + (int64_t)seg * ws_slot_bytes(pic.R, rb);
    for (int u = tid; u < units; u += PNG_THREADS) reinterpret_cast<uint4*>(slot)[u] = s_img4[u];
    if (tid == 0) {
        uint32_t* meta = reinterpret_cast<uint32_t*>(pic.ws);
        meta[seg] = (uint32_t)(12 + n);
        meta[pic.nseg + seg] = s_red[0] % ADLER_MOD;
        meta[2 * pic.nseg + seg] = s_red[1] % ADLER_MOD;
    }
}

__global__ void __launch_bounds__(PNG_THREADS) png_assemble_kernel(const PngParams P) {
    __shared__ uint32_t s_sum[3];
    const PngPic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x;
    const int seg = blockIdx.x - pic.seg0, nseg = pic.nseg;
    const int rb = pic.W * pic.C + 1;
    const uint32_t* meta = reinterpret_cast<const uint32_t*>(pic.ws);
    if (tid < 3) s_sum[tid] = 0;
    __syncthreads();
    uint32_t before = 0;
    for (int k = tid; k < seg; k += PNG_THREADS) before += meta[k];
    if (before) atomicAdd(&s_sum[0], before);
    __syncthreads();
    const int64_t offset = PNG_PROLOGUE + (int64_t)s_sum[0];
    const int len = (int)meta[seg];

    // the chunk to its place: 16-byte stores where the destination allows, the ends byte by byte
    const uint8_t* src = pic.ws + ws_meta_bytes(nseg) + (int64_t)seg * ws_slot_bytes(pic.R, rb);
    uint8_t* dst = pic.out + offset;
    const int head = min(len, (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
    const int body = (len - head) / 16;
    if (tid < head) dst[tid] = src[tid];
    for (int u = tid; u < body; u += PNG_THREADS) {
        uint4 v;
        __builtin_memcpy(&v, src + head + 16 * u, 16);
        *reinterpret_cast<uint4*>(dst + head + 16 * u) = v;
    }
    const int done = head + 16 * body;
    if (tid < len - done) dst[done + tid] = src[done + tid];

    if (seg == 0 && tid == 0) {
        uint8_t h[PNG_PROLOGUE] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A, 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
        put_be32(h + 16, (uint32_t)pic.W);
        put_be32(h + 20, (uint32_t)pic.H);
        h[24] = 8; h[25] = pic.C == 3 ? 2 : 0; h[26] = h[27] = h[28] = 0;
        put_be32(h + 29, crc_bitwise(h + 12, 17));
        h[33] = h[34] = h[35] = 0; h[36] = 2; h[37] = 'I'; h[38] = 'D'; h[39] = 'A'; h[40] = 'T';
        h[41] = 0x78; h[42] = 0x01;                        // zlib: deflate, 32 KiB window, fastest; (0x7801 % 31 == 0)
        put_be32(h + 43, crc_bitwise(h + 37, 6));
        for (int i = 0; i < PNG_PROLOGUE; ++i) pic.out[i] = h[i];
    }
    if (seg == nseg - 1) {
        // Adler-32 of all filtered bytes from the segments' sums: a byte i of segment k with `after` bytes behind its segment adds
        // v to a and (n_k - i + after) v to b; the initial a = 1 adds the total length to b.
        const int64_t raw_total = (int64_t)pic.H * rb, seg_full = (int64_t)pic.R * rb;
        uint32_t pa = 0, pb = 0;
        for (int k = tid; k < nseg; k += PNG_THREADS) {
            const int64_t end = min(raw_total, (k + 1) * seg_full);
            const uint32_t after = (uint32_t)((raw_total - end) % ADLER_MOD);
            const uint32_t sa = meta[nseg + k], sb = meta[2 * nseg + k];
            pa = (pa + sa) % ADLER_MOD;
            pb = (uint32_t)((pb + sb + (uint64_t)sa * after) % ADLER_MOD);
        }
        atomicAdd(&s_sum[1], pa);
        atomicAdd(&s_sum[2], pb);
        __syncthreads();
        if (tid == 0) {
            const uint32_t a = (1u + s_sum[1]) % ADLER_MOD;
            const uint32_t b = (uint32_t)((raw_total % ADLER_MOD + s_sum[2]) % ADLER_MOD);
            uint8_t t[PNG_EPILOGUE] = {0, 0, 0, 6, 'I', 'D', 'A', 'T', 0x03, 0x00};         // BFINAL = 1, BTYPE = 01, end of block
            put_be32(t + 10, (b << 16) | a);
            put_be32(t + 14, crc_bitwise(t + 4, 10));
            t[18] = t[19] = t[20] = t[21] = 0; t[22] = 'I'; t[23] = 'E'; t[24] = 'N'; t[25] = 'D';
            put_be32(t + 26, crc_bitwise(t + 22, 4));
            uint8_t* end = dst + len;
            for (int i = 0; i < PNG_EPILOGUE; ++i) end[i] = t[i];
            *pic.length = offset + len + PNG_EPILOGUE;
        }
    }
}

}  // namespace

namespace hps {
int64_t png_ws_bytes(int64_t H, int64_t W, int64_t C) {
    if (H > PNG_MAX_H || W > PNG_MAX_ROW || !supported((int)H, (int)W, (int)C)) return -1;
    const int R = seg_rows((int)W, (int)C), nseg = ceil_div((int)H, R);
    return ws_meta_bytes(nseg) + nseg * ws_slot_bytes(R, 1 + (int)(W * C));
}
}  // namespace hps

extern "C" int hps_sizeof_png_encode_args(void) { return (int)sizeof(hps_png_encode_args); }

extern "C" int hps_png_segment_rows(int H, int W, int C) {
    if (!supported(H, W, C)) {
        hps::bad_arg("hps_png_segment_rows: C is 1 or 3, W C in [1, 12288], H in [1, 32768]");
        return -1;
    }
    return seg_rows(W, C);
}

// The bound.  The file is: signature 8, IHDR 25, the header chunk 12 + 2, one chunk of 12 + n_k per segment, the closing chunk
// 12 + 6, IEND 12.  A segment of S_k filtered bytes is coded with the fixed tables in ceil((3 + t + 7 + 3) / 8) + 4 bytes, t <= 9 S_k
// token bits (a literal takes at most 9 bits, and a match of L >= 3 bytes at most 18 bits <= 9 L) -- the 9 / 8 bound -- but the
// kernel takes one stored block, 5 + S_k bytes, whenever the fixed form is longer, so n_k <= S_k + 5 always (S_k <= 16 384 < 65 536:
// one stored block holds it).  The S_k sum to H (1 + W C).  Hence
//     file <= 8 + 25 + 14 + H (1 + W C) + 17 ceil(H / R) + 18 + 12.
extern "C" int64_t hps_png_bound(int H, int W, int C) {
    if (!supported(H, W, C)) {
        hps::bad_arg("hps_png_bound: C is 1 or 3, W C in [1, 12288], H in [1, 32768]");
        return -1;
    }
    const int64_t nseg = hps::ceil_div(H, seg_rows(W, C));
    return PNG_PROLOGUE + (int64_t)H * (1 + W * C) + 17 * nseg + PNG_EPILOGUE;
}

extern "C" int hps_png_encode(const hps_png_encode_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_png_encode: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_png_encode_args)) return bad_arg("hps_png_encode: struct_bytes is not sizeof(hps_png_encode_args)");
    if (a->num_images < 1 || a->num_images > HPS_PNG_MAX_IMAGES) return bad_arg("hps_png_encode: num_images in [1, HPS_PNG_MAX_IMAGES]");
    PngParams P;
    P.n = a->num_images;
    int segs = 0;
    for (int i = 0; i < HPS_PNG_MAX_IMAGES; ++i) {
        PngPic& p = P.pic[i];
        if (i >= a->num_images) {
            p = PngPic{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 1, 0, 0x7fffffff};
            continue;
        }
        const hps_png_image& im = a->image[i];
        if (!im.pixels || !im.out || !im.length || !im.workspace) return bad_arg("hps_png_encode: null pointer (a picture's pixels, out, length, workspace)");
        if (im.C != 1 && im.C != 3) return bad_arg("hps_png_encode: C is 1 (greyscale) or 3 (RGB)");
        if (im.H < 1 || im.W < 1) return bad_arg("hps_png_encode: H and W are at least 1");
        if (!supported(im.H, im.W, im.C)) return bad_arg("hps_png_encode: supported pictures have W C <= 12288 and H <= 32768");
        if (im.capacity < hps_png_bound(im.H, im.W, im.C)) return bad_arg("hps_png_encode: a picture's capacity is below hps_png_bound(H, W, C)");
        if ((reinterpret_cast<uintptr_t>(im.pixels) | reinterpret_cast<uintptr_t>(im.out) | reinterpret_cast<uintptr_t>(im.workspace)) & 15)
            return bad_arg("hps_png_encode: pixels, out and workspace must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(im.length) & 7) return bad_arg("hps_png_encode: length must be 8-byte aligned");
        p.px = im.pixels; p.ws = static_cast<uint8_t*>(im.workspace); p.out = im.out; p.length = reinterpret_cast<long long*>(im.length);
        p.H = im.H; p.W = im.W; p.C = im.C;
        p.R = seg_rows(im.W, im.C);
        p.nseg = ceil_div(im.H, p.R);
        p.seg0 = segs;
        segs += p.nseg;
    }
    png_segment_kernel<<<segs, PNG_THREADS, 0, (hipStream_t)stream>>>(P);
    if (int rc = check_launch("hps_png_encode (segments)")) return rc;
    png_assemble_kernel<<<segs, PNG_THREADS, 0, (hipStream_t)stream>>>(P);
    return check_launch("hps_png_encode (assemble)");
}
