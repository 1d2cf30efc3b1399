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
// No global atomics; the LDS atomics are integer OR / XOR / ADD / MAX, whose results do not depend on arrival order.  Every loop bound is
// a function of the sizes.
//
// A picture of strategy 1 (hps_png_image.strategy; include/hps.h documents the stream) goes through the same two launches; its segments
// take the filter among all five types by the same rule, count the tokens' 286 literal/length symbols in LDS, build a length-limited
// canonical code from the counts (build_code), code its lengths with the code-length alphabet (a second, 7-bit-limited code of the same
// construction) and emit ONE dynamic block where strategy 0 emits a fixed one.  Everything but the two-queue Huffman merge (one lane,
// at most 285 steps of two or three dependent LDS reads) and the Kraft repair over 15 counters runs on all lanes.  The dynamic coder's
// scratch lies in the staging buffer behind the place of the finished chunk: no LDS is added beyond three more filter sums per row.
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
    int strategy;                         // 0: fixed Huffman, Sub / Up; 1: one dynamic block per segment, all five filters
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
    __device__ void put(uint32_t v, int nb) {                                   // nb <= 21 bits, already in stream order (LSB first)
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

// ---- strategy 1: a dynamic Huffman block -------------------------------------------------------------------------------------------
constexpr int PNG_LL = 286, PNG_CL = 19;  // the literal/length and the code-length alphabets
constexpr int PNG_SYMS = 288;
constexpr int PNG_LL_BITS = 15, PNG_CL_BITS = 7;
// The dynamic coder's scratch.  It lies in the staging buffer behind the finished chunk (12 + S + 5 bytes rounded up to 16 <= 16 416),
// which is free once the rows are filtered.
constexpr int PNG_DYN_OFFSET = PNG_SEG_BYTES + 64;
struct DynScratch {
    uint32_t cnt[PNG_SYMS];               // the literal/length counts
    int sw[PNG_SYMS], iw[PNG_SYMS];       // leaf weights ascending; internal nodes' weights in the order of their creation
    uint16_t pl[PNG_SYMS], pi[PNG_SYMS];  // the parent (an internal node) of every leaf and of every internal node
    uint16_t code[PNG_SYMS];              // canonical codes, already bit-reversed for the LSB-first stream
    uint8_t len[PNG_SYMS];
    uint8_t seq[PNG_SYMS];                // the code length sequence: hlit literal/length lengths, one distance length
    uint32_t clcnt[32];
    uint16_t clcode[32];
    uint8_t cllen[32];
    uint32_t bl[16], next[16];            // codes per length; the first code of each length
    int n, hlit, hclen;
};
static_assert(PNG_DYN_OFFSET % 16 == 0 && PNG_DYN_OFFSET + (int)sizeof(DynScratch) <= PNG_RAW_LDS, "the scratch fits behind the chunk");
static_assert(12 + PNG_SEG_BYTES + 5 + 15 <= PNG_DYN_OFFSET, "the finished chunk ends before the scratch");
__constant__ uint8_t c_clorder[PNG_CL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ inline int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
__device__ inline uint32_t magnitude(int d) {                                    // |d mod 256 read as a signed byte|
    d &= 255;
    return d < 128 ? d : 256 - d;
}

// The code lengths and canonical codes of an alphabet of N <= 2 PNG_THREADS symbols from its counts (0 = unused), no length above M;
// called by the whole workgroup.  include/hps.h states the rule:
//   1. the used symbols in descending order of count, ties in ascending order of index (every lane ranks its symbols by counting: N
//      broadcast LDS reads each);
//   2. the leaves per depth of the two-queue Huffman tree on the counts, a leaf before an internal node of equal weight (lane 0 merges:
//      n - 1 steps; then every lane climbs from its leaves to the root), depths above M counted as M;
//   3. while the Kraft sum exceeds 1, one code of M bits leaves and one code of the greatest length below M that has any becomes two
//      codes one bit longer (lane 0; at most n steps over M counters);
//   4. the first symbols in the order of 1 take the shortest lengths; codes are deflate's canonical ones (every lane counts the symbols
//      of its length before it).
__device__ void build_code(const uint32_t* cnt, int N, int M, DynScratch& W, uint8_t* len, uint16_t* code) {
    const int tid = threadIdx.x;
    if (tid < 16) W.bl[tid] = 0;
    if (tid == 0) W.n = 0;
    __syncthreads();
    uint32_t c[2];
    int rank[2];
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * PNG_THREADS;
        c[h] = s < N ? cnt[s] : 0;
        rank[h] = 0;
        if (c[h]) {
            for (int t = 0; t < N; ++t) {
                const uint32_t ct = cnt[t];
                rank[h] += (ct > c[h] || (ct == c[h] && t < s)) ? 1 : 0;
            }
            atomicAdd(&W.n, 1);
        }
    }
    __syncthreads();
    const int n = W.n;
    for (int h = 0; h < 2; ++h)
        if (c[h]) W.sw[n - 1 - rank[h]] = (int)c[h];
    __syncthreads();
    if (tid == 0 && n >= 2) {
        int li = 0, ii = 0;
        for (int k = 0; k < n - 1; ++k) {
            int w2 = 0;
            for (int pick = 0; pick < 2; ++pick) {
                if (li < n && (ii >= k || W.sw[li] <= W.iw[ii])) { w2 += W.sw[li]; W.pl[li++] = (uint16_t)k; }
                else { w2 += W.iw[ii]; W.pi[ii++] = (uint16_t)k; }
            }
            W.iw[k] = w2;
        }
    }
    __syncthreads();
    for (int h = 0; h < 2; ++h)
        if (c[h]) {
            int d = 1;
            if (n >= 2) {
                int k = W.pl[n - 1 - rank[h]];
                for (int step = 0; step < n && k != n - 2; ++step) { k = W.pi[k]; ++d; }
            }
            atomicAdd(&W.bl[min(d, M)], 1u);
        }
    __syncthreads();
    if (tid == 0) {
        uint32_t total = 0;
        for (int d = 1; d <= M; ++d) total += W.bl[d] << (M - d);
        for (int it = 0; it < N && total > (1u << M); ++it) {
            --W.bl[M];
            for (int i = M - 1; i >= 1; --i)
                if (W.bl[i]) { --W.bl[i]; W.bl[i + 1] += 2; break; }
            --total;
        }
        uint32_t first = 0;
        for (int d = 1; d <= M; ++d) W.next[d] = first = (first + W.bl[d - 1]) << 1;
    }
    __syncthreads();
    for (int h = 0; h < 2; ++h) {
        const int s = tid + h * PNG_THREADS;
        if (s >= N) continue;
        int L = 0;
        if (c[h]) {
            int cum = 0;
            for (int d = 1; d <= M; ++d) {
                cum += (int)W.bl[d];
                if (rank[h] < cum) { L = d; break; }
            }
        }
        len[s] = (uint8_t)L;
    }
    __syncthreads();
    for (int h = 0; h < 2; ++h)
        if (c[h]) {
            const int s = tid + h * PNG_THREADS, L = len[s];
            uint32_t k = W.next[L];
            for (int t = 0; t < s; ++t) k += len[t] == L ? 1 : 0;
            code[s] = (uint16_t)(__brev(k) >> (32 - L));
        }
    __syncthreads();
}

// One position of the code length sequence as a code-length symbol: position k of a maximal run of r equal values v.  A run of zeros is
// cut into pieces of 138 from its start: 11 .. 138 is symbol 18, 3 .. 10 symbol 17 (emitted by the piece's first position), 1 or 2
// stay symbols 0.  A run of a length v > 0 is v once, then pieces of 6: 3 .. 6 is symbol 16, 1 or 2 stay symbols v.  sym < 0: no symbol.
__device__ inline void cl_token(int v, int k, int r, int& sym, int& eb, int& ext) {
    sym = -1; eb = 0; ext = 0;
    if (v != 0 && k == 0) { sym = v; return; }
    const int cut = v ? 6 : 138;
    if (v) { --k; --r; }
    const int q = k / cut, off = k - q * cut, piece = min(cut, r - q * cut);
    if (piece < 3) sym = v;
    else if (off == 0) {
        if (v) { sym = 16; eb = 2; ext = piece - 3; }
        else if (piece >= 11) { sym = 18; eb = 7; ext = piece - 11; }
        else { sym = 17; eb = 3; ext = piece - 3; }
    }
}

struct HistSink {                          // the fixed code's bits and the symbols' counts in one walk
    uint32_t* cnt;
    int bits = 0;
    __device__ void literal(uint32_t v) { bits += literal_bits(v); atomicAdd(&cnt[v], 1u); }
    __device__ void match(int L) {
        int sym, eb, extra;
        length_symbol(L, sym, eb, extra);
        bits += match_bits(L);
        atomicAdd(&cnt[sym], 1u);
    }
};
struct DynCountSink {
    const uint8_t* len;
    int bits = 0;
    __device__ void literal(uint32_t v) { bits += len[v]; }
    __device__ void match(int L) {
        int sym, eb, extra;
        length_symbol(L, sym, eb, extra);
        bits += len[sym] + eb + 1;                                               // + the one-bit code of distance 1
    }
};
struct DynEmitSink {
    EmitSink out;
    const uint8_t* len;
    const uint16_t* code;
    __device__ void literal(uint32_t v) { out.put(code[v], len[v]); }
    __device__ void match(int L) {
        int sym, eb, extra;
        length_symbol(L, sym, eb, extra);
        out.put(code[sym] | ((uint32_t)extra << len[sym]), len[sym] + eb + 1);   // at most 15 + 5 + 1 bits; distance 1 is the bit 0
    }
};

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
    __shared__ uint32_t s_rowsum[PNG_MAX_SEG_ROWS][5];     // sum of |residual| per row and filter type
    __shared__ uint8_t s_rowtype[PNG_MAX_SEG_ROWS];
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
    if (tid < PNG_MAX_SEG_ROWS)
        for (int f = 0; f < 5; ++f) s_rowsum[tid][f] = 0;
    if (tid < 3) s_red[tid] = 0;
    __syncthreads();

    const bool dynamic = pic.strategy == 1;
    const int K = hps::ceil_div(S, PNG_THREADS);
    const int b0 = min(S, tid * K), b1 = min(S, b0 + K);
    const uint8_t* raw = s_img - a0;                       // raw[g] = byte g of the picture

    // the filter of every row: sums of |residual| per type, residuals read as signed bytes (strategy 0: Sub and Up only).  Paeth's
    // upper-left byte is 0 for x < C and on the picture's first row; it lies in the staged row above otherwise.
    {
        int r = b0 / rb, c = b0 - r * rb;
        uint32_t acc[5] = {0, 0, 0, 0, 0};
        for (int i = b0; i < b1; ++i) {
            if (c > 0) {
                const int x = c - 1, g = (row0 + r) * WC + x;
                const bool top = row0 + r == 0;
                const int cur = raw[g], left = x >= C ? raw[g - C] : 0, up = top ? 0 : raw[g - WC];
                acc[1] += magnitude(cur - left);
                acc[2] += magnitude(cur - up);
                if (dynamic) {
                    const int ul = (x >= C && !top) ? raw[g - WC - C] : 0;
                    acc[0] += magnitude(cur);
                    acc[3] += magnitude(cur - ((left + up) >> 1));
                    acc[4] += magnitude(cur - paeth(left, up, ul));
                }
            }
            if (++c == rb || i + 1 == b1) {
                atomicAdd(&s_rowsum[r][1], acc[1]);
                atomicAdd(&s_rowsum[r][2], acc[2]);
                if (dynamic) {
                    atomicAdd(&s_rowsum[r][0], acc[0]);
                    atomicAdd(&s_rowsum[r][3], acc[3]);
                    atomicAdd(&s_rowsum[r][4], acc[4]);
                }
                for (int f = 0; f < 5; ++f) acc[f] = 0;
                if (c == rb) { c = 0; ++r; }
            }
        }
    }
    __syncthreads();
    if (tid < rows) {
        int type = s_rowsum[tid][1] < s_rowsum[tid][2] ? 1 : 2;              // strategy 0: Sub only where strictly smaller than Up
        if (dynamic) {                                                          // strategy 1: the smallest sum, ties to the lowest type
            type = 0;
            for (int f = 1; f < 5; ++f)
                if (s_rowsum[tid][f] < s_rowsum[tid][type]) type = f;
        }
        s_rowtype[tid] = (uint8_t)type;
    }
    __syncthreads();
    // the filtered bytes and their Adler-32 sums: a = sum v, b = sum (S - i) v
    {
        int r = b0 / rb, c = b0 - r * rb;
        uint32_t sa = 0, sb = 0;
        for (int i = b0; i < b1; ++i) {
            const int type = s_rowtype[r];
            uint32_t v;
            if (c == 0) v = (uint32_t)type;
            else {
                const int x = c - 1, g = (row0 + r) * WC + x;
                const bool top = row0 + r == 0;
                const int cur = raw[g], left = x >= C ? raw[g - C] : 0, up = top ? 0 : raw[g - WC];
                int ref = type == 1 ? left : up;
                if (type == 0) ref = 0;
                else if (type == 3) ref = (left + up) >> 1;
                else if (type == 4) ref = paeth(left, up, (x >= C && !top) ? raw[g - WC - C] : 0);
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
    DynScratch& W = *reinterpret_cast<DynScratch*>(s_img + PNG_DYN_OFFSET);   // the raw rows are no longer needed
    int lane_fixed_bits;
    if (dynamic) {
        for (int i = tid; i < PNG_SYMS; i += PNG_THREADS) W.cnt[i] = 0;
        if (tid < 32) W.clcnt[tid] = 0;
        if (tid == 0) W.hlit = 257;
        __syncthreads();
        HistSink hist{W.cnt};
        walk_tokens(s_filt, b0, b1, prevz, nextz, hist);
        if (tid == 0) atomicAdd(&W.cnt[256], 1u);                               // the end-of-block symbol
        lane_fixed_bits = hist.bits;
    } else {
        CountSink count;
        walk_tokens(s_filt, b0, b1, prevz, nextz, count);
        lane_fixed_bits = count.bits;
    }
    int token_bits = 0;
    const int pos = block_scan_excl<OpAdd>(lane_fixed_bits, 0, s_scan, false, &token_bits);

    // fixed block: 3 header bits, the tokens, end of block (7), an empty stored block (3 bits, pad, 00 00 FF FF); or one stored block
    const int nfixed = (3 + token_bits + 7 + 3 + 7) / 8 + 4;
    int n = nfixed;

    // strategy 1, the dynamic block: 17 header bits, 3 hclen bits, the code length symbols, the tokens, end of block, the same close
    bool use_dynamic = false;
    int hlit = 0, hclen = 0, hdr_bits = 0, dyn_bits = 0, dpos = 0, clpos = 0;
    int clsym[2] = {-1, -1}, cleb[2] = {0, 0}, clext[2] = {0, 0};
    if (dynamic) {
        build_code(W.cnt, PNG_LL, PNG_LL_BITS, W, W.len, W.code);
        for (int s = 257 + tid; s < PNG_LL; s += PNG_THREADS)
            if (W.len[s]) atomicMax(&W.hlit, s + 1);
        __syncthreads();
        hlit = W.hlit;
        const int nseq = hlit + 1;                                              // and the one distance code: length 1 for symbol 0
        for (int i = tid; i < nseq; i += PNG_THREADS) W.seq[i] = i < hlit ? W.len[i] : 1;
        __syncthreads();
        // two positions of the sequence per lane; the runs of equal values they lie in, from scans over the run starts
        const int i0 = 2 * tid, i1 = i0 + 1;
        const bool in0 = i0 < nseq, in1 = i1 < nseq;
        const int v0 = in0 ? W.seq[i0] : -1, v1 = in1 ? W.seq[i1] : -1;
        const bool bd0 = in0 && (i0 == 0 || v0 != W.seq[i0 - 1]), bd1 = in1 && v1 != v0;
        const int prevb = block_scan_excl<OpMax>(bd1 ? i1 : (bd0 ? i0 : -1), -1, s_scan, false, nullptr);
        const int nextb = block_scan_excl<OpMin>(bd0 ? i0 : (bd1 ? i1 : nseq), nseq, s_scan, true, nullptr);
        const int st0 = bd0 ? i0 : prevb, st1 = bd1 ? i1 : st0;
        if (in0) cl_token(v0, i0 - st0, (bd1 ? i1 : nextb) - st0, clsym[0], cleb[0], clext[0]);
        if (in1) cl_token(v1, i1 - st1, nextb - st1, clsym[1], cleb[1], clext[1]);
        for (int h = 0; h < 2; ++h)
            if (clsym[h] >= 0) atomicAdd(&W.clcnt[clsym[h]], 1u);
        __syncthreads();
        build_code(W.clcnt, PNG_CL, PNG_CL_BITS, W, W.cllen, W.clcode);
        if (tid == 0) {
            int h = 4;
            for (int k = PNG_CL - 1; k >= 4; --k)
                if (W.cllen[c_clorder[k]]) { h = k + 1; break; }
            W.hclen = h;
        }
        __syncthreads();
        hclen = W.hclen;
        int clbits = 0, cl_total = 0;
        for (int h = 0; h < 2; ++h)
            if (clsym[h] >= 0) clbits += W.cllen[clsym[h]] + cleb[h];
        clpos = block_scan_excl<OpAdd>(clbits, 0, s_scan, false, &cl_total);
        hdr_bits = 17 + 3 * hclen + cl_total;
        DynCountSink dcount{W.len};
        walk_tokens(s_filt, b0, b1, prevz, nextz, dcount);
        dpos = block_scan_excl<OpAdd>(dcount.bits, 0, s_scan, false, &dyn_bits);
        const int ndyn = (hdr_bits + dyn_bits + W.len[256] + 3 + 7) / 8 + 4;
        if (ndyn <= nfixed) { use_dynamic = true; n = ndyn; }                   // on a tie the dynamic block
    }
    const bool stored = n > S + 5;
    if (stored) { n = S + 5; use_dynamic = false; }
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
    } else if (use_dynamic) {
        if (tid == 0) {
            // BFINAL = 0, BTYPE = 10, HLIT - 257 (5 bits), HDIST - 1 = 0 (5), HCLEN - 4 (4); the code-length code's lengths in deflate's order
            EmitSink head{s_words, 64u};
            head.put(4u | ((uint32_t)(hlit - 257) << 3) | ((uint32_t)(hclen - 4) << 13), 17);
            for (int k = 0; k < hclen; ++k) head.put(W.cllen[c_clorder[k]], 3);
            EmitSink eob{s_words, (uint32_t)(64 + hdr_bits + dyn_bits)};
            eob.put(W.code[256], W.len[256]);
        }
        EmitSink lengths{s_words, (uint32_t)(64 + 17 + 3 * hclen + clpos)};
        for (int h = 0; h < 2; ++h)
            if (clsym[h] >= 0) {
                const int L = W.cllen[clsym[h]];
                lengths.put(W.clcode[clsym[h]] | ((uint32_t)clext[h] << L), L + cleb[h]);
            }
        DynEmitSink emit{EmitSink{s_words, (uint32_t)(64 + hdr_bits + dpos)}, W.len, W.code};
        walk_tokens(s_filt, b0, b1, prevz, nextz, emit);
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
// one stored block holds it), and strategy 1 takes its dynamic block only where that is no longer than the fixed form, so the same
// holds for it.  The S_k sum to H (1 + W C).  Hence
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
            p = PngPic{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 1, 0, 0x7fffffff, 0};
            continue;
        }
        const hps_png_image& im = a->image[i];
        if (!im.pixels || !im.out || !im.length || !im.workspace) return bad_arg("hps_png_encode: null pointer (a picture's pixels, out, length, workspace)");
        if (im.C != 1 && im.C != 3) return bad_arg("hps_png_encode: C is 1 (greyscale) or 3 (RGB)");
        if (im.H < 1 || im.W < 1) return bad_arg("hps_png_encode: H and W are at least 1");
        if (im.strategy != 0 && im.strategy != 1) return bad_arg("hps_png_encode: strategy is 0 (fixed Huffman code) or 1 (dynamic Huffman code)");
        if (!supported(im.H, im.W, im.C)) return bad_arg("hps_png_encode: supported pictures have W C <= 12288 and H <= 32768");
        if (im.capacity < hps_png_bound(im.H, im.W, im.C)) return bad_arg("hps_png_encode: a picture's capacity is below hps_png_bound(H, W, C)");
        if ((reinterpret_cast<uintptr_t>(im.pixels) | reinterpret_cast<uintptr_t>(im.out) | reinterpret_cast<uintptr_t>(im.workspace)) & 15)
            return bad_arg("hps_png_encode: pixels, out and workspace must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(im.length) & 7) return bad_arg("hps_png_encode: length must be 8-byte aligned");
        p.px = im.pixels; p.ws = static_cast<uint8_t*>(im.workspace); p.out = im.out; p.length = reinterpret_cast<long long*>(im.length);
        p.H = im.H; p.W = im.W; p.C = im.C; p.strategy = im.strategy;
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
