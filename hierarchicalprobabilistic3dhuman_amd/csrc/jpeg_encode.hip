// Baseline JPEG files made on the device (no reference counterpart: the reference hands its pictures to cv2.imwrite on the host).  A
// finished (H, W, C) uint8 picture becomes the bytes of a complete file -- SOI, APP0, DQT, SOF0, DHT, SOS, the scan, EOI -- equal byte
// for byte to what libjpeg(-turbo) writes at the same quality and sampling (include/hps.h states the file; csrc/jpeg_encode.h holds the
// per-block functions, shared with the host check).  Four launches per call, whatever the number and size of the pictures.  Every
// launch has one workgroup of JPE_THREADS lanes per JPE_THREADS consecutive blocks of a picture's scan (a multiple of every MCU size,
// so a workgroup holds whole MCUs):
//   jpe_blocks_kernel   one lane per 8 x 8 block: the samples row by row (colour conversion, down-sampling, edge replication), the row
//                       pass of the DCT in registers, the column pass from LDS, quantisation into zig-zag order; a dummy block takes
//                       its source's DC from LDS.  Out: the coefficients (coalesced dword stores from LDS) and, per block, its DC value
//                       and the bit count of its AC part.
//   jpe_count_kernel    one lane per block: the DC difference to the block before it of the same component, the block's bit count;
//                       the workgroup's sum.
//   jpe_bits_kernel     the workgroup's bit offset is the sum of the sums before it.  Every lane writes its block's bits into an LDS bit
//                       buffer (atomic OR on zeroed words: the bits are disjoint, so the result is exact); two lanes also write the two
//                       blocks BEFORE the workgroup's first, which hold the at most 7 bits that share a byte with it.  The workgroup then
//                       owns every byte whose LAST bit is its own -- all complete in LDS -- stores them into the unstuffed stream (whole
//                       dwords, the ends byte by byte) and counts its FF bytes.  The last workgroup pads with 1 bits.
//   jpe_file_kernel     the workgroup's place in the file is the header, its first byte's index and the FF bytes before it: every lane
//                       copies a run of the workgroup's bytes with a 00 behind each FF.  The first workgroup writes the header, the last
//                       EOI and the length.
// No global atomics; the LDS atomics are integer OR and ADD, whose results do not depend on arrival order.  Every loop bound is a
// function of the sizes.  Nothing is written at or behind out + *length.
#include "hps_common.h"
#include "jpeg_encode.h"

namespace {

constexpr int JPE_THREADS = 192;          // blocks per workgroup: a multiple of the MCU sizes 1, 3, 4 and 6
constexpr int JPE_ROW = 66;               // int16 per block in LDS: 33 dwords, so that lanes reading one position hit 32 different banks
constexpr int JPE_LDS_WORDS = ((JPE_THREADS + 2) * JPE_MAX_BLOCK_BITS + 31 + 31) / 32 + 1;
constexpr int JPE_MAX_DIM = 8192;
static_assert(JPE_LDS_WORDS * 4 <= 48 * 1024, "the bit buffer fits the LDS");
static_assert(JPE_THREADS % 6 == 0 && JPE_THREADS % 4 == 0, "a workgroup holds whole MCUs");

__constant__ JpeTables c_tables = jpe_make_tables();

struct JpePic {
    const uint8_t* px;
    uint8_t* ws;
    uint8_t* out;
    long long* length;
    int H, W, C, quality, sampling;
    int nblk, nwg, wg0;                   // blocks, workgroups, workgroups of the pictures before this one
};
struct JpeParams {
    JpePic pic[HPS_JPEG_ENC_MAX_IMAGES];
    int n;
};

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
// a picture's workspace: coefficients (128 bytes per block), DC | AC bits << 16 per block, bits per block, bits and FF bytes per
// workgroup, the unstuffed stream
struct JpeLayout {
    int64_t info, nbits, part, ff, stream, total;
};
__host__ __device__ inline JpeLayout jpe_layout(int nblk) {
    const int nwg = (nblk + JPE_THREADS - 1) / JPE_THREADS;
    JpeLayout L;
    L.info = (int64_t)nblk * 128;
    L.nbits = L.info + align16((int64_t)nblk * 4);
    L.part = L.nbits + align16((int64_t)nblk * 4);
    L.ff = L.part + align16((int64_t)nwg * 4);
    L.stream = L.ff + align16((int64_t)nwg * 4);
    L.total = L.stream + align16(((int64_t)nblk * JPE_MAX_BLOCK_BITS + 7) / 8 + 4);
    return L;
}

inline bool supported(int H, int W, int C, int sampling) {
    return (C == 1 || (C == 3 && sampling >= 0 && sampling <= 2)) && H >= 1 && H <= JPE_MAX_DIM && W >= 1 && W <= JPE_MAX_DIM;
}

__device__ inline const JpePic& find_picture(const JpeParams& P, int block) {
    int p = 0;
    for (int i = 1; i < HPS_JPEG_ENC_MAX_IMAGES; ++i)
        if (i < P.n && block >= P.pic[i].wg0) p = i;
    return P.pic[p];
}

// exclusive sum in lane order over the workgroup; *total receives the sum over all lanes
__device__ int block_scan_excl(int v, int* s, int* total) {
    const int tid = threadIdx.x;
    s[tid] = v;
    for (int off = 1; off < JPE_THREADS; off <<= 1) {
        __syncthreads();
        const int t = tid >= off ? s[tid - off] : 0;
        __syncthreads();
        s[tid] += t;
    }
    __syncthreads();
    const int r = tid > 0 ? s[tid - 1] : 0;
    *total = s[JPE_THREADS - 1];
    __syncthreads();
    return r;
}

// the sum of v[0 .. n) by the whole workgroup (64-bit: a picture's scan can pass 2^32 bits)
__device__ unsigned long long block_sum_before(const uint32_t* v, int n, unsigned long long* s) {
    if (threadIdx.x == 0) *s = 0;
    __syncthreads();
    unsigned long long acc = 0;
    for (int k = threadIdx.x; k < n; k += JPE_THREADS) acc += v[k];
    if (acc) atomicAdd(s, acc);
    __syncthreads();
    const unsigned long long r = *s;
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(JPE_THREADS) jpe_blocks_kernel(const JpeParams P) {
    __shared__ int16_t s_row[JPE_THREADS * JPE_ROW];       // after the row pass, natural order
    __shared__ __attribute__((aligned(4))) int16_t s_zz[JPE_THREADS * JPE_ROW];      // quantised, zig-zag order
    __shared__ uint16_t s_q[2][64];
    const JpePic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x, w = blockIdx.x - pic.wg0;
    const int first = w * JPE_THREADS, i = first + tid;
    if (tid < 128) s_q[tid >> 6][tid & 63] = (uint16_t)jpe_quant(c_tables.base[tid >> 6][tid & 63], pic.quality);
    const JpeGeometry g = jpe_geometry(pic.H, pic.W, pic.C, pic.sampling);
    const bool valid = i < pic.nblk;
    JpeBlock b = {0, 0, 0, i, -1};
    if (valid) b = jpe_block(g, i);
    const bool real = valid && b.source == i;
    const int table = b.comp ? 1 : 0;
    __syncthreads();
    int16_t* row = s_row + tid * JPE_ROW;
    int16_t* zz = s_zz + tid * JPE_ROW;
    if (real) {
#pragma unroll 1
        for (int y = 0; y < 8; ++y) {
            int r[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) r[x] = jpe_sample(pic.px, g, b.comp, 8 * b.bx + x, 8 * b.by + y) - 128;
            jpe_fdct_1d(r, 1, true);
#pragma unroll
            for (int x = 0; x < 8; ++x) row[8 * y + x] = (int16_t)r[x];      // |r| < 2^13 after the row pass
        }
#pragma unroll 1
        for (int c = 0; c < 8; ++c) {
            int col[8];
#pragma unroll
            for (int y = 0; y < 8; ++y) col[y] = row[8 * y + c];
            jpe_fdct_1d(col, 1, false);
#pragma unroll
            for (int y = 0; y < 8; ++y) zz[c_tables.zigzag[8 * y + c]] = (int16_t)jpe_quantise(col[y], s_q[table][8 * y + c]);
        }
    }
    __syncthreads();
    if (valid && !real) {                                    // a dummy: its source lies in the same MCU, so in this workgroup
        for (int k = 1; k < 64; ++k) zz[k] = 0;
        zz[0] = s_zz[(b.source - first) * JPE_ROW];
    }
    __syncthreads();
    const int nvalid = min(JPE_THREADS, pic.nblk - first);
    uint32_t* coef = reinterpret_cast<uint32_t*>(pic.ws) + (int64_t)first * 32;
    const uint32_t* lds = reinterpret_cast<const uint32_t*>(s_zz);
    for (int j = tid; j < nvalid * 32; j += JPE_THREADS) coef[j] = lds[(j >> 5) * (JPE_ROW / 2) + (j & 31)];
    if (valid) {
        const JpeLayout L = jpe_layout(pic.nblk);
        const int ac = jpe_ac_bits(c_tables, table, zz);
        reinterpret_cast<uint32_t*>(pic.ws + L.info)[i] = ((uint32_t)ac << 16) | (uint16_t)zz[0];
    }
}

__global__ void __launch_bounds__(JPE_THREADS) jpe_count_kernel(const JpeParams P) {
    __shared__ uint32_t s_sum;
    const JpePic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x, w = blockIdx.x - pic.wg0;
    const int i = w * JPE_THREADS + tid;
    const JpeLayout L = jpe_layout(pic.nblk);
    const uint32_t* info = reinterpret_cast<const uint32_t*>(pic.ws + L.info);
    if (tid == 0) s_sum = 0;
    __syncthreads();
    if (i < pic.nblk) {
        const JpeGeometry g = jpe_geometry(pic.H, pic.W, pic.C, pic.sampling);
        const JpeBlock b = jpe_block(g, i);
        const uint32_t own = info[i];
        const int dc = (int16_t)(own & 0xFFFF), before = b.pred >= 0 ? (int16_t)(info[b.pred] & 0xFFFF) : 0;
        const uint32_t nb = (own >> 16) + (uint32_t)jpe_dc_bits(c_tables, b.comp ? 1 : 0, dc - before);
        reinterpret_cast<uint32_t*>(pic.ws + L.nbits)[i] = nb;
        atomicAdd(&s_sum, nb);
    }
    __syncthreads();
    if (tid == 0) reinterpret_cast<uint32_t*>(pic.ws + L.part)[w] = s_sum;
}

struct LdsOr {
    uint32_t* words;
    __device__ void operator()(uint32_t i, uint32_t v) const { atomicOr(&words[i], v); }
};

__device__ inline void emit_block(const JpePic& pic, const JpeGeometry& g, const JpeLayout& L, int i, uint32_t pos, uint32_t* words) {
    const JpeBlock b = jpe_block(g, i);
    const uint32_t* info = reinterpret_cast<const uint32_t*>(pic.ws + L.info);
    const int dc = (int16_t)(info[i] & 0xFFFF), before = b.pred >= 0 ? (int16_t)(info[b.pred] & 0xFFFF) : 0;
    JpeWordSink<LdsOr> sink{LdsOr{words}, pos};
    jpe_block_bits(c_tables, b.comp ? 1 : 0, reinterpret_cast<const int16_t*>(pic.ws) + (int64_t)i * 64, dc - before, sink);
}

// what a workgroup owns of the unstuffed stream: the bytes whose last bit is one of its own (the last workgroup: the padded byte too)
struct JpeOwned {
    unsigned long long base, end;         // its bits
    long long j0, j1;                     // its bytes
};
__device__ inline JpeOwned owned_bytes(unsigned long long base, uint32_t bits, bool last) {
    JpeOwned o;
    o.base = base;
    o.end = base + bits;
    o.j0 = (long long)(base >> 3);
    o.j1 = (long long)(last ? (o.end + 7) >> 3 : o.end >> 3);
    return o;
}

__global__ void __launch_bounds__(JPE_THREADS) jpe_bits_kernel(const JpeParams P) {
    __shared__ uint32_t s_words[JPE_LDS_WORDS];
    __shared__ int s_scan[JPE_THREADS];
    __shared__ unsigned long long s_base;
    __shared__ uint32_t s_ff;
    const JpePic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x, w = blockIdx.x - pic.wg0;
    const int first = w * JPE_THREADS, i = first + tid;
    const JpeLayout L = jpe_layout(pic.nblk);
    const JpeGeometry g = jpe_geometry(pic.H, pic.W, pic.C, pic.sampling);
    const uint32_t* nbits = reinterpret_cast<const uint32_t*>(pic.ws + L.nbits);
    const unsigned long long base = block_sum_before(reinterpret_cast<const uint32_t*>(pic.ws + L.part), w, &s_base);
    int total = 0;
    const int off = block_scan_excl(i < pic.nblk ? (int)nbits[i] : 0, s_scan, &total);
    // the two blocks before the first (w > 0: there are JPE_THREADS >= 2 of them): at least 8 bits, all that can share a byte
    const uint32_t p1 = w > 0 ? nbits[first - 1] : 0, p2 = w > 0 ? nbits[first - 2] : 0;
    const unsigned long long origin = (base - p1 - p2) & ~31ull;           // bit 0 of the LDS buffer in the stream
    const uint32_t rel = (uint32_t)(base - origin);
    const bool last = w == pic.nwg - 1;
    const JpeOwned own = owned_bytes(base, (uint32_t)total, last);
    const int nwords = (int)((own.end - origin + 7 + 31) / 32);              // <= JPE_LDS_WORDS: 31 + (JPE_THREADS + 2) blocks + 7
    if (tid == 0) s_ff = 0;
    for (int k = tid; k < nwords; k += JPE_THREADS) s_words[k] = 0;
    __syncthreads();
    if (i < pic.nblk) emit_block(pic, g, L, i, rel + (uint32_t)off, s_words);
    if (w > 0 && tid < 2) emit_block(pic, g, L, first - 1 - tid, tid == 0 ? rel - p1 : rel - p1 - p2, s_words);
    if (last && tid == 0 && (own.end & 7)) {
        const int pad = 8 - (int)(own.end & 7);
        JpeWordSink<LdsOr> sink{LdsOr{s_words}, rel + (uint32_t)total};
        sink.put((1u << pad) - 1, pad);
    }
    __syncthreads();
    // the owned bytes to the stream: byte j is byte 3 - (j & 3) of word j >> 2; whole dwords where all four bytes are owned
    uint8_t* stream = pic.ws + L.stream;
    const long long o4 = (long long)(origin >> 5);                            // the stream dword of LDS word 0
    long long d0 = (own.j0 + 3) >> 2, d1 = own.j1 >> 2;
    if (d1 < d0) d1 = d0;
    uint32_t ff = 0;
    for (long long d = d0 + tid; d < d1; d += JPE_THREADS) {
        const uint32_t v = s_words[d - o4];
        reinterpret_cast<uint32_t*>(stream)[d] = __builtin_bswap32(v);
        ff += ((v >> 24) == 0xFF) + (((v >> 16) & 0xFF) == 0xFF) + (((v >> 8) & 0xFF) == 0xFF) + ((v & 0xFF) == 0xFF);
    }
    if (tid == 0)
        for (long long j = own.j0; j < own.j1; ++j) {
            if (j >= 4 * d0 && j < 4 * d1) { j = 4 * d1 - 1; continue; }
            const uint32_t v = (s_words[(j >> 2) - o4] >> (24 - 8 * (int)(j & 3))) & 0xFF;
            stream[j] = (uint8_t)v;
            ff += v == 0xFF;
        }
    if (ff) atomicAdd(&s_ff, ff);
    __syncthreads();
    if (tid == 0) reinterpret_cast<uint32_t*>(pic.ws + L.ff)[w] = s_ff;
}

__global__ void __launch_bounds__(JPE_THREADS) jpe_file_kernel(const JpeParams P) {
    __shared__ uint8_t s_header[JPE_MAX_HEADER];
    __shared__ int s_scan[JPE_THREADS];
    __shared__ unsigned long long s_sum;
    const JpePic& pic = find_picture(P, blockIdx.x);
    const int tid = threadIdx.x, w = blockIdx.x - pic.wg0;
    const JpeLayout L = jpe_layout(pic.nblk);
    const uint32_t* part = reinterpret_cast<const uint32_t*>(pic.ws + L.part);
    const unsigned long long base = block_sum_before(part, w, &s_sum);
    const unsigned long long ff_before = block_sum_before(reinterpret_cast<const uint32_t*>(pic.ws + L.ff), w, &s_sum);
    const bool last = w == pic.nwg - 1;
    const JpeOwned own = owned_bytes(base, part[w], last);
    const int nh = jpe_header_bytes(pic.C);
    if (w == 0) {
        if (tid == 0) jpe_header(c_tables, s_header, pic.H, pic.W, pic.C, pic.quality, pic.sampling);
        __syncthreads();
        for (int k = tid; k < nh; k += JPE_THREADS) pic.out[k] = s_header[k];
    }
    // every lane a run of the workgroup's bytes: FF bytes before it in the workgroup, then the copy with the stuffing
    const uint8_t* stream = pic.ws + L.stream;
    const int n = (int)(own.j1 - own.j0), K = hps::ceil_div(n, JPE_THREADS);
    const int b0 = min(n, tid * K), b1 = min(n, b0 + K);
    int ff = 0;
    for (int k = b0; k < b1; ++k) ff += stream[own.j0 + k] == 0xFF;
    int ff_total = 0;
    const int ff_lane = block_scan_excl(ff, s_scan, &ff_total);
    uint8_t* dst = pic.out + nh + own.j0 + (long long)ff_before;
    jpe_stuff(stream + own.j0 + b0, b1 - b0, dst + b0 + ff_lane);
    if (last && tid == 0) {
        dst[n + ff_total] = 0xFF;
        dst[n + ff_total + 1] = 0xD9;
        *pic.length = nh + own.j1 + (long long)ff_before + ff_total + 2;
    }
}

}  // namespace

namespace hps {
int64_t jpeg_enc_ws_bytes(int64_t H, int64_t W, int64_t d2) {
    const int64_t C = d2 & 255, sampling = d2 >> 8;
    if (H < 1 || H > JPE_MAX_DIM || W < 1 || W > JPE_MAX_DIM || !supported((int)H, (int)W, (int)C, (int)sampling)) return -1;
    return jpe_layout(jpe_geometry((int)H, (int)W, (int)C, (int)sampling).nblk).total;
}
}  // namespace hps

extern "C" int hps_sizeof_jpeg_encode_args(void) { return (int)sizeof(hps_jpeg_encode_args); }

// The bound (jpe_bound, csrc/jpeg_encode.h).  The file is the header (328 bytes for one component, 623 for three: constant), the scan
// and EOI (2).  A block is a DC code of at most 11 bits with at most 11 magnitude bits -- the difference of two DC values in
// [-1024, 1016] has at most 11 -- and at most 63 AC symbols, each a code of at most 16 bits with at most 10 magnitude bits (a ZRL only
// stands where coefficients are zero, and 16 zeros cost less as one ZRL than as 16 coded coefficients): at most 22 + 63 * 26 = 1660 bits.
// The scan before stuffing is the blocks (dummies included) and at most 7 padding bits, so at most ceil(1660 blocks / 8) bytes, and
// stuffing at most doubles a byte.
extern "C" int64_t hps_jpeg_encode_bound(int H, int W, int C, int sampling) {
    if (!supported(H, W, C, sampling)) {
        hps::bad_arg("hps_jpeg_encode_bound: C is 1 or 3, H and W in [1, 8192], sampling (C = 3) 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
        return -1;
    }
    return jpe_bound(H, W, C, sampling);
}

extern "C" int hps_jpeg_encode(const hps_jpeg_encode_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_jpeg_encode: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_jpeg_encode_args)) return bad_arg("hps_jpeg_encode: struct_bytes is not sizeof(hps_jpeg_encode_args)");
    if (a->num_images < 1 || a->num_images > HPS_JPEG_ENC_MAX_IMAGES) return bad_arg("hps_jpeg_encode: num_images in [1, HPS_JPEG_ENC_MAX_IMAGES]");
    JpeParams P;
    P.n = a->num_images;
    int wgs = 0;
    for (int i = 0; i < HPS_JPEG_ENC_MAX_IMAGES; ++i) {
        JpePic& p = P.pic[i];
        if (i >= a->num_images) {
            p = JpePic{nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, 0, 0, 0, 0x7fffffff};
            continue;
        }
        const hps_jpeg_enc_image& im = a->image[i];
        if (!im.pixels || !im.out || !im.length || !im.workspace) return bad_arg("hps_jpeg_encode: null pointer (a picture's pixels, out, length, workspace)");
        if (im.C != 1 && im.C != 3) return bad_arg("hps_jpeg_encode: C is 1 (greyscale) or 3 (RGB)");
        if (im.H < 1 || im.W < 1 || im.H > JPE_MAX_DIM || im.W > JPE_MAX_DIM) return bad_arg("hps_jpeg_encode: H and W in [1, 8192]");
        if (im.quality < 1 || im.quality > 100) return bad_arg("hps_jpeg_encode: quality in [1, 100]");
        if (im.C == 3 && (im.sampling < 0 || im.sampling > 2)) return bad_arg("hps_jpeg_encode: sampling is 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)");
        if (im.capacity < jpe_bound(im.H, im.W, im.C, im.sampling)) return bad_arg("hps_jpeg_encode: a picture's capacity is below hps_jpeg_encode_bound(H, W, C, sampling)");
        if ((reinterpret_cast<uintptr_t>(im.pixels) | reinterpret_cast<uintptr_t>(im.out) | reinterpret_cast<uintptr_t>(im.workspace)) & 15)
            return bad_arg("hps_jpeg_encode: pixels, out and workspace must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(im.length) & 7) return bad_arg("hps_jpeg_encode: length must be 8-byte aligned");
        p.px = im.pixels; p.ws = static_cast<uint8_t*>(im.workspace); p.out = im.out; p.length = reinterpret_cast<long long*>(im.length);
        p.H = im.H; p.W = im.W; p.C = im.C; p.quality = im.quality; p.sampling = im.C == 3 ? im.sampling : 0;
        p.nblk = jpe_geometry(p.H, p.W, p.C, p.sampling).nblk;
        p.nwg = ceil_div(p.nblk, JPE_THREADS);
        p.wg0 = wgs;
        wgs += p.nwg;
    }
    const hipStream_t s = (hipStream_t)stream;
    jpe_blocks_kernel<<<wgs, JPE_THREADS, 0, s>>>(P);
    if (int rc = check_launch("hps_jpeg_encode (blocks)")) return rc;
    jpe_count_kernel<<<wgs, JPE_THREADS, 0, s>>>(P);
    if (int rc = check_launch("hps_jpeg_encode (bit counts)")) return rc;
    jpe_bits_kernel<<<wgs, JPE_THREADS, 0, s>>>(P);
    if (int rc = check_launch("hps_jpeg_encode (bits)")) return rc;
    jpe_file_kernel<<<wgs, JPE_THREADS, 0, s>>>(P);
    return check_launch("hps_jpeg_encode (file)");
}
