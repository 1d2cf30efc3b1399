// hps_jpeg_parse / hps_jpeg_decode (include/hps.h): baseline JPEG files to PIL's pixels on the device.  Five launches per call:
//   jpeg_unstuff_kernel   one workgroup per file removes FF 00 and RSTn and records the interval starts; the others zero the coefficients
//   jpeg_entropy_kernel   one workgroup per file: Huffman tables into LDS, the self-synchronising decode, its prefix sum, the write pass
//   jpeg_dc_kernel        one workgroup per (file, component): DC differences -> values, segmented by restart interval
//   jpeg_idct_kernel      eight lanes per block: dequantise, islow IDCT -> component planes
//   jpeg_colour_kernel    one lane per pixel: fancy upsampling, YCbCr -> RGB, the status word
// The bit reader, the symbol decode and the block step are csrc/jpeg_decode.h, shared with the host check.
#include "hps_common.h"
#include "jpeg_decode.h"

namespace hps {
namespace {

constexpr int JT = 1024;                       // lanes of the unstuff and entropy workgroups
constexpr int J_MIN_SUBSEQ = 128, J_MAX_SUBSEQ = 4096, J_DEFAULT_SUBSEQ = 512;
constexpr int J_ZERO_BLOCKS = 32;              // workgroups per file that zero its coefficients
constexpr uint32_t J_FRESH = 0xffffffffu;
__constant__ uint8_t g_natural[64] = JPG_NATURAL_ORDER;

// one file by value in the kernels' arguments (48 bytes; 64 of them stay below the 4 KiB argument limit)
struct JImg {
    const uint8_t* data;
    const hps_jpeg_header* hdr;                // DEVICE copy: tables only
    uint8_t* out;
    uint8_t* ws;
    uint16_t width, height, ri, shape;         // shape: ncomp | hs << 4 | vs << 8 | out channels << 12
    uint32_t scan_offset, scan_length;
};
struct JBatch {
    int n, subseq_bits;
    int32_t* status;
    int32_t* rounds;
    JImg img[HPS_FRONTEND_MAX_IMAGES];
};
static_assert(sizeof(JBatch) <= 3200, "kernel arguments");

// a file's workspace (byte offsets, all multiples of 16)
struct JLayout {
    int64_t part, stream, istart, sub_base, sub_start, sub_end, sub_int, sub_blk0, rec[2], coefs, plane[3], total;
    uint32_t stream_words, cap_sub;
    int plane_w[3], plane_h[3];
};

__host__ __device__ inline JLayout jpeg_layout(uint32_t scan_length, const JpgGeometry& g, int ncomp, int hs, int vs) {
    JLayout L;
    int64_t o = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = o;
        o += (bytes + 15) / 16 * 16;
        return at;
    };
    L.part = take(16);
    L.stream_words = (scan_length + 3) / 4 + 4;
    L.stream = take((int64_t)L.stream_words * 4);
    L.cap_sub = (uint32_t)(((int64_t)scan_length * 8) / J_MIN_SUBSEQ + g.num_intervals + 1);
    L.istart = take(((int64_t)g.num_intervals + 1) * 4);
    L.sub_base = take(((int64_t)g.num_intervals + 1) * 4);
    L.sub_start = take((int64_t)L.cap_sub * 4);
    L.sub_end = take((int64_t)L.cap_sub * 4);
    L.sub_int = take((int64_t)L.cap_sub * 4);
    L.sub_blk0 = take((int64_t)L.cap_sub * 4);
    L.rec[0] = take((int64_t)L.cap_sub * 16);
    L.rec[1] = take((int64_t)L.cap_sub * 16);
    L.coefs = take((int64_t)g.num_blocks * 128);
    for (int c = 0; c < 3; ++c) {
        L.plane_w[c] = c < ncomp ? g.mcus_x * 8 * (c == 0 && ncomp == 3 ? hs : 1) : 0;
        L.plane_h[c] = c < ncomp ? g.mcus_y * 8 * (c == 0 && ncomp == 3 ? vs : 1) : 0;
        L.plane[c] = take((int64_t)L.plane_w[c] * L.plane_h[c]);
    }
    L.total = o;
    return L;
}

struct JView {                                  // what a kernel derives from its JImg
    int width, height, ncomp, hs, vs, outc;
    JpgGeometry g;
    JLayout L;
};
__device__ inline JView jpeg_view(const JImg& im) {
    JView v;
    v.width = im.width;
    v.height = im.height;
    v.ncomp = im.shape & 15;
    v.hs = (im.shape >> 4) & 15;
    v.vs = (im.shape >> 8) & 15;
    v.outc = (im.shape >> 12) & 15;
    v.g = jpg_geometry(v.width, v.height, v.ncomp, v.hs, v.vs, im.ri);
    v.L = jpeg_layout(im.scan_length, v.g, v.ncomp, v.hs, v.vs);
    return v;
}

// exclusive prefix sum over the JT lanes of a workgroup; *total: the sum.  wave_sums: 16 words of LDS.
__device__ inline uint32_t block_exscan(uint32_t v, uint32_t* wave_sums, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                            // the previous call's readers are done
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < JT / 64; ++w) {
        const uint32_t s = wave_sums[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// inclusive segmented sum over N lanes (Hillis-Steele in LDS): a lane whose flag is set starts a segment.  Returns the sum from the
// segment's start (or lane 0) through this lane; *seen: a flag at or before this lane.
template <int N>
__device__ inline int seg_scan(int v, int f, int* sv, int* sf, int* seen) {
    const int t = threadIdx.x;
    __syncthreads();
    sv[t] = v;
    sf[t] = f;
    __syncthreads();
#pragma unroll 1
    for (int d = 1; d < N; d <<= 1) {
        int ov = 0, of = 0;
        if (t >= d) {
            ov = sv[t - d];
            of = sf[t - d];
        }
        __syncthreads();
        if (t >= d) {
            if (!f) v += ov;
            f |= of;
            sv[t] = v;
            sf[t] = f;
        }
        __syncthreads();
    }
    *seen = f;
    return v;
}

__device__ inline bool is_rst(uint32_t c) { return c >= 0xd0u && c <= 0xd7u; }

__global__ __launch_bounds__(JT) void jpeg_unstuff_kernel(const JBatch B) {
    const JImg& im = B.img[blockIdx.y];
    const JView v = jpeg_view(im);
    if (blockIdx.x > 0) {                       // zero the coefficients (the write pass stores the non-zero ones only)
        uint4* c = reinterpret_cast<uint4*>(im.ws + v.L.coefs);
        const int64_t n16 = (int64_t)v.g.num_blocks * 8;
        for (int64_t i = (int64_t)(blockIdx.x - 1) * JT + threadIdx.x; i < n16; i += (int64_t)J_ZERO_BLOCKS * JT) c[i] = make_uint4(0, 0, 0, 0);
        return;
    }
    __shared__ uint32_t wave_sums[JT / 64];
    const uint8_t* src = im.data + im.scan_offset;
    const uint32_t len = im.scan_length, nint = (uint32_t)v.g.num_intervals;
    uint8_t* dst = im.ws + v.L.stream;
    uint32_t* istart = reinterpret_cast<uint32_t*>(im.ws + v.L.istart);
    uint32_t kept = 0, markers = 0;             // carried over the iterations, the same in every lane
    int bad = 0;
    for (uint32_t base = 0; base < len; base += JT * 16) {
        const uint32_t i0 = base + threadIdx.x * 16;
        uint32_t b[18];
#pragma unroll
        for (int j = 0; j < 18; ++j) {
            const int64_t i = (int64_t)i0 + j - 1;
            b[j] = (i >= 0 && i < (int64_t)len) ? src[i] : 0u;
        }
        uint32_t keep = 0, mark = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t prev = b[j], c = b[j + 1], next = b[j + 2];
            const bool m_end = i0 + j < len && prev == 0xffu && is_rst(c);
            const bool drop = i0 + j >= len || m_end || (c == 0u && prev == 0xffu) || (c == 0xffu && is_rst(next));
            if (!drop) keep |= 1u << j;
            if (m_end) mark |= 1u << j;
        }
        uint32_t total;
        const uint32_t ex = block_exscan((uint32_t)__popc(keep) | ((uint32_t)__popc(mark) << 16), wave_sums, &total);
        uint32_t o = kept + (ex & 0xffffu), m = markers + (ex >> 16);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((keep >> j) & 1u) dst[o++] = (uint8_t)b[j + 1];       // o <= i0 + j < len: inside the stream buffer
            if ((mark >> j) & 1u) {
                ++m;
                if ((b[j + 1] & 7u) != ((m - 1) & 7u)) bad = 1;
                if (m < nint) istart[m] = o; else bad = 1;
            }
        }
        kept += total & 0xffffu;
        markers += total >> 16;
    }
    if (threadIdx.x == 0) istart[0] = 0;
    for (uint32_t m = (markers < nint ? markers : nint - 1) + 1 + threadIdx.x; m <= nint; m += JT) istart[m] = kept;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) reinterpret_cast<int32_t*>(im.ws + v.L.part)[0] = bad ? HPS_JPEG_ST_MARKERS : 0;
}

__device__ inline uint32_t pack_state(const JpgState& st) { return st.blk | (st.k << 3) | (st.nblk << 9); }

__global__ __launch_bounds__(JT) void jpeg_entropy_kernel(const JBatch B) {
    const JImg& im = B.img[blockIdx.x];
    const JView v = jpeg_view(im);
    __shared__ JpgTable tabs[6];
    __shared__ uint32_t wave_sums[JT / 64];
    __shared__ int sv[JT], sf[JT];
    __shared__ uint8_t natural[64];
    const int tid = threadIdx.x;
    const uint32_t S = (uint32_t)B.subseq_bits, nint = (uint32_t)v.g.num_intervals;
    const uint32_t nluma = (uint32_t)v.g.nluma, bpm = (uint32_t)v.g.bpm;
    const uint32_t* istart = reinterpret_cast<const uint32_t*>(im.ws + v.L.istart);
    uint32_t* sub_base = reinterpret_cast<uint32_t*>(im.ws + v.L.sub_base);
    uint32_t* sub_start = reinterpret_cast<uint32_t*>(im.ws + v.L.sub_start);
    uint32_t* sub_end = reinterpret_cast<uint32_t*>(im.ws + v.L.sub_end);
    uint32_t* sub_int = reinterpret_cast<uint32_t*>(im.ws + v.L.sub_int);
    uint32_t* sub_blk0 = reinterpret_cast<uint32_t*>(im.ws + v.L.sub_blk0);
    uint4* rec[2] = {reinterpret_cast<uint4*>(im.ws + v.L.rec[0]), reinterpret_cast<uint4*>(im.ws + v.L.rec[1])};
    int16_t* coefs = reinterpret_cast<int16_t*>(im.ws + v.L.coefs);
    const JpgStream stream = {reinterpret_cast<const uint32_t*>(im.ws + v.L.stream), v.L.stream_words};

    // the six tables
    {
        if (tid < 64) natural[tid] = g_natural[tid];
        for (int t = 0; t < 6; ++t) {
            const hps_jpeg_huff* h = t < 3 ? &im.hdr->dc[t] : &im.hdr->ac[t - 3];
            if (tid < 256) tabs[t].vals[tid] = h->vals[tid];
            if (tid == 256 + t) jpg_table_lengths(h, &tabs[t]);
        }
        __syncthreads();
        for (int t = 0; t < 6; ++t) tabs[t].look[tid] = jpg_look_entry(&tabs[t], tid);
    }
    // subsequences per interval -> sub_base
    uint32_t n_sub = 0;
    for (uint32_t base = 0; base < nint; base += JT) {
        const uint32_t k = base + tid;
        uint32_t cnt = 0;
        if (k < nint) {
            const uint32_t a = istart[k], b = istart[k + 1];
            const uint32_t bits = b > a ? (b - a) * 8u : 0u;
            cnt = bits ? (bits + S - 1) / S : 1u;
        }
        uint32_t total;
        const uint32_t ex = block_exscan(cnt, wave_sums, &total);
        if (k < nint) sub_base[k] = n_sub + ex;
        n_sub += total;
    }
    if (n_sub > v.L.cap_sub) n_sub = v.L.cap_sub;       // cannot happen (include/hps.h: the bound holds for every subseq_bits >= 128)
    if (tid == 0) sub_base[nint] = n_sub;
    __syncthreads();
    for (uint32_t s = tid; s < n_sub; s += JT) {
        uint32_t lo = 0, hi = nint - 1;                  // the last interval whose base is <= s
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (sub_base[mid] <= s) lo = mid; else hi = mid - 1;
        }
        const uint32_t j = s - sub_base[lo], a = istart[lo], b = istart[lo + 1];
        const uint32_t iend = (b > a ? b : a) * 8u;
        uint32_t start = a * 8u + j * S;
        if (start > iend) start = iend;
        sub_start[s] = start;
        sub_end[s] = iend - start > S ? start + S : iend;
        sub_int[s] = lo | (j == 0 ? 0x80000000u : 0u);
    }
    __syncthreads();

    // the synchronisation loop.  A record: x, y the exit (bit; block | coefficient << 3 | blocks completed << 9), z, w the entry it came from
    int kout = 0, val = 0;
    for (uint32_t s = tid; s < n_sub; s += JT) {
        const uint32_t k = sub_int[s] & 0x7fffffffu, a = istart[k], b = istart[k + 1];
        const uint32_t iend = (b > a ? b : a) * 8u, stop = sub_end[s];
        JpgState st = {sub_start[s], 0, 0, 0};
        JpgReader rd;
        jpg_reader_init(&rd, stream, st.p, iend);
        while (st.p < stop) jpg_step(tabs, nluma, bpm, &rd, &st, &kout, &val);
        rec[0][s] = make_uint4(st.p, pack_state(st), J_FRESH, J_FRESH);
    }
    int cur = 0;
    uint32_t rounds = 1;
    __syncthreads();
    for (uint32_t r = 1; r < n_sub; ++r) {
        int changed = 0;
        const uint4* R = rec[cur];
        uint4* W = rec[cur ^ 1];
        for (uint32_t s = tid; s < n_sub; s += JT) {
            const uint4 old = R[s];
            const uint32_t ki = sub_int[s];
            if (ki & 0x80000000u) {
                W[s] = old;
                continue;
            }
            const uint4 prev = R[s - 1];
            if (old.z == prev.x && old.w == (prev.y & 0x1ffu)) {
                W[s] = old;
                continue;
            }
            const uint32_t k = ki, a = istart[k], b = istart[k + 1];
            const uint32_t iend = (b > a ? b : a) * 8u, stop = sub_end[s];
            JpgState st = {prev.x, prev.y & 7u, (prev.y >> 3) & 63u, 0};
            JpgReader rd;
            jpg_reader_init(&rd, stream, st.p, iend);
            while (st.p < stop) jpg_step(tabs, nluma, bpm, &rd, &st, &kout, &val);
            const uint4 neu = make_uint4(st.p, pack_state(st), prev.x, prev.y & 0x1ffu);
            W[s] = neu;
            if (neu.x != old.x || neu.y != old.y) changed = 1;
        }
        cur ^= 1;
        ++rounds;
        if (!__syncthreads_or(changed)) break;
    }
    const uint4* F = rec[cur];

    // every lane's first block: the interval's first block plus the blocks its predecessors in the interval completed
    int carry = 0;
    for (uint32_t base = 0; base < n_sub; base += JT) {
        const uint32_t s = base + tid;
        int nb = 0, first = 0;
        if (s < n_sub) {
            nb = (int)(F[s].y >> 9);
            first = (int)(sub_int[s] >> 31);
        }
        int seen;
        int inc = seg_scan<JT>(nb, first, sv, sf, &seen);
        if (!seen) inc += carry;
        if (s < n_sub) sub_blk0[s] = (uint32_t)(inc - nb);
        __syncthreads();
        if (tid == JT - 1) sv[0] = inc;
        __syncthreads();
        carry = sv[0];
    }
    __syncthreads();

    // the write pass
    int err = 0;
    const uint32_t mcus = (uint32_t)(v.g.mcus_x * v.g.mcus_y), mpi = (uint32_t)v.g.mcus_per_interval;
    for (uint32_t s = tid; s < n_sub; s += JT) {
        const uint32_t ki = sub_int[s], k = ki & 0x7fffffffu, a = istart[k], b = istart[k + 1];
        const uint32_t iend = (b > a ? b : a) * 8u, stop = sub_end[s];
        const uint32_t last_mcu = (k + 1) * mpi < mcus ? (k + 1) * mpi : mcus;
        const uint32_t blk_lo = k * mpi * bpm, blk_hi = last_mcu * bpm;       // <= num_blocks: the coefficient buffer's rows
        JpgState st = {sub_start[s], 0, 0, 0};
        if (!(ki & 0x80000000u)) {
            const uint4 prev = F[s - 1];
            st.p = prev.x;
            st.blk = prev.y & 7u;
            st.k = (prev.y >> 3) & 63u;
        }
        const uint32_t b0 = blk_lo + sub_blk0[s];
        JpgReader rd;
        jpg_reader_init(&rd, stream, st.p, iend);
        while (st.p < stop && b0 + st.nblk < blk_hi) {
            const uint32_t blk = b0 + st.nblk;
            const int fl = jpg_step(tabs, nluma, bpm, &rd, &st, &kout, &val);
            if (fl & JPG_STEP_VALUE) coefs[(size_t)blk * 64 + natural[kout & 63]] = (int16_t)val;
            if (fl & JPG_STEP_ERROR) err |= HPS_JPEG_ST_CODE;
            if (st.p > iend) err |= HPS_JPEG_ST_OVERRUN;
        }
        const bool last = s + 1 == n_sub || (sub_int[s + 1] & 0x80000000u);
        if (last && b0 + st.nblk < blk_hi) err |= HPS_JPEG_ST_SHORT;
    }
    int all = 0;
    for (int bit = HPS_JPEG_ST_CODE; bit <= HPS_JPEG_ST_SHORT; bit <<= 1)
        if (__syncthreads_or(err & bit)) all |= bit;
    if (tid == 0) {
        int32_t* part = reinterpret_cast<int32_t*>(im.ws + v.L.part);
        part[1] = all;
        part[2] = (int32_t)rounds;
    }
}

// DC differences -> values: per component, in scan order, restarting at every restart interval
__global__ __launch_bounds__(256) void jpeg_dc_kernel(const JBatch B) {
    const JImg& im = B.img[blockIdx.y];
    const JView v = jpeg_view(im);
    const int c = blockIdx.x;
    if (c >= v.ncomp) return;
    __shared__ int sv[256], sf[256];
    int16_t* coefs = reinterpret_cast<int16_t*>(im.ws + v.L.coefs);
    const int bc = c == 0 ? v.g.nluma : 1, off = c == 0 ? 0 : v.g.nluma + c - 1;
    const int mcus = v.g.mcus_x * v.g.mcus_y, E = mcus * bc, mpi = v.g.mcus_per_interval;
    int carry = 0;
    for (int base = 0; base < E; base += 1024) {
        const int e0 = base + threadIdx.x * 4;
        int d[4], f[4], blk[4], run = 0, any = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + i;
            d[i] = 0;
            f[i] = 0;
            blk[i] = -1;
            if (e < E) {
                const int m = e / bc, j = e - m * bc;
                blk[i] = m * v.g.bpm + off + j;
                f[i] = j == 0 && m % mpi == 0;
                d[i] = coefs[(size_t)blk[i] * 64];
            }
            run = f[i] ? d[i] : run + d[i];
            any |= f[i];
            d[i] = run;                                   // the sum from the lane's first element, or its last flag
        }
        int seen;
        const int inc = seg_scan<256>(run, any, sv, sf, &seen);
        __syncthreads();
        sv[threadIdx.x] = inc;
        sf[threadIdx.x] = seen;
        __syncthreads();
        int before = carry;                               // what precedes this lane's elements within their segment
        if (threadIdx.x > 0) before = sf[threadIdx.x - 1] ? sv[threadIdx.x - 1] : sv[threadIdx.x - 1] + carry;
        const int next_carry = sf[255] ? sv[255] : sv[255] + carry;
        int flagged = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            flagged |= f[i];
            if (blk[i] >= 0) coefs[(size_t)blk[i] * 64] = (int16_t)(flagged ? d[i] : d[i] + before);
        }
        carry = next_carry;
    }
}

__device__ __forceinline__ void idct_1d(const int c[8], int out[8]) {
    int z1 = (c[2] + c[6]) * 4433;
    const int t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
    const int t0 = (int)((unsigned)(c[0] + c[4]) << 13), t1 = (int)((unsigned)(c[0] - c[4]) << 13);
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a = c[7], b = c[5], d = c[3], e = c[1];
    z1 = a + e;
    int z2 = b + d, z3 = a + d, z4 = b + e;
    const int z5 = (z3 + z4) * 9633;
    a *= 2446;
    b *= 16819;
    d *= 25172;
    e *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 *= -16069;
    z4 *= -3196;
    z3 += z5;
    z4 += z5;
    a += z1 + z3;
    b += z2 + z4;
    d += z2 + z3;
    e += z1 + z4;
    out[0] = t10 + e;
    out[7] = t10 - e;
    out[1] = t11 + d;
    out[6] = t11 - d;
    out[2] = t12 + b;
    out[5] = t12 - b;
    out[3] = t13 + a;
    out[4] = t13 - a;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JBatch B) {
    const JImg& im = B.img[blockIdx.y];
    const JView v = jpeg_view(im);
    if ((int64_t)blockIdx.x * 32 >= v.g.num_blocks) return;          // uniform over the workgroup
    __shared__ int wsb[32][8][9];
    const int lb = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int blk = blockIdx.x * 32 + lb;
    const bool live = blk < v.g.num_blocks;
    int comp = 0, bx = 0, by = 0;
    if (live) {
        const int mcu = blk / v.g.bpm, r = blk - mcu * v.g.bpm;
        const int mx = mcu % v.g.mcus_x, my = mcu / v.g.mcus_x;
        if (v.ncomp == 1 || r >= v.g.nluma) {
            comp = v.ncomp == 1 ? 0 : r - v.g.nluma + 1;
            bx = mx;
            by = my;
        } else {
            bx = mx * v.hs + r % v.hs;
            by = my * v.vs + r / v.hs;
        }
        const int16_t* cf = reinterpret_cast<const int16_t*>(im.ws + v.L.coefs) + (size_t)blk * 64;
        const uint8_t* qt = im.hdr->quant[comp];
        int c[8], o[8];
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) c[r8] = (int)cf[r8 * 8 + q] * (int)qt[r8 * 8 + q];
        idct_1d(c, o);
#pragma unroll
        for (int r8 = 0; r8 < 8; ++r8) wsb[lb][r8][q] = (o[r8] + (1 << 10)) >> 11;
    }
    __syncthreads();
    if (live) {
        int c[8], o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) c[i] = wsb[lb][q][i];
        idct_1d(c, o);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int p = ((o[i] + (1 << 17)) >> 18) + 128;
            p = p < 0 ? 0 : p > 255 ? 255 : p;
            w[i >> 2] |= (uint32_t)p << (8 * (i & 3));
        }
        uint8_t* plane = im.ws + (comp == 0 ? v.L.plane[0] : comp == 1 ? v.L.plane[1] : v.L.plane[2]);
        const int pw = comp == 0 ? v.L.plane_w[0] : v.L.plane_w[1];
        *reinterpret_cast<uint2*>(plane + (size_t)(by * 8 + q) * pw + bx * 8) = make_uint2(w[0], w[1]);
    }
}

__device__ inline int clamp255(int x) { return x < 0 ? 0 : x > 255 ? 255 : x; }

// one chroma sample at output pixel (x, y): libjpeg's fancy upsampling on the component's real samples
__device__ inline int chroma_at(const uint8_t* p, int pw, int cw, int ch, int hs, int vs, int x, int y) {
    if (hs == 1) return p[(size_t)y * pw + x];
    const int i = x >> 1, il = i > 0 ? i - 1 : 0, ir = i + 1 < cw ? i + 1 : cw - 1;
    if (vs == 1) {
        const uint8_t* s = p + (size_t)y * pw;
        return (x & 1) ? (3 * s[i] + s[ir] + 2) >> 2 : (3 * s[i] + s[il] + 1) >> 2;
    }
    const int j = y >> 1, jf = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* near = p + (size_t)j * pw;
    const uint8_t* far = p + (size_t)jf * pw;
    const int t = 3 * near[i] + far[i];
    return (x & 1) ? (3 * t + 3 * near[ir] + far[ir] + 7) >> 4 : (3 * t + 3 * near[il] + far[il] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const JBatch B) {
    const JImg& im = B.img[blockIdx.y];
    const JView v = jpeg_view(im);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int32_t* part = reinterpret_cast<const int32_t*>(im.ws + v.L.part);
        B.status[blockIdx.y] = part[0] | part[1];
        if (B.rounds) B.rounds[blockIdx.y] = part[2];
    }
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)v.width * v.height) return;
    const int y = (int)(pix / v.width), x = (int)(pix - (int64_t)y * v.width);
    const int Y = im.ws[v.L.plane[0] + (size_t)y * v.L.plane_w[0] + x];
    uint8_t* o = im.out + pix * v.outc;
    if (v.ncomp == 1) {
        o[0] = (uint8_t)Y;
        if (v.outc == 3) {
            o[1] = (uint8_t)Y;
            o[2] = (uint8_t)Y;
        }
        return;
    }
    const int cw = (v.width + v.hs - 1) / v.hs, ch = (v.height + v.vs - 1) / v.vs;
    const int cb = chroma_at(im.ws + v.L.plane[1], v.L.plane_w[1], cw, ch, v.hs, v.vs, x, y) - 128;
    const int cr = chroma_at(im.ws + v.L.plane[2], v.L.plane_w[2], cw, ch, v.hs, v.vs, x, y) - 128;
    o[0] = (uint8_t)clamp255(Y + ((91881 * cr + 32768) >> 16));
    o[1] = (uint8_t)clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    o[2] = (uint8_t)clamp255(Y + ((116130 * cb + 32768) >> 16));
}

bool shape_ok(int ncomp, int hs, int vs) {
    if (ncomp == 1) return hs == 1 && vs == 1;
    return ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}

}  // namespace

int64_t jpeg_ws_bytes(int64_t scan_length, int64_t d1, int64_t d2) {
    const int64_t width = d1 & 0xffffffffll, height = d1 >> 32;
    const int64_t ncomp = d2 & 0xff, hs = (d2 >> 8) & 0xff, vs = (d2 >> 16) & 0xff, ri = d2 >> 32;
    if (scan_length > HPS_JPEG_MAX_SCAN_BYTES || width < 1 || height < 1 || width > HPS_JPEG_MAX_DIM || height > HPS_JPEG_MAX_DIM || ri > 65535 ||
        !shape_ok((int)ncomp, (int)hs, (int)vs))
        return -1;
    const JpgGeometry g = jpg_geometry((int)width, (int)height, (int)ncomp, (int)hs, (int)vs, (int)ri);
    return jpeg_layout((uint32_t)scan_length, g, (int)ncomp, (int)hs, (int)vs).total;
}

}  // namespace hps

extern "C" int hps_sizeof_jpeg_header(void) { return (int)sizeof(hps_jpeg_header); }
extern "C" int hps_sizeof_jpeg_decode_args(void) { return (int)sizeof(hps_jpeg_decode_args); }

extern "C" int hps_jpeg_parse(const uint8_t* data, int64_t length, hps_jpeg_header* header) {
    if (!data || !header || length < 0) return hps::bad_arg("hps_jpeg_parse: null pointer or negative length");
    char msg[400];
    msg[0] = 0;
    const int rc = jpg_parse(data, length, header, msg, sizeof(msg));
    if (rc == 0) return HPS_OK;
    if (rc > 0) {
        hps::set_error("hps_jpeg_parse: not for the device: %s", msg);
        return HPS_JPEG_NOT_FOR_DEVICE;
    }
    hps::set_error("hps_jpeg_parse: malformed file: %s", msg);
    return HPS_E_BADARG;
}

extern "C" int hps_jpeg_decode(const hps_jpeg_decode_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_jpeg_decode: null pointer");
    if (a->struct_bytes != (int)sizeof(hps_jpeg_decode_args)) {
        set_error("bad argument: hps_jpeg_decode: struct_bytes %d != sizeof(hps_jpeg_decode_args) %d", a->struct_bytes, (int)sizeof(hps_jpeg_decode_args));
        return HPS_E_BADARG;
    }
    if (a->num_images < 1 || a->num_images > HPS_FRONTEND_MAX_IMAGES) return bad_arg("hps_jpeg_decode: num_images outside [1, HPS_FRONTEND_MAX_IMAGES]");
    if (!a->status) return bad_arg("hps_jpeg_decode: null status");
    if (a->mode != HPS_JPEG_RGB && a->mode != HPS_JPEG_NATIVE && a->mode != HPS_JPEG_GREY) return bad_arg("hps_jpeg_decode: mode");
    int S = a->subseq_bits;
    if (S == 0) S = J_DEFAULT_SUBSEQ;
    if (S < J_MIN_SUBSEQ || S > J_MAX_SUBSEQ || (S & (S - 1))) return bad_arg("hps_jpeg_decode: subseq_bits is 0 or a power of two in [128, 4096]");
    JBatch B;
    memset(&B, 0, sizeof(B));
    B.n = a->num_images;
    B.subseq_bits = S;
    B.status = a->status;
    B.rounds = a->rounds;
    int max_blocks = 0;
    int64_t max_pixels = 0;
    for (int i = 0; i < a->num_images; ++i) {
        const hps_jpeg_image& im = a->image[i];
        const hps_jpeg_header* h = im.header;
        if (!im.data || !h || !im.header_dev || !im.out || !im.workspace) return bad_arg("hps_jpeg_decode: null pointer in an image");
        if (h->struct_bytes != (int)sizeof(hps_jpeg_header)) return bad_arg("hps_jpeg_decode: a header's struct_bytes");
        if (((uintptr_t)im.workspace & 15) || ((uintptr_t)im.header_dev & 3)) return bad_arg("hps_jpeg_decode: workspace 16-byte, header_dev 4-byte aligned");
        if (h->width < 1 || h->height < 1 || h->width > HPS_JPEG_MAX_DIM || h->height > HPS_JPEG_MAX_DIM || !shape_ok(h->ncomp, h->hs, h->vs) ||
            h->restart_interval < 0 || h->restart_interval > 65535 || h->scan_offset < 0 || h->scan_length < 0 || h->scan_length > HPS_JPEG_MAX_SCAN_BYTES || h->file_bytes < 0 ||
            h->file_bytes >= (1 << 28) || (int64_t)h->scan_offset + h->scan_length > h->file_bytes)
            return bad_arg("hps_jpeg_decode: a header outside the device profile (hps_jpeg_parse writes valid ones)");
        const JpgGeometry g = jpg_geometry(h->width, h->height, h->ncomp, h->hs, h->vs, h->restart_interval);
        if (g.num_blocks != h->num_blocks || g.num_intervals != h->num_intervals) return bad_arg("hps_jpeg_decode: a header's num_blocks / num_intervals");
        if (a->mode == HPS_JPEG_GREY && h->ncomp != 1) {
            set_error("hps_jpeg_decode: HPS_JPEG_GREY of a three-component file (decode it on the host)");
            return HPS_E_UNSUPPORTED;
        }
        const int outc = a->mode == HPS_JPEG_RGB ? 3 : h->ncomp;
        JImg& d = B.img[i];
        d.data = im.data;
        d.hdr = im.header_dev;
        d.out = im.out;
        d.ws = (uint8_t*)im.workspace;
        d.width = (uint16_t)h->width;
        d.height = (uint16_t)h->height;
        d.ri = (uint16_t)h->restart_interval;
        d.shape = (uint16_t)(h->ncomp | (h->hs << 4) | (h->vs << 8) | (outc << 12));
        d.scan_offset = (uint32_t)h->scan_offset;
        d.scan_length = (uint32_t)h->scan_length;
        max_blocks = g.num_blocks > max_blocks ? g.num_blocks : max_blocks;
        const int64_t px = (int64_t)h->width * h->height;
        max_pixels = px > max_pixels ? px : max_pixels;
    }
    hipStream_t s = (hipStream_t)stream;
    const unsigned n = (unsigned)a->num_images;
    hipLaunchKernelGGL(jpeg_unstuff_kernel, dim3(1 + J_ZERO_BLOCKS, n), dim3(JT), 0, s, B);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(n), dim3(JT), 0, s, B);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(3, n), dim3(256), 0, s, B);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 31) / 32), n), dim3(256), 0, s, B);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((max_pixels + 255) / 256), n), dim3(256), 0, s, B);
    return check_launch("hps_jpeg_decode");
}
