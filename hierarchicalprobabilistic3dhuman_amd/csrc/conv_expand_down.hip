// Bottleneck entry block (models/resnet.py:102-122 with the down-sample branch built at :184-188): the expand convolution conv3 (1x1 / 1)
// + bn3, the block's down-sample (1x1 / s) + BatchNorm on the block's input, their sum and the ReLU in ONE launch
// (hps_bottleneck_expand_down).  The identity bn_d(conv_d(x)) has the output geometry and the Cout of conv3 and its only reader is
// conv3's epilogue, so a workgroup computes its own tile of it first -- the K loop of csrc/conv_pad.hip over the Cin channels of x --
// finishes it (scale, shift, + 0, rounded as the separate launch stores it) into registers in the epilogue's pixel-row layout, runs
// the K loop again over the Cmid channels of t, and adds the held tile where hps_conv2d_bn_act_pad reads its residual frame.  The
// frame of the identity is never written or read.  Both loops walk their chunks in hps_conv2d_bn_act_pad's order with the same
// MFMA sequence per chunk, and the epilogue expressions are the same, so every output has the bits of the two launches
//     hps_conv2d_bn_act_pad(x, w_d, ..., stride, relu = 0) -> d;   hps_conv2d_bn_act_pad(t, w_3, ..., residual = d, relu = 1).
// This file instantiates nothing of conv_pad.hip: the existing launches keep their code.
#include "hps_common.h"

namespace hps {
namespace expand {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PBK = 32;   // K-chunk (floats), as in conv_pad.hip

// n / d for n < 2^32 with magic = floor(2^32 / d) (0xffffffff for d = 1): the estimate is at most one short
__device__ __forceinline__ unsigned fastdiv(unsigned n, unsigned d, unsigned magic) {
    unsigned q = __umulhi(n, magic);
    if (n - q * d >= d) ++q;
    return q;
}
static unsigned div_magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ull / d); }

// one 1-KiB LDS-DMA piece: lane l fetches 16 bytes at sbase + voff and they land at lds_addr + 16 l (conv_pad.hip)
__device__ __forceinline__ void lds_dma16_sv(unsigned voff, const float* sbase, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_addr)
                 : "memory");
}

// one halo-padded NHWC input frame read by 1x1 windows: output pixel (b, ho, wo) reads pixel (ho * stride + off, wo * stride + off)
struct Frame {
    int img_pitch, row_pitch, pix_pitch;   // floats
    int stride, off;
};
struct Geom {
    Frame t, x;                            // the expand convolution's input (stride 1) and the block's input (stride s)
    int Ho, Wo, Mtot, Cout, opad, tiles_m;
    unsigned magic_howo, magic_wo;
};

// offset (floats) of output pixel m, channel 0, in the output frame
__device__ __forceinline__ unsigned out_pixel_offset(unsigned m, const Geom& g) {
    const unsigned howo = (unsigned)(g.Ho * g.Wo);
    const unsigned b = fastdiv(m, howo, g.magic_howo), rem = m - b * howo;
    const unsigned ho = fastdiv(rem, (unsigned)g.Wo, g.magic_wo), wo = rem - ho * g.Wo;
    return ((b * (g.Ho + 2 * g.opad) + ho + g.opad) * (g.Wo + 2 * g.opad) + wo + g.opad) * (unsigned)g.Cout;
}

// acc += A (BM pixels x K) * B (BN filters x K)^T over ``chunks`` chunks of 32: conv_pad_kernel's K loop for a 1x1 window (one tap: both
// sources advance by one chunk), the same stages, DMA spreading, fragment order and MFMA sequence.
template <int BM, int BN, int WM, int WN, int ST>
__device__ __forceinline__ void k_loop(f32x16 (&acc)[WM / 32][WN / 32], const float* a_src, const float* b_src, const Frame& f, int filter_k,
                                       int chunks, const Geom& g, float* sA, float* sB, int m0, int n0) {
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_LD = BM / 32, B_LD = BN / 32;        // DMA pieces per wave per chunk
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    const int kl = lane >> 5, il = lane & 31;
    const int drow = wave * 8 + (lane >> 3);
    const int dquad = ((lane & 7) ^ ((drow >> 1) & 7)) * 4;

    unsigned a_off[A_LD], b_off[B_LD];                  // per-lane byte offsets, constant for the whole loop
    {
        const unsigned howo = (unsigned)(g.Ho * g.Wo);
#pragma unroll
        for (int r = 0; r < A_LD; ++r) {
            const unsigned m = (unsigned)(m0 + drow + 32 * r);
            unsigned o = 0;                              // tile overhang rows read pixel 0 (results discarded)
            if (m < (unsigned)g.Mtot) {
                const unsigned b = fastdiv(m, howo, g.magic_howo), rem = m - b * howo;
                const unsigned ho = fastdiv(rem, (unsigned)g.Wo, g.magic_wo), wo = rem - ho * g.Wo;
                o = b * f.img_pitch + (ho * f.stride + f.off) * f.row_pitch + (wo * f.stride + f.off) * f.pix_pitch;
            }
            a_off[r] = (o + dquad) * 4u;
        }
#pragma unroll
        for (int r = 0; r < B_LD; ++r) b_off[r] = ((unsigned)(n0 + drow + 32 * r) * filter_k + dquad) * 4u;
    }
    const unsigned lds_a = (unsigned)(size_t)(lptr_t)(sA + wave * 8 * PBK);
    const unsigned lds_b = (unsigned)(size_t)(lptr_t)(sB + wave * 8 * PBK);
    auto advance = [&]() { a_src += PBK; b_src += PBK; };
    auto dma_chunk = [&](int buf) {
        const unsigned la = __builtin_amdgcn_readfirstlane(lds_a + buf * BM * PBK * 4);
        const unsigned lb = __builtin_amdgcn_readfirstlane(lds_b + buf * BN * PBK * 4);
#pragma unroll
        for (int r = 0; r < A_LD; ++r) lds_dma16_sv(a_off[r], a_src, la + r * 32 * PBK * 4);
#pragma unroll
        for (int r = 0; r < B_LD; ++r) lds_dma16_sv(b_off[r], b_src, lb + r * 32 * PBK * 4);
        advance();
    };
    auto dma_piece = [&](int p, const float* pa_src, const float* pb_src, unsigned la, unsigned lb) {
        if (p < A_LD) lds_dma16_sv(a_off[p < A_LD ? p : 0], pa_src, la + p * 32 * PBK * 4);
        else if (p < A_LD + B_LD) lds_dma16_sv(b_off[p >= A_LD && p < A_LD + B_LD ? p - A_LD : 0], pb_src, lb + (p - A_LD) * 32 * PBK * 4);
    };
    const int fsw = (il >> 1) & 7;                       // f(row) of the fragment rows this lane reads

    dma_chunk(0);
#pragma unroll
    for (int q = 1; q < ST - 1; ++q)
        if (q < chunks) dma_chunk(q);
    for (int c = 0; c < chunks; ++c) {
        const int buf = ST == 2 ? c & 1 : c % ST;
        {
            const int younger = min(ST - 2, chunks - 1 - c);
            if (ST >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (A_LD + B_LD)) : "memory");
            else if (ST >= 3 && younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_LD) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();                                     // everyone's pieces have landed, and the buffer refilled below is no longer being read
        static_assert(A_LD + B_LD <= (PBK / 8) * TM * TN, "one DMA piece per accumulator block of a chunk at most");
        const bool more = c + (ST - 1) < chunks;         // the chunk fetched during this one
        const float* na_src = a_src;
        const float* nb_src = b_src;
        const int nbuf = ST == 2 ? buf ^ 1 : (c + ST - 1) % ST;
        const unsigned nla = __builtin_amdgcn_readfirstlane(lds_a + nbuf * BM * PBK * 4);
        const unsigned nlb = __builtin_amdgcn_readfirstlane(lds_b + nbuf * BN * PBK * 4);
        if (more) advance();
        const float* pa = sA + (size_t)buf * BM * PBK + (wm0 + il) * PBK;
        const float* pb = sB + (size_t)buf * BN * PBK + (wn0 + il) * PBK;
        float4 a4[2][TM], b4[2][TN];
        auto load_frags = [&](int gq, int s) {
            const int slot = ((2 * gq + kl) ^ fsw) * 4;
#pragma unroll
            for (int i = 0; i < TM; ++i) a4[s][i] = *reinterpret_cast<const float4*>(pa + i * 32 * PBK + slot);
#pragma unroll
            for (int j = 0; j < TN; ++j) b4[s][j] = *reinterpret_cast<const float4*>(pb + j * 32 * PBK + slot);
        };
        load_frags(0, 0);
#pragma unroll
        for (int gq = 0; gq < PBK / 8; ++gq) {
            if (gq + 1 < PBK / 8) load_frags(gq + 1, (gq + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);
            // k order inside the group is x, y, z, w for every accumulator (the summation order of conv_pad.hip)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].x, a4[gq & 1][i].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].y, a4[gq & 1][i].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].z, a4[gq & 1][i].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].w, a4[gq & 1][i].w, acc[i][j], 0, 0, 0);
                    if (more) {
                        __builtin_amdgcn_sched_barrier(0);
                        dma_piece((gq * TM + i) * TN + j, na_src, nb_src, nla, nlb);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

template <int BM, int BN, int WM, int WN, int ST = 2>
__global__ __launch_bounds__(256) void expand_down_kernel(const float* __restrict__ t, const float* __restrict__ w3,
                                                          const float* __restrict__ scale3, const float* __restrict__ shift3,
                                                          const float* __restrict__ x, const float* __restrict__ wd,
                                                          const float* __restrict__ scaled, const float* __restrict__ shiftd,
                                                          float* __restrict__ y, const Geom g) {
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per workgroup");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;                                   // [ST][BM][32]
    float* sB = smem + ST * BM * PBK;                   // [ST][BN][32]
    const int bx = blockIdx.x;
    const int tile_n = bx / g.tiles_m, tile_m = bx % g.tiles_m;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    const int kl = lane >> 5, il = lane & 31;

    // the epilogue's layout (conv_pad.hip): each wave transposes its 32-pixel sub-tiles through a private LDS patch [32][WN + 4], then
    // WN / 4 consecutive lanes own one pixel's WN channels
    constexpr int EP = WN + 4;                 // patch pitch (floats)
    constexpr int LPP = WN / 4;                // lanes per pixel
    constexpr int PPI = 64 / LPP;              // pixels per wave instruction
    constexpr int U = 32 / PPI;
    static_assert(4 * 32 * EP <= ST * (BM + BN) * PBK, "the epilogue patches fit in the K-loop buffers");
    float* patch = smem + wave * 32 * EP;
    const int c4 = (lane % LPP) * 4;
    const int co = n0 + wn0 + c4;

    f32x16 acc[TM][TN];
    auto clear = [&]() {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    };
    auto to_patch = [&](int i) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4*>(patch + il * EP + j * 32 + 8 * q + 4 * kl) =
                    make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
    };

    // ---- the identity's tile: bn_d(conv_d(x)), finished as hps_conv2d_bn_act_pad (relu = 0, no residual) stores it ----
    clear();
    k_loop<BM, BN, WM, WN, ST>(acc, x, wd, g.x, g.x.pix_pitch, g.x.pix_pitch / PBK, g, sA, sB, m0, n0);
    float4 idv[TM][U];
    {
        const float4 sc = *reinterpret_cast<const float4*>(scaled + co), sh = *reinterpret_cast<const float4*>(shiftd + co);
        __syncthreads();                           // every wave is done with the K-loop buffers
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            to_patch(i);                           // wave-private patch: no barrier, the LDS queue is in order per wave
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float4 a = *reinterpret_cast<const float4*>(patch + (u * PPI + lane / LPP) * EP + c4);
                // "+ 0" as in conv_pad.hip's epilogue (residual absent = zero addend): the same bits
                idv[i][u] = make_float4(a.x * sc.x + sh.x + 0.f, a.y * sc.y + sh.y + 0.f, a.z * sc.z + sh.z + 0.f, a.w * sc.w + sh.w + 0.f);
            }
        }
        __syncthreads();                           // the patches lie in the buffers the next loop's DMA fills
    }

    // ---- the expand convolution, the sum and the ReLU ----
    clear();
    k_loop<BM, BN, WM, WN, ST>(acc, t, w3, g.t, g.t.pix_pitch, g.t.pix_pitch / PBK, g, sA, sB, m0, n0);
    const float4 sc = *reinterpret_cast<const float4*>(scale3 + co), sh = *reinterpret_cast<const float4*>(shift3 + co);
    __syncthreads();                               // every wave is done with the K-loop buffers
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        to_patch(i);
        if (m0 + BM <= g.Mtot) {                   // full tile: straight-line code (conv_pad.hip)
            unsigned po[U];
            float4 a[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                po[u] = out_pixel_offset((unsigned)(m0 + wm0 + i * 32 + u * PPI + lane / LPP), g) + (unsigned)co;
                a[u] = *reinterpret_cast<const float4*>(patch + (u * PPI + lane / LPP) * EP + c4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float4 v = make_float4(a[u].x * sc.x + sh.x + idv[i][u].x, a[u].y * sc.y + sh.y + idv[i][u].y,
                                       a[u].z * sc.z + sh.z + idv[i][u].z, a[u].w * sc.w + sh.w + idv[i][u].w);
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                *reinterpret_cast<float4*>(y + po[u]) = v;
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = m0 + wm0 + i * 32 + u * PPI + lane / LPP;
            const bool live = m < g.Mtot;
            const unsigned po = live ? out_pixel_offset((unsigned)m, g) + (unsigned)co : 0u;
            const float4 a = *reinterpret_cast<const float4*>(patch + (u * PPI + lane / LPP) * EP + c4);
            float4 v = make_float4(a.x * sc.x + sh.x + idv[i][u].x, a.y * sc.y + sh.y + idv[i][u].y, a.z * sc.z + sh.z + idv[i][u].z,
                                   a.w * sc.w + sh.w + idv[i][u].w);
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            if (live) *reinterpret_cast<float4*>(y + po) = v;
        }
    }
}

template <int BM, int BN, int WM, int WN, int ST = 2>
static int launch(const float* t, const float* w3, const float* scale3, const float* shift3, const float* x, const float* wd,
                  const float* scaled, const float* shiftd, float* y, Geom g, hipStream_t s) {
    g.tiles_m = ceil_div(g.Mtot, BM);
    const size_t lds = (size_t)ST * (BM + BN) * PBK * sizeof(float);
    static_assert((size_t)ST * (BM + BN) * PBK * sizeof(float) <= 64 * 1024, "within the default dynamic LDS");
    hipLaunchKernelGGL((expand_down_kernel<BM, BN, WM, WN, ST>), dim3(g.tiles_m * (g.Cout / BN)), dim3(256), lds, s, t, w3, scale3, shift3, x,
                       wd, scaled, shiftd, y, g);
    return check_launch("hps_bottleneck_expand_down");
}

}  // namespace expand
}  // namespace hps

using namespace hps;

extern "C" int hps_bottleneck_expand_down(const float* t, const float* w3, const float* scale3, const float* shift3, const float* x,
                                          const float* w_down, const float* scale_down, const float* shift_down, float* y, int B, int H,
                                          int W, int stride, int tpad, int xpad, int opad, int Cmid, int Cin, int Cout, int variant,
                                          int ksplit, hps_stream_t stream) {
    using namespace hps::expand;
    if (!t || !w3 || !scale3 || !shift3 || !x || !w_down || !scale_down || !shift_down || !y)
        return bad_arg("hps_bottleneck_expand_down: null pointer");
    if (stride != 1 && stride != 2) return bad_arg("hps_bottleneck_expand_down: stride must be 1 or 2");
    if (H <= 0 || W <= 0 || tpad < 0 || xpad < 0 || opad < 0) return bad_arg("hps_bottleneck_expand_down: H, W > 0 and halos >= 0 required");
    if (Cout <= 0 || Cout % 64 != 0) return bad_arg("hps_bottleneck_expand_down: Cout % 64 == 0 required");
    if (Cin <= 0 || Cin % PBK != 0) return bad_arg("hps_bottleneck_expand_down: Cin % 32 == 0 required");
    if (Cmid <= 0 || Cmid % PBK != 0) return bad_arg("hps_bottleneck_expand_down: Cmid % 32 == 0 required");
    if (ksplit > 1)
        return bad_arg("hps_bottleneck_expand_down: no split K (ksplit <= 1); issue the two convolutions through hps_conv2d_bn_act_pad");
    if (variant != 0 && variant != 1 && variant != 2 && variant != 3 && variant != 5)
        return bad_arg("hps_bottleneck_expand_down: variant must be 0, 1, 2, 3 or 5");
    if (B <= 0) return HPS_OK;
    Geom g;
    g.Ho = (H - 1) / stride + 1;
    g.Wo = (W - 1) / stride + 1;
    g.t.pix_pitch = Cmid;
    g.t.row_pitch = (g.Wo + 2 * tpad) * Cmid;
    g.t.img_pitch = (g.Ho + 2 * tpad) * g.t.row_pitch;
    g.t.stride = 1;
    g.t.off = tpad;
    g.x.pix_pitch = Cin;
    g.x.row_pitch = (W + 2 * xpad) * Cin;
    g.x.img_pitch = (H + 2 * xpad) * g.x.row_pitch;
    g.x.stride = stride;
    g.x.off = xpad;
    const size_t t_bytes = (size_t)B * (g.Ho + 2 * tpad) * (g.Wo + 2 * tpad) * Cmid * 4, x_bytes = (size_t)B * (H + 2 * xpad) * (W + 2 * xpad) * Cin * 4;
    const size_t y_floats = (size_t)B * (g.Ho + 2 * opad) * (g.Wo + 2 * opad) * Cout;
    if (t_bytes >= 0xffffffffull || x_bytes >= 0xffffffffull || (size_t)Cout * Cmid * 4 >= 0xffffffffull ||
        (size_t)Cout * Cin * 4 >= 0xffffffffull || y_floats >= 0xffffffffull || (size_t)B * g.Ho * g.Wo >= 0x7fffffffull)
        return bad_arg("hps_bottleneck_expand_down: tensor exceeds the 32-bit lane offsets");
    g.Mtot = B * g.Ho * g.Wo;
    g.Cout = Cout;
    g.opad = opad;
    g.tiles_m = 0;
    g.magic_howo = div_magic((unsigned)(g.Ho * g.Wo));
    g.magic_wo = div_magic((unsigned)g.Wo);
    hipStream_t s = (hipStream_t)stream;
    if (variant == 0) {
        // hps_conv2d_bn_act_pad's rule; where it picks the 256 x 64 tile (Cout = 64) the 64 x 64 one stands in: a tile shape never changes
        // an output's summation order
        if (Cout % 128 == 0 && ((long)g.Mtot / 128) * (Cout / 128) >= 256) variant = 1;
        else variant = 3;
    }
    if (variant == 1 && Cout % 128 != 0) variant = 2;
    switch (variant) {
        case 1: return launch<128, 128, 64, 64>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        case 2: return launch<128, 64, 64, 32>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        case 3: return launch<64, 64, 32, 32>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        default: return launch<64, 64, 32, 32, 4>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);      // 5: four-stage K loop
    }
}
