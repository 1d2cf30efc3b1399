// What the direct implicit-GEMM convolution kernels share: conv_pad_kernel (csrc/conv_pad.hip) and expand_down_kernel
// (csrc/conv_expand_down.hip) differ in what a workgroup does with its tile, not in how a tile is computed or stored.  One workgroup =
// 4 waves on a BM pixels x BN filters tile; both operands reach LDS by LDS-DMA from halo-padded NHWC frames; a wave's WM x WN part is
// TM x TN accumulator blocks of v_mfma_f32_32x32x2f32.  This header holds the one K loop, the lane offsets that feed it and the layout
// of the epilogue, so two launches that must agree to the bit instantiate the same code.  (The scale / shift / addend / ReLU store of a
// sub-tile is written out in both kernels: docs/conv_tile.md has what the compiler did with a shared one.)
// The shared pieces take the kernel's lane and wave instead of reading threadIdx again: with a second read hipcc placed the
// epilogue's waits differently (docs/conv_tile.md).
#pragma once

#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PBK = 32;   // K-chunk (floats); one 128-byte LDS row per tile row

// n / d for n < 2^32 with magic = floor(2^32 / d) (0xffffffff for d = 1): the estimate is at most one short
__device__ __forceinline__ unsigned fastdiv(unsigned n, unsigned d, unsigned magic) {
    unsigned q = __umulhi(n, magic);
    if (n - q * d >= d) ++q;
    return q;
}
static unsigned div_magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ull / d); }

// one 1-KiB LDS-DMA piece: lane l fetches 16 bytes at sbase + voff and they land at lds_addr + 16 l.
// Issued from inline asm so that hipcc does not drain it in front of the next ds_read (conv.hip lds_dma16).
__device__ __forceinline__ void lds_dma16_sv(unsigned voff, const float* sbase, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(sbase), "s"(lds_addr)
                 : "memory");
}

// one halo-padded NHWC input frame: tap (0, 0) of output pixel (b, ho, wo) reads pixel (ho * stride + off, wo * stride + off)
struct InFrame {
    int img_pitch, row_pitch, pix_pitch;   // floats
    int stride, off;
};
// the output pixels m = (b * Ho + ho) * Wo + wo of a launch and the frame (halo opad) they are stored to
struct OutGeom {
    int Ho, Wo, Mtot, Cout, opad;
    unsigned magic_howo, magic_wo;
};
inline void set_out_geom(OutGeom& o, int B, int Ho, int Wo, int Cout, int opad) {
    o.Ho = Ho; o.Wo = Wo; o.Mtot = B * Ho * Wo; o.Cout = Cout; o.opad = opad;
    o.magic_howo = div_magic((unsigned)(Ho * Wo));
    o.magic_wo = div_magic((unsigned)Wo);
}

// offset (floats) of output pixel m, channel 0, in the output frame
__device__ __forceinline__ unsigned out_pixel_offset(unsigned m, const OutGeom& o) {
    const unsigned howo = (unsigned)(o.Ho * o.Wo);
    const unsigned b = fastdiv(m, howo, o.magic_howo), rem = m - b * howo;
    const unsigned ho = fastdiv(rem, (unsigned)o.Wo, o.magic_wo), wo = rem - ho * o.Wo;
    return ((b * (o.Ho + 2 * o.opad) + ho + o.opad) * (o.Wo + 2 * o.opad) + wo + o.opad) * (unsigned)o.Cout;
}

// offset (floats) of the window start of output pixel m in input frame f; tile overhang rows read pixel 0 (results discarded)
__device__ __forceinline__ unsigned in_pixel_offset(unsigned m, const InFrame& f, const OutGeom& o) {
    if (m >= (unsigned)o.Mtot) return 0;
    const unsigned howo = (unsigned)(o.Ho * o.Wo);
    const unsigned b = fastdiv(m, howo, o.magic_howo), rem = m - b * howo;
    const unsigned ho = fastdiv(rem, (unsigned)o.Wo, o.magic_wo), wo = rem - ho * o.Wo;
    return b * f.img_pitch + (ho * f.stride + f.off) * f.row_pitch + (wo * f.stride + f.off) * f.pix_pitch;
}

// The per-lane byte offsets of a tile's DMA pieces, constant for a whole K loop.  DMA role of a lane: tile row
// (32 r + 8 wave + lane / 8), LDS slot lane % 8 <- source quad slot ^ f(row), f(row) = (row >> 1) & 7 (conv.hip: conflict-free
// ds_read_b128).  a: pixel m0 + row -> its window start in frame f; b: filter n0 + row of a (Cout, filter_k) n-major filter.
template <int A_LD, int B_LD>
struct LaneOffsets {
    unsigned a[A_LD], b[B_LD];
};
template <int A_LD, int B_LD>
__device__ __forceinline__ LaneOffsets<A_LD, B_LD> lane_offsets(const InFrame& f, const OutGeom& o, int filter_k, int m0, int n0, int lane,
                                                                 int wave) {
    LaneOffsets<A_LD, B_LD> off;
    const int drow = wave * 8 + (lane >> 3);
    const int dquad = ((lane & 7) ^ ((drow >> 1) & 7)) * 4;
#pragma unroll
    for (int r = 0; r < A_LD; ++r) off.a[r] = (in_pixel_offset((unsigned)(m0 + drow + 32 * r), f, o) + dquad) * 4u;
#pragma unroll
    for (int r = 0; r < B_LD; ++r) off.b[r] = ((unsigned)(n0 + drow + 32 * r) * filter_k + dquad) * 4u;
    return off;
}

// Where the chunks of a K loop come from: the SGPR base pointers of the chunk fetched next, moved on by scalar code.
// TapWalk: the (kh, kw, ci0) walk over a window -- the A pointer advances by 32 floats per chunk and jumps at tap / row ends.
struct TapWalk {
    const float* a_src;
    const float* b_src;
    int ci, kw;                            // chunk inside the tap, tap inside the filter row
    int cpt, kws;                          // chunks per tap, taps per filter row
    int tap_jump, row_jump;                // from the last chunk of a tap to the next tap / to the next filter row
    __device__ __forceinline__ void advance() {
        b_src += PBK;
        if (++ci < cpt) a_src += PBK;
        else {
            ci = 0;
            if (++kw < kws) a_src += tap_jump;
            else { kw = 0; a_src += row_jump; }
        }
    }
};
// LinearWalk: a 1x1 window (one tap: both sources advance by one chunk)
struct LinearWalk {
    const float* a_src;
    const float* b_src;
    __device__ __forceinline__ void advance() { a_src += PBK; b_src += PBK; }
};

// acc += A (BM pixels x K) * B (BN filters x K)^T over ``chunks`` chunks of 32 floats, starting where ``walk`` stands.
// ST = K-loop stages (LDS buffers per operand: sA [ST][BM][32], sB [ST][BN][32]).  2: the next chunk's DMA pieces are issued during this
// chunk's MFMAs (the throughput form: several workgroups per CU cover each other's DMA latency).  3 / 4 (round 5, latency mode:
// hps_conv2d_bn_act_pad variant 5): two / three chunks ahead -- at batch 1 a 64 x 64 tile's chunk is 16 MFMAs per wave (0.43 us) with
// ONE workgroup on the CU, and a chunk fetched one ahead arrived ~0.6 us after it was needed: 1.0 us per chunk, 18.3 us for a layer1
// convolution of 18 chunks (three stages: 15.3 us).
// spread = false is the dev library's hps_dev_conv_pad_ablate(3) (the earlier burst, two-stage form only); the product passes true.
template <int BM, int BN, int WM, int WN, int ST, class Walk>
__device__ __forceinline__ void k_loop(f32x16 (&acc)[WM / 32][WN / 32], const LaneOffsets<BM / 32, BN / 32>& off,
                                       Walk& walk, int chunks, float* sA, float* sB, const bool spread) {
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_LD = BM / 32, B_LD = BN / 32;        // DMA pieces per wave per chunk
    typedef __attribute__((address_space(3))) void* lptr_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    const int kl = lane >> 5, il = lane & 31;

    const unsigned lds_a = (unsigned)(size_t)(lptr_t)(sA + wave * 8 * PBK);
    const unsigned lds_b = (unsigned)(size_t)(lptr_t)(sB + wave * 8 * PBK);
    auto dma_chunk = [&](int buf) {
        const unsigned la = __builtin_amdgcn_readfirstlane(lds_a + buf * BM * PBK * 4);
        const unsigned lb = __builtin_amdgcn_readfirstlane(lds_b + buf * BN * PBK * 4);
#pragma unroll
        for (int r = 0; r < A_LD; ++r) lds_dma16_sv(off.a[r], walk.a_src, la + r * 32 * PBK * 4);
#pragma unroll
        for (int r = 0; r < B_LD; ++r) lds_dma16_sv(off.b[r], walk.b_src, lb + r * 32 * PBK * 4);
        walk.advance();
    };
    // one piece of the chunk whose sources are (pa_src, pb_src): piece p < A_LD is an A piece, the rest B pieces
    auto dma_piece = [&](int p, const float* pa_src, const float* pb_src, unsigned la, unsigned lb) {
        if (p < A_LD) lds_dma16_sv(off.a[p < A_LD ? p : 0], pa_src, la + p * 32 * PBK * 4);
        else if (p < A_LD + B_LD) lds_dma16_sv(off.b[p >= A_LD && p < A_LD + B_LD ? p - A_LD : 0], pb_src, lb + (p - A_LD) * 32 * PBK * 4);
    };

    const int fsw = (il >> 1) & 7;                       // f(row) of the fragment rows this lane reads
    dma_chunk(0);
#pragma unroll
    for (int q = 1; q < ST - 1; ++q)
        if (q < chunks) dma_chunk(q);
    for (int c = 0; c < chunks; ++c) {
        const int buf = ST == 2 ? c & 1 : c % ST;
        // this wave's pieces of chunk c have landed; with more than two stages the pieces of up to ST - 2 younger chunks, issued after
        // them (A_LD + B_LD per chunk), may still be in flight
        {
            const int younger = min(ST - 2, chunks - 1 - c);
            if (ST >= 4 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (A_LD + B_LD)) : "memory");
            else if (ST >= 3 && younger >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_LD + B_LD) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();                                     // ... everyone's have, and the buffer refilled below is no longer being read
        // The next chunk's DMA pieces are issued ONE PER FOUR MFMAs, not in a burst after the barrier: every 1 KiB piece costs the
        // SIMD 36-57 cycles that no other wave's MFMAs cover (tools/mfma_dma_overlap.hip: the loop skeleton runs at 139.4 TF/s with
        // the burst and 143.0 spread); on the stem 0.906 -> 0.888 ms (tests/dev/stem_ablate.py, mode 3 = burst).
        static_assert(A_LD + B_LD <= (PBK / 8) * TM * TN, "one DMA piece per accumulator block of a chunk at most");
        const bool more = c + (ST - 1) < chunks;         // the chunk fetched during this one: c + 1 (two stages), c + 2, c + 3
        const float* na_src = walk.a_src;
        const float* nb_src = walk.b_src;
        const int nbuf = ST == 2 ? buf ^ 1 : (c + ST - 1) % ST;
        const unsigned nla = __builtin_amdgcn_readfirstlane(lds_a + nbuf * BM * PBK * 4);
        const unsigned nlb = __builtin_amdgcn_readfirstlane(lds_b + nbuf * BN * PBK * 4);
        if (more) {
            if (spread) walk.advance();
            else dma_chunk(buf ^ 1);
        }
        const float* pa = sA + (size_t)buf * BM * PBK + (wm0 + il) * PBK;
        const float* pb = sB + (size_t)buf * BN * PBK + (wn0 + il) * PBK;
        // Fragments are double-buffered by hand: group gq + 1 is requested before the MFMAs of group gq are issued (the
        // sched_barriers keep hipcc from sinking the reads to their uses -- left alone it reloads the same 16 registers after
        // the group's last MFMA and waits out the LDS round trip in front of the next group).
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
            // k order inside the group is x, y, z, w for every accumulator (same summation order as conv.hip)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].x, a4[gq & 1][i].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].y, a4[gq & 1][i].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].z, a4[gq & 1][i].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b4[gq & 1][j].w, a4[gq & 1][i].w, acc[i][j], 0, 0, 0);
                    if (spread && more) {
                        __builtin_amdgcn_sched_barrier(0);
                        dma_piece((gq * TM + i) * TN + j, na_src, nb_src, nla, nlb);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// The epilogue's layout.  The filter fragment is the MFMA's row operand and the pixel fragment its column operand (products commute,
// the k order is unchanged), so a lane ends up with ONE pixel (column = lane & 31) and, per register quad q, four consecutive output
// channels: row = (r & 3) + 8 q + 4 (lane >> 5)  ->  128-bit accesses along Cout.  Each wave transposes its 32-pixel sub-tiles through
// a private LDS patch [32][WN + 4] (the +4 keeps both the 128-bit writes -- 16 lanes = 16 pixels, bank step 4 -- and the row reads
// conflict free), then WN/4 consecutive lanes own one pixel's WN channels: residual loads and output stores are 16 bytes per lane,
// WN*4 contiguous bytes per pixel (64 stores -> 16 per wave).  The four patches lie in the K-loop buffers: a __syncthreads() separates
// them from the loop before and from a loop after.
template <int WN>
struct PatchShape {
    static constexpr int EP = WN + 4;      // patch pitch (floats)
    static constexpr int LPP = WN / 4;     // lanes per pixel
    static constexpr int PPI = 64 / LPP;   // pixels per wave instruction
    static constexpr int U = 32 / PPI;     // pixels per lane and sub-tile
};
// this wave's patch, and the first of the four channels a lane owns there (+ n0 + wn0: in the output frame)
template <int WN>
__device__ __forceinline__ float* wave_patch(float* smem, int wave) { return smem + wave * 32 * PatchShape<WN>::EP; }
template <int WN>
__device__ __forceinline__ int patch_channel(int lane) { return (lane % PatchShape<WN>::LPP) * 4; }

// one 32-pixel sub-tile (TN accumulator blocks) into the wave-private patch: no barrier, the LDS queue is in order per wave
template <int WN>
__device__ __forceinline__ void to_patch(float* patch, const f32x16 (&acc)[WN / 32], int lane) {
    const int kl = lane >> 5, il = lane & 31;
#pragma unroll
    for (int j = 0; j < WN / 32; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4*>(patch + il * PatchShape<WN>::EP + j * 32 + 8 * q + 4 * kl) =
                make_float4(acc[j][4 * q], acc[j][4 * q + 1], acc[j][4 * q + 2], acc[j][4 * q + 3]);
}

// ---- host side ----

// The tile variant of hps_conv2d_bn_act_pad's numbering for a request: 0 = the rule of hps_conv2d_bn_act_v3 (measured per layer): the
// largest tile that still gives every CU a workgroup; 1 (128 x 128) falls back to 2 (128 x 64) where Cout is no multiple of 128.
inline int resolve_tile_variant(int variant, int Mtot, int Cout) {
    if (variant == 0) {
        if (Cout % 128 == 0 && ((long)Mtot / 128) * (Cout / 128) >= 256) variant = 1;
        else if (Cout == 64 && Mtot / 256 >= 512) variant = 4;
        else variant = 3;
    }
    if (variant == 1 && Cout % 128 != 0) variant = 2;
    return variant;
}

// a tensor of this many floats is within reach of the 32-bit per-lane byte offsets
inline bool fits_lane_offsets(size_t floats) { return floats * 4 < 0xffffffffull; }

}  // namespace hps
