// Grouped fp32-MFMA convolution for 16-channel granularity (include/hps.h: hps_conv2d_bn_act_c16): the layers of HRNet-W48
// (models/pose2D_hrnet.py) that csrc/conv_pad.hip (Cin % 32, Cout % 64) and csrc/conv_wino.hip (Cout % 64, 16 x 16-pixel blocks)
// do not take -- branch widths 48 and 96, maps of 96 x 72 ... 12 x 9 pixels, the 17-channel final layer.
//
// Implicit GEMM on v_mfma_f32_16x16x4_f32, operands straight from global memory (no LDS): a wave owns MT x 16 output pixels and up
// to NT x 16 output channels (NT = 4, or 1 for launches with few workgroups).  Lane l = (j = l & 15, q = l >> 4) holds, per
// 16-channel chunk, ONE float4 of its pixel's channels c0 + 4 q .. c0 + 4 q + 3 and one float4 of the same channels of filter row j
// of each 16-channel output group; step t = 0..3 of the chunk multiplies component t, i.e. the k slot q of step t is channel
// c0 + 4 q + t.  The filter is the A operand, so a lane ends up with four CONSECUTIVE output channels (4 q .. 4 q + 3 of the group)
// of its pixel: one 16-byte store into the NHWC frame.
//
// Summation order of an output (the layer alone decides it): accumulator 0; taps in the order (kh, kw); within a tap the channel
// chunks c0 = 0, 16, ...; within a chunk the steps t = 0..3, each ONE MFMA that adds the four products of channels c0 + t, c0 + 4 + t,
// c0 + 8 + t, c0 + 12 + t to the accumulator.  Nothing in it depends on B, on the tile (MT, NT), on the position of the pixel in its
// tile, or on the other problems of a grouped launch.  No atomics.
//
// Operand fragments live in a ring of four register sets: a chunk is fetched three chunks ahead of its MFMAs.
#include "hps_common.h"

namespace hps {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct C16Dev {
    const float* x;
    const float* w;
    const float* scale;
    const float* shift;
    const float* res;
    float* y;
    int Cin, Cout, Coutp, K, stride, Wo, HoWo, Mtot;
    int in_row, in_img, off;          // floats per frame row / image of x; ipad - pad
    int out_row, out_img, opad;       // floats per frame row / image of y (and residual)
    int relu, tiles_n, blk_end;       // blk_end: first block index behind this problem's blocks
};

// register sets of operand fragments in flight per wave: a chunk is fetched C16_STAGES - 1 chunks ahead of its MFMAs (a wave's K loop
// is serial, and with one or a few images nothing else on the SIMD covers the fetch latency)
constexpr int C16_STAGES = 4;

struct C16Table {
    C16Dev p[HPS_C16_MAX_PROBLEMS];
    int n;
};

template <int MT, int NT>
__global__ __launch_bounds__(256) void conv_c16_kernel(const C16Table tab) {
    // which problem: block-uniform
    int pi = 0;
#pragma unroll
    for (int i = 0; i + 1 < HPS_C16_MAX_PROBLEMS; ++i)
        if (i + 1 < tab.n && (int)blockIdx.x >= tab.p[i].blk_end) pi = i + 1;
    const C16Dev& P = tab.p[pi];
    const int blk = (int)blockIdx.x - (pi ? tab.p[pi - 1].blk_end : 0);
    const int tile_n = blk % P.tiles_n, tile_m = blk / P.tiles_n;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int Cin = P.Cin, Coutp = P.Coutp, K = P.K;

    const int n0 = tile_n * (16 * NT);
    const int nact = min(NT, (Coutp - n0) >> 4);                 // active 16-channel output groups of this tile: wave-uniform

    int a_off[MT], o_off[MT];
    bool valid[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int m = tile_m * (64 * MT) + wave * (16 * MT) + mt * 16 + j;
        valid[mt] = m < P.Mtot;
        const int mm = valid[mt] ? m : 0;                       // pixel 0 always exists: a masked lane reads it and stores nothing
        const int b = mm / P.HoWo, r = mm - b * P.HoWo;
        const int oy = r / P.Wo, ox = r - oy * P.Wo;
        a_off[mt] = b * P.in_img + (oy * P.stride + P.off) * P.in_row + (ox * P.stride + P.off) * Cin + 4 * q;
        o_off[mt] = b * P.out_img + (oy + P.opad) * P.out_row + (ox + P.opad) * P.Cout;
    }
    int w_off[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) w_off[nt] = (n0 + min(nt, nact - 1) * 16 + j) * Cin + 4 * q;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int cchunks = Cin >> 4;
    const int nchunks = K * K * cchunks;
    const int tap_w = Coutp * Cin;
    // walking state of the NEXT chunk to fetch
    int kw = 0, cc = 0;
    int xo = 0, wo = 0;                                          // float offsets of (kh, kw, c0) into x / w
    float4 a_buf[C16_STAGES][MT], b_buf[C16_STAGES][NT];
    auto fetch = [&](float4(&a)[MT], float4(&b)[NT]) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const float4*>(P.x + (a_off[mt] + xo));
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
            if (nt < nact) b[nt] = *reinterpret_cast<const float4*>(P.w + (w_off[nt] + wo));
        // advance to the following chunk
        ++cc;
        xo += 16;
        wo += 16;
        if (cc == cchunks) {
            cc = 0;
            ++kw;                                                // the tap row's next pixel follows this one's channels: xo is there
            if (kw == K) {
                kw = 0;                                          // next filter row
                xo += P.in_row - K * Cin;
            }
            wo += tap_w - Cin;
        }
    };
    auto multiply = [&](const float4(&a)[MT], const float4(&b)[NT]) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                if (nt < nact) {
                    const float bv = t == 0 ? b[nt].x : t == 1 ? b[nt].y : t == 2 ? b[nt].z : b[nt].w;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const float av = t == 0 ? a[mt].x : t == 1 ? a[mt].y : t == 2 ? a[mt].z : a[mt].w;
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv, av, acc[mt][nt], 0, 0, 0);
                    }
                }
            }
        }
    };
#pragma unroll
    for (int s = 0; s < C16_STAGES; ++s) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) b_buf[s][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < nchunks) fetch(a_buf[s], b_buf[s]);
    }
    // chunk it + s lives in register set s; once multiplied, the set is refilled with chunk it + s + C16_STAGES
    for (int it = 0; it < nchunks; it += C16_STAGES) {
#pragma unroll
        for (int s = 0; s < C16_STAGES; ++s) {
            if (it + s < nchunks) {
                multiply(a_buf[s], b_buf[s]);
                if (it + s + C16_STAGES < nchunks) fetch(a_buf[s], b_buf[s]);
            }
        }
    }

    // epilogue: y = act(acc * scale + shift [+ residual]); lane: pixel j of each mt, channels n0 + 16 nt + 4 q + (0..3)
    const int Cout = P.Cout;
    const bool vec = (Cout & 3) == 0;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (nt >= nact) continue;
        const int co = n0 + nt * 16 + 4 * q;
        if (co >= Cout) continue;
        if (vec) {
            const float4 sc = *reinterpret_cast<const float4*>(P.scale + co);
            const float4 sh = *reinterpret_cast<const float4*>(P.shift + co);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if (!valid[mt]) continue;
                float4 v;
                v.x = __builtin_fmaf(acc[mt][nt][0], sc.x, sh.x);
                v.y = __builtin_fmaf(acc[mt][nt][1], sc.y, sh.y);
                v.z = __builtin_fmaf(acc[mt][nt][2], sc.z, sh.z);
                v.w = __builtin_fmaf(acc[mt][nt][3], sc.w, sh.w);
                if (P.res) {
                    const float4 r = *reinterpret_cast<const float4*>(P.res + (o_off[mt] + co));
                    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
                }
                if (P.relu) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
                *reinterpret_cast<float4*>(P.y + (o_off[mt] + co)) = v;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = co + r;
                if (c >= Cout) continue;
                const float sc = P.scale[c], sh = P.shift[c];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    if (!valid[mt]) continue;
                    float v = __builtin_fmaf(acc[mt][nt][r], sc, sh);
                    if (P.res) v += P.res[o_off[mt] + c];
                    if (P.relu) v = fmaxf(v, 0.f);
                    P.y[o_off[mt] + c] = v;
                }
            }
        }
    }
}

// Validates one problem and fills its device descriptor (tiles_n for NT = 4; blk_end is the launch's to set); *mtot receives its
// number of output pixels B * Ho * Wo (0: nothing to do).
static int c16_fill(const hps_c16_problem& p, C16Dev& d, long* mtot) {
    if (!p.x || !p.w || !p.scale || !p.shift || !p.y) return bad_arg("hps_conv2d_bn_act_c16: null pointer");
    if (p.Cin <= 0 || p.Cin % 16 != 0) return bad_arg("hps_conv2d_bn_act_c16: Cin % 16 == 0 required");
    if (p.K != 1 && p.K != 3) return bad_arg("hps_conv2d_bn_act_c16: filter size must be 1 or 3 (square, pad = K / 2)");
    if (p.stride != 1 && p.stride != 2) return bad_arg("hps_conv2d_bn_act_c16: stride must be 1 or 2");
    const int pad = p.K / 2;
    if (p.ipad < pad || p.opad < 0) return bad_arg("hps_conv2d_bn_act_c16: the input halo must cover the convolution padding");
    if (p.Cout < 1 || p.H < 1 || p.W < 1 || p.B < 0) return bad_arg("hps_conv2d_bn_act_c16: Cout, H, W >= 1 and B >= 0 required");
    const uintptr_t align_in = (uintptr_t)p.x | (uintptr_t)p.w;
    uintptr_t align_out = 0;
    if (p.Cout % 4 == 0) align_out = (uintptr_t)p.y | (uintptr_t)p.residual | (uintptr_t)p.scale | (uintptr_t)p.shift;
    if ((align_in | align_out) & 15) return bad_arg("hps_conv2d_bn_act_c16: pointers must be 16-byte aligned");
    const int Ho = (p.H + 2 * pad - p.K) / p.stride + 1, Wo = (p.W + 2 * pad - p.K) / p.stride + 1;
    const int Coutp = (p.Cout + 15) / 16 * 16;
    const long Hp = p.H + 2 * p.ipad, Wp = p.W + 2 * p.ipad;
    const long in_elems = (long)p.B * Hp * Wp * p.Cin, out_elems = (long)p.B * (Ho + 2 * p.opad) * (Wo + 2 * p.opad) * p.Cout;
    if (in_elems >= 0x7fffffffL || out_elems >= 0x7fffffffL || (long)p.K * p.K * Coutp * p.Cin >= 0x7fffffffL)
        return bad_arg("hps_conv2d_bn_act_c16: tensor exceeds the 32-bit lane offsets");
    d.x = p.x; d.w = p.w; d.scale = p.scale; d.shift = p.shift; d.res = p.residual; d.y = p.y;
    d.Cin = p.Cin; d.Cout = p.Cout; d.Coutp = Coutp; d.K = p.K; d.stride = p.stride;
    d.Wo = Wo; d.HoWo = Ho * Wo; d.Mtot = p.B * Ho * Wo;
    d.in_row = (int)(Wp * p.Cin); d.in_img = (int)(Hp * Wp * p.Cin); d.off = p.ipad - pad;
    d.out_row = (Wo + 2 * p.opad) * p.Cout; d.out_img = (Ho + 2 * p.opad) * d.out_row; d.opad = p.opad;
    d.relu = p.relu ? 1 : 0;
    d.tiles_n = (Coutp + 63) / 64;                               // for NT = 4; the launch recomputes it for the tile it picks
    d.blk_end = 0;
    *mtot = d.Mtot;
    return HPS_OK;
}

}  // namespace hps

using namespace hps;

extern "C" int hps_sizeof_c16_problem(void) { return (int)sizeof(hps_c16_problem); }

extern "C" int hps_conv2d_bn_act_c16(const hps_c16_problem* problems, int n_problems, hps_stream_t stream) {
    if (n_problems == 0) return HPS_OK;
    if (!problems) return bad_arg("hps_conv2d_bn_act_c16: null pointer (problem table)");
    if (n_problems < 0 || n_problems > HPS_C16_MAX_PROBLEMS)
        return bad_arg("hps_conv2d_bn_act_c16: 1 to 4 problems per launch");
    C16Table tab;
    long mtot[HPS_C16_MAX_PROBLEMS];
    int n = 0;
    long blocks1 = 0;
    for (int i = 0; i < n_problems; ++i) {
        C16Dev d;
        long m = 0;
        if (int rc = c16_fill(problems[i], d, &m)) return rc;
        if (m == 0) continue;                                    // B == 0: nothing to do
        mtot[n] = m;
        tab.p[n++] = d;
        blocks1 += (m + 63) / 64 * d.tiles_n;
    }
    if (n == 0) return HPS_OK;
    // The tile -- MT x 16 pixels and NT x 16 output channels per wave -- never changes an output's summation order; it is picked for the
    // whole launch by the number of workgroups: 32 pixels per wave once 16 would give every CU more than four workgroups, 16 channels
    // per wave (four times the workgroups, each with a quarter of the serial MFMA chain) while 64 would leave CUs without one.
    const int MT = blocks1 > 4 * 256 ? 2 : 1;
    const int NT = blocks1 < 2 * 256 ? 1 : 4;
    long total = 0;
    for (int i = 0; i < n; ++i) {
        tab.p[i].tiles_n = (tab.p[i].Coutp + 16 * NT - 1) / (16 * NT);
        total += (mtot[i] + 64 * MT - 1) / (64 * MT) * tab.p[i].tiles_n;
        if (total >= 0x7fffffffL) return bad_arg("hps_conv2d_bn_act_c16: too many tiles");
        tab.p[i].blk_end = (int)total;
    }
    for (int i = n; i < HPS_C16_MAX_PROBLEMS; ++i) tab.p[i] = tab.p[n - 1];
    tab.n = n;
    hipStream_t s = (hipStream_t)stream;
    if (MT == 2) hipLaunchKernelGGL((conv_c16_kernel<2, 4>), dim3((unsigned)total), dim3(256), 0, s, tab);
    else if (NT == 4) hipLaunchKernelGGL((conv_c16_kernel<1, 4>), dim3((unsigned)total), dim3(256), 0, s, tab);
    else hipLaunchKernelGGL((conv_c16_kernel<1, 1>), dim3((unsigned)total), dim3(256), 0, s, tab);
    return check_launch("hps_conv2d_bn_act_c16");
}
