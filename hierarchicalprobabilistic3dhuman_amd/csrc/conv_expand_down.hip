// Bottleneck entry block (models/resnet.py:102-122 with the down-sample branch built at :184-188): the expand convolution conv3 (1x1 / 1)
// + bn3, the block's down-sample (1x1 / s) + BatchNorm on the block's input, their sum and the ReLU in ONE launch
// (hps_bottleneck_expand_down).  The identity bn_d(conv_d(x)) has the output geometry and the Cout of conv3 and its only reader is
// conv3's epilogue, so a workgroup computes its own tile of it first -- a K loop over the Cin channels of x -- finishes it (scale, shift,
// + 0, rounded as the separate launch stores it) into registers in the epilogue's pixel-row layout, runs the K loop again over the Cmid
// channels of t, and adds the held tile where hps_conv2d_bn_act_pad reads its residual frame.  The frame of the identity is never
// written or read.  Every output has the bits of the two launches
//     hps_conv2d_bn_act_pad(x, w_d, ..., stride, relu = 0) -> d;   hps_conv2d_bn_act_pad(t, w_3, ..., residual = d, relu = 1)
// because this kernel and conv_pad_kernel (csrc/conv_pad.hip) instantiate the same loop (csrc/conv_tile.h: lane_offsets, k_loop over the
// chunks of one tap, the same stages, DMA spreading, fragment order and MFMA sequence) and the same patch transpose, and finish a
// sub-tile with the same expression, scale * acc + shift + addend: the addend is the held tile here, a residual frame or 0 there.
#include "conv_tile.h"

namespace hps {
namespace expand {

struct Geom {
    InFrame t, x;                          // the expand convolution's input (stride 1) and the block's input (stride s), read by 1x1 windows
    OutGeom out;
    int tiles_m;
};

template <int BM, int BN, int WM, int WN, int ST = 2>
__global__ __launch_bounds__(256) void expand_down_kernel(const float* __restrict__ t, const float* __restrict__ w3,
                                                          const float* __restrict__ scale3, const float* __restrict__ shift3,
                                                          const float* __restrict__ x, const float* __restrict__ wd,
                                                          const float* __restrict__ scaled, const float* __restrict__ shiftd,
                                                          float* __restrict__ y, const Geom g) {
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    typedef PatchShape<WN> P;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per workgroup");
    static_assert(4 * 32 * P::EP <= ST * (BM + BN) * PBK, "the epilogue patches fit in the K-loop buffers");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;                                   // [ST][BM][32]
    float* sB = smem + ST * BM * PBK;                   // [ST][BN][32]
    const int bx = blockIdx.x;
    const int tile_n = bx / g.tiles_m, tile_m = bx % g.tiles_m;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    float* patch = wave_patch<WN>(smem, wave);
    const int c4 = patch_channel<WN>(lane);
    const int co = n0 + wn0 + c4;

    f32x16 acc[TM][TN];
    // acc = (the tile's pixels of frame f) x (its filters of the (Cout, f.pix_pitch) filter w)^T
    auto conv1x1 = [&](const float* src, const float* w, const InFrame& f) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        const auto off = lane_offsets<BM / 32, BN / 32>(f, g.out, f.pix_pitch, m0, n0, lane, wave);
        LinearWalk walk{src, w};
        k_loop<BM, BN, WM, WN, ST>(acc, off, walk, f.pix_pitch / PBK, sA, sB, true);
    };

    // ---- the identity's tile: bn_d(conv_d(x)), finished as hps_conv2d_bn_act_pad (relu = 0, no residual) stores it ----
    conv1x1(x, wd, g.x);
    float4 idv[TM][P::U];
    {
        const float4 sc = *reinterpret_cast<const float4*>(scaled + co), sh = *reinterpret_cast<const float4*>(shiftd + co);
        __syncthreads();                           // every wave is done with the K-loop buffers
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            to_patch<WN>(patch, acc[i], lane);
#pragma unroll
            for (int u = 0; u < P::U; ++u) {
                const float4 a = *reinterpret_cast<const float4*>(patch + (u * P::PPI + lane / P::LPP) * P::EP + c4);
                // "+ 0" as in conv_pad.hip's epilogue (residual absent = zero addend): the same bits
                idv[i][u] = make_float4(a.x * sc.x + sh.x + 0.f, a.y * sc.y + sh.y + 0.f, a.z * sc.z + sh.z + 0.f, a.w * sc.w + sh.w + 0.f);
            }
        }
        __syncthreads();                           // the patches lie in the buffers the next loop's DMA fills
    }

    // ---- the expand convolution, the sum and the ReLU ----
    conv1x1(t, w3, g.t);
    const float4 sc = *reinterpret_cast<const float4*>(scale3 + co), sh = *reinterpret_cast<const float4*>(shift3 + co);
    __syncthreads();                               // every wave is done with the K-loop buffers
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        to_patch<WN>(patch, acc[i], lane);
        if (m0 + BM <= g.out.Mtot) {               // full tile: straight-line code (conv_pad.hip)
            unsigned po[P::U];
            float4 a[P::U];
#pragma unroll
            for (int u = 0; u < P::U; ++u) {
                po[u] = out_pixel_offset((unsigned)(m0 + wm0 + i * 32 + u * P::PPI + lane / P::LPP), g.out) + (unsigned)co;
                a[u] = *reinterpret_cast<const float4*>(patch + (u * P::PPI + lane / P::LPP) * P::EP + c4);
            }
#pragma unroll
            for (int u = 0; u < P::U; ++u) {
                float4 v = make_float4(a[u].x * sc.x + sh.x + idv[i][u].x, a[u].y * sc.y + sh.y + idv[i][u].y, a[u].z * sc.z + sh.z + idv[i][u].z, a[u].w * sc.w + sh.w + idv[i][u].w);
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                *reinterpret_cast<float4*>(y + po[u]) = v;
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < P::U; ++u) {
            const int m = m0 + wm0 + i * 32 + u * P::PPI + lane / P::LPP;
            const bool live = m < g.out.Mtot;
            const unsigned po = live ? out_pixel_offset((unsigned)m, g.out) + (unsigned)co : 0u;
            const float4 a = *reinterpret_cast<const float4*>(patch + (u * P::PPI + lane / P::LPP) * P::EP + c4);
            float4 v = make_float4(a.x * sc.x + sh.x + idv[i][u].x, a.y * sc.y + sh.y + idv[i][u].y, a.z * sc.z + sh.z + idv[i][u].z, a.w * sc.w + sh.w + idv[i][u].w);
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            if (live) *reinterpret_cast<float4*>(y + po) = v;
        }
    }
}

template <int BM, int BN, int WM, int WN, int ST = 2>
static int launch(const float* t, const float* w3, const float* scale3, const float* shift3, const float* x, const float* wd,
                  const float* scaled, const float* shiftd, float* y, Geom g, hipStream_t s) {
    g.tiles_m = ceil_div(g.out.Mtot, BM);
    const size_t lds = (size_t)ST * (BM + BN) * PBK * sizeof(float);
    static_assert((size_t)ST * (BM + BN) * PBK * sizeof(float) <= 64 * 1024, "within the default dynamic LDS");
    hipLaunchKernelGGL((expand_down_kernel<BM, BN, WM, WN, ST>), dim3(g.tiles_m * (g.out.Cout / BN)), dim3(256), lds, s, t, w3, scale3, shift3, x,
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
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    Geom g;
    g.t.pix_pitch = Cmid;
    g.t.row_pitch = (Wo + 2 * tpad) * Cmid;
    g.t.img_pitch = (Ho + 2 * tpad) * g.t.row_pitch;
    g.t.stride = 1;
    g.t.off = tpad;
    g.x.pix_pitch = Cin;
    g.x.row_pitch = (W + 2 * xpad) * Cin;
    g.x.img_pitch = (H + 2 * xpad) * g.x.row_pitch;
    g.x.stride = stride;
    g.x.off = xpad;
    const size_t t_floats = (size_t)B * (Ho + 2 * tpad) * (Wo + 2 * tpad) * Cmid, x_floats = (size_t)B * (H + 2 * xpad) * (W + 2 * xpad) * Cin;
    const size_t y_floats = (size_t)B * (Ho + 2 * opad) * (Wo + 2 * opad) * Cout;
    if (!fits_lane_offsets(t_floats) || !fits_lane_offsets(x_floats) || !fits_lane_offsets((size_t)Cout * Cmid) ||
        !fits_lane_offsets((size_t)Cout * Cin) || y_floats >= 0xffffffffull || (size_t)B * Ho * Wo >= 0x7fffffffull)
        return bad_arg("hps_bottleneck_expand_down: tensor exceeds the 32-bit lane offsets");
    set_out_geom(g.out, B, Ho, Wo, Cout, opad);
    g.tiles_m = 0;
    hipStream_t s = (hipStream_t)stream;
    variant = resolve_tile_variant(variant, g.out.Mtot, Cout);
    if (variant == 4) variant = 3;         // the 64 x 64 tile stands in for 256 x 64: a tile shape never changes an output's summation order
    switch (variant) {
        case 1: return launch<128, 128, 64, 64>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        case 2: return launch<128, 64, 64, 32>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        case 3: return launch<64, 64, 32, 32>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);
        default: return launch<64, 64, 32, 32, 4>(t, w3, scale3, shift3, x, w_down, scale_down, shift_down, y, g, s);      // 5: four-stage K loop
    }
}
