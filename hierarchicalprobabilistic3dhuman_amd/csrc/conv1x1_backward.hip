// Both gradients of a 1x1 / pad 0 convolution (the 36 pointwise layers and the four down-samples of the Bottleneck encoder,
// models/resnet.py:92-96, :105, :113, :184-188, under torch autograd) as LDS-tiled GEMMs over NHWC rows on v_mfma_f32_32x32x2_f32.
//
//   hps_conv1x1_dgrad   dx[b,iy,ix,ci] = sum over co of g[b, iy / s, ix / s, co] * wt[co][ci]   (+ another branch's gradient)
//   hps_conv1x1_wgrad   G[co][ci]      = sum over pixels of g[b,oy,ox,co] * x[b, oy s, ox s, ci]
//
// A workgroup is four waves, each on a 64 x 64 (64 x 32) part of a 128 x 128 (128 x 64) output tile; both operands of a K stage of 32
// go global -> registers -> LDS once per workgroup (the next stage's loads are in flight during the MFMAs of this one), where
// csrc/conv_backward.hip has every wave read its rows from global memory again.
//
// Summation orders.  hps_conv1x1_dgrad repeats hps_conv_dgrad's: inside a step of 8 output channels MFMA j contracts channels
// co0 + j and co0 + 4 + j, the fp32 chain is cut every DGRAD_CHAIN channels and the pieces are added in order -- the same sequence of
// (a, b) pairs enters each accumulator, so every output has that kernel's bits whatever tile it falls in.  hps_conv1x1_wgrad cuts the
// pixel sum into slices of conv1x1_wgrad_slice_pixels(Cin, Cout) pixels -- a rule on the layer alone --, adds chain pieces of
// WGRAD_CHAIN pixels in order inside a slice, and the slices in slice order in float64, rounded once.  No atomics anywhere.
#include "conv_backward.h"

namespace hps {
namespace {

constexpr int C1_THREADS = 256;
constexpr int C1_BM = 128;                 // rows of a workgroup's tile: dx pixels (dgrad), output channels (wgrad)
constexpr int C1_KS = 32;                  // K of one LDS stage: output channels (dgrad), pixels (wgrad)
constexpr int C1_AS = C1_KS + 4;           // dgrad A row (one pixel's 32 channels) + 16 bytes: the 16-byte reads of 32 rows spread over the banks
constexpr int C1_WS = C1_BM + 32;          // wgrad rows (one pixel's 128 channels): the two lane halves read rows 2k and 2k + 1, 32 banks apart

// twice the harmonic mean of the channel counts, at least 1024, a multiple of WGRAD_CHAIN: with P >= that many pixels the
// ceil(P / S) partial filters take at most P (Cin + Cout) / 2 + Cin Cout floats, the two operands P (Cin + Cout) or more
__host__ __device__ inline int conv1x1_wgrad_slice_pixels(int Cin, int Cout) {
    const long hm = (2l * Cin * Cout + Cin + Cout - 1) / ((long)Cin + Cout);
    const long s = (hm + WGRAD_CHAIN - 1) / WGRAD_CHAIN * WGRAD_CHAIN;
    return (int)(s < 1024 ? 1024 : s);
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// four floats of a row whose first ``n`` exist (n <= 0: none); ``vec``: the row is 16-byte aligned and n is 0 or >= 4
__device__ __forceinline__ float4 load4(const float* p, int n, bool vec) {
    if (n <= 0) return zero4();
    if (vec) return *reinterpret_cast<const float4*>(p);
    float4 v = zero4();
    v.x = p[0];
    if (n > 1) v.y = p[1];
    if (n > 2) v.z = p[2];
    if (n > 3) v.w = p[3];
    return v;
}

// ---- data gradient: 128 dx pixels x 64 NT input channels per workgroup, K = Cout in stages of 32 ----
template <int NT>
__global__ __launch_bounds__(C1_THREADS, 2) void conv1x1_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ wt,
                                                                   const float* __restrict__ other, float* __restrict__ dx, int B, int H,
                                                                   int W, int Cin, int Cout, int stride, int gpad, int dpad, int Cdx,
                                                                   int Ho, int Wo) {
    constexpr int BN = 64 * NT;                                 // input channels per workgroup
    constexpr int BS = BN + 8;                                  // B row: lane half h reads rows 4 h + j, 32 banks apart
    constexpr int BROW = BN / 4;                                // loader threads per B row (16 bytes each)
    constexpr int BPASS = C1_KS * BROW / C1_THREADS;            // B rows are loaded in this many passes of 256 / BROW rows
    __shared__ float As[C1_BM * C1_AS];
    __shared__ float Bs[C1_KS * BS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const long total = (long)B * H * W;
    const long q0 = (long)blockIdx.x * C1_BM;
    const int ci0 = blockIdx.y * BN;
    const int Hg = Ho + 2 * gpad, Wg = Wo + 2 * gpad;
    const bool vec = (Cin & 3) == 0;

    // loader: thread t brings channels 4 (t % 8) .. + 3 of pixels t / 8 + 32 i (A) and columns 4 (t % BROW) .. + 3 of rows t / BROW + .. (B)
    const int arow = tid >> 3, acol = (tid & 7) * 4;
    const int brow = tid / BROW, bcol = (tid % BROW) * 4;
    long aoff[4];                                               // the pixel's row of g; -1: past the end or off the stride lattice (zero)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long q = q0 + arow + 32 * i;
        aoff[i] = -1;
        if (q < total) {
            const int b = (int)(q / ((long)H * W)), rem = (int)(q % ((long)H * W));
            const int iy = rem / W, ix = rem % W;
            const int oy = iy / stride, ox = ix / stride;
            if (oy * stride == iy && ox * stride == ix && oy < Ho && ox < Wo)
                aoff[i] = (((long)b * Hg + oy + gpad) * Wg + ox + gpad) * Cout;
        }
    }
    float4 ra[4], rb[BPASS];
    auto load_stage = [&](int cs) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ra[i] = (aoff[i] >= 0 && cs + acol < Cout) ? *reinterpret_cast<const float4*>(g + aoff[i] + cs + acol) : zero4();
#pragma unroll
        for (int i = 0; i < BPASS; ++i) {
            const int co = cs + brow + (C1_THREADS / BROW) * i, ci = ci0 + bcol;
            rb[i] = co < Cout ? load4(wt + (long)co * Cin + ci, Cin - ci, vec) : zero4();
        }
    };

    f32x16 tot[2][NT], acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[0][t] = tot[1][t] = acc[0][t] = acc[1][t] = zero16();
    load_stage(0);
    for (int cs = 0; cs < Cout; cs += C1_KS) {
        __syncthreads();                                        // the previous stage has been read
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&As[(arow + 32 * i) * C1_AS + acol]) = ra[i];
#pragma unroll
        for (int i = 0; i < BPASS; ++i) *reinterpret_cast<float4*>(&Bs[(brow + (C1_THREADS / BROW) * i) * BS + bcol]) = rb[i];
        __syncthreads();
        if (cs + C1_KS < Cout) load_stage(cs + C1_KS);
        const int steps = (Cout - cs < C1_KS ? Cout - cs : C1_KS) >> 3;         // Cout % 8 == 0; wave-uniform
        for (int st = 0; st < steps; ++st) {
            // K order inside a step of 8 output channels, as conv_dgrad_kernel: lane half h holds channels co0 + 4 h + j, j = 0..3
            float4 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) a[mt] = *reinterpret_cast<const float4*>(&As[(wm * 64 + 32 * mt + r) * C1_AS + 8 * st + 4 * h]);
            const float av[2][4] = {{a[0].x, a[0].y, a[0].z, a[0].w}, {a[1].x, a[1].y, a[1].z, a[1].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float bw = Bs[(8 * st + 4 * h + j) * BS + wn * 32 * NT + 32 * t + r];
                    acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bw, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bw, acc[1][t], 0, 0, 0);
                }
        }
        if (((cs + C1_KS) % DGRAD_CHAIN) == 0 || cs + C1_KS >= Cout) {          // a chain piece ends: add it, in order
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                tot[0][t] += acc[0][t];
                tot[1][t] += acc[1][t];
                acc[0][t] = acc[1][t] = zero16();
            }
        }
    }
    const int Hd = H + 2 * dpad, Wd = W + 2 * dpad;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long q = q0 + wm * 64 + 32 * mt + mfma_row(i, h);
            if (q >= total) continue;
            const int b = (int)(q / ((long)H * W)), rem = (int)(q % ((long)H * W));
            const long base = (((long)b * Hd + rem / W + dpad) * Wd + rem % W + dpad) * Cdx;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int ci = ci0 + wn * 32 * NT + 32 * t + r;
                if (ci < Cin) {
                    float v = tot[mt][t][i];
                    if (other) v += other[base + ci];
                    dx[base + ci] = v;
                }
            }
        }
}

// ---- weight gradient: 128 output channels x 128 input channels per workgroup and pixel slice, K = pixels in stages of 32 ----
__global__ __launch_bounds__(C1_THREADS) void conv1x1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                   float* __restrict__ part, int B, int H, int W, int ipad, int Cx, int Cin,
                                                                   int Cout, int stride, int gpad, int Ho, int Wo, int S, int n_ci_tiles) {
    __shared__ float As[C1_KS * C1_WS];
    __shared__ float Bs[C1_KS * C1_WS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const int co0 = (blockIdx.x / n_ci_tiles) * C1_BM, ci0 = (blockIdx.x % n_ci_tiles) * C1_BM;
    const int total = B * Ho * Wo, map = Ho * Wo;               // below 2^31 (checked on the host)
    const long pb = (long)blockIdx.y * S;
    const int pbeg = (int)pb, pend = (int)(pb + S < total ? pb + S : total);
    const int Hp = H + 2 * ipad, Wp = W + 2 * ipad, Hg = Ho + 2 * gpad, Wg = Wo + 2 * gpad;
    const bool vec = (Cin & 3) == 0 && (Cx & 3) == 0;
    const int prow = tid >> 5, col = (tid & 31) * 4;            // loader: channels col .. col + 3 of pixels prow + 8 i of the stage
    float4 ra[4], rb[4];
    auto load_stage = [&](int p0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = p0 + prow + 8 * i;
            ra[i] = rb[i] = zero4();
            if (p < pend) {
                const int b = p / map, rem = p - b * map;
                const int oy = rem / Wo, ox = rem - oy * Wo;
                if (co0 + col < Cout)                           // Cout % 8 == 0: all four or none, 16-byte aligned
                    ra[i] = *reinterpret_cast<const float4*>(g + (((long)b * Hg + oy + gpad) * Wg + ox + gpad) * Cout + co0 + col);
                rb[i] = load4(x + (((long)b * Hp + oy * stride + ipad) * Wp + ox * stride + ipad) * Cx + ci0 + col, Cin - ci0 - col, vec);
            }
        }
    };
    f32x16 tot[2][2], acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) tot[0][t] = tot[1][t] = acc[0][t] = acc[1][t] = zero16();
    load_stage(pbeg);
    for (int p0 = pbeg; p0 < pend; p0 += C1_KS) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4*>(&As[(prow + 8 * i) * C1_WS + col]) = ra[i];
            *reinterpret_cast<float4*>(&Bs[(prow + 8 * i) * C1_WS + col]) = rb[i];
        }
        __syncthreads();
        if (p0 + C1_KS < pend) load_stage(p0 + C1_KS);
#pragma unroll 4
        for (int k = 0; k < C1_KS / 2; ++k) {                   // MFMA k contracts pixels p0 + 2 k and p0 + 2 k + 1 (zeros past the slice)
            float a[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = As[(2 * k + h) * C1_WS + wm * 64 + 32 * t + r];
                bv[t] = Bs[(2 * k + h) * C1_WS + wn * 64 + 32 * t + r];
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], bv[t], acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], bv[t], acc[1][t], 0, 0, 0);
            }
        }
        if (((p0 - pbeg + C1_KS) % WGRAD_CHAIN) == 0 || p0 + C1_KS >= pend) {     // a chain piece of 64 pixels ends: add it, in order
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                tot[0][t] += acc[0][t];
                tot[1][t] += acc[1][t];
                acc[0][t] = acc[1][t] = zero16();
            }
        }
    }
    float* out = part + (long)blockIdx.y * Cout * Cin;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + wm * 64 + 32 * mt + mfma_row(i, h), ci = ci0 + wn * 64 + 32 * t + r;
                if (co < Cout && ci < Cin) out[(long)co * Cin + ci] = tot[mt][t][i];
            }
}

__global__ __launch_bounds__(256) void conv1x1_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ G, long n, int slices) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
#pragma unroll 4
    for (int sl = 0; sl < slices; ++sl) s += (double)part[(long)sl * n + e];
    G[e] = (float)s;
}

// output map of a 1x1 / stride / pad 0 layer; false: sizes the kernels' index arithmetic does not carry (pixel counts are ints there)
bool conv1x1_geometry(int B, int H, int W, int Cin, int Cout, int stride, int* Ho, int* Wo) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (stride != 1 && stride != 2)) return false;
    *Ho = (H - 1) / stride + 1;
    *Wo = (W - 1) / stride + 1;
    return true;
}

bool fits_int(long frame_pixels) { return frame_pixels < (1l << 31) - 4 * C1_BM; }

}  // namespace
}  // namespace hps

using namespace hps;

extern "C" int hps_conv1x1_wgrad_slice_pixels(int Cin, int Cout) { return (Cin < 1 || Cout < 1) ? 0 : conv1x1_wgrad_slice_pixels(Cin, Cout); }

extern "C" size_t hps_conv1x1_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int stride) {
    int Ho, Wo;
    if (!conv1x1_geometry(B, H, W, Cin, Cout, stride, &Ho, &Wo)) return 0;
    const long total = (long)B * Ho * Wo, S = conv1x1_wgrad_slice_pixels(Cin, Cout);
    return (size_t)((total + S - 1) / S) * Cout * Cin * sizeof(float);
}

extern "C" int hps_conv1x1_wgrad(const float* x, const float* g, float* G, float* workspace, int B, int H, int W, int ipad, int Cx,
                                 int Cin, int Cout, int stride, int gpad, hps_stream_t stream) {
    if (!x || !g || !G || !workspace) return bad_arg("hps_conv1x1_wgrad: null pointer");
    if (stride != 1 && stride != 2) return bad_arg("hps_conv1x1_wgrad: stride 1 or 2 required");
    int Ho, Wo;
    if (!conv1x1_geometry(B, H, W, Cin, Cout, stride, &Ho, &Wo)) return bad_arg("hps_conv1x1_wgrad: geometry");
    if (Cout % 8 != 0) return bad_arg("hps_conv1x1_wgrad: Cout % 8 == 0 required");
    if (ipad < 0 || gpad < 0 || Cx < Cin) return bad_arg("hps_conv1x1_wgrad: ipad, gpad >= 0 and Cx >= Cin required");
    if (!fits_int((long)B * (H + 2l * ipad) * (W + 2l * ipad)) || !fits_int((long)B * (Ho + 2l * gpad) * (Wo + 2l * gpad)))
        return bad_arg("hps_conv1x1_wgrad: 2^31 frame pixels or more");
    const long total = (long)B * Ho * Wo;
    const int S = conv1x1_wgrad_slice_pixels(Cin, Cout);
    const long slices = (total + S - 1) / S;
    if (slices > 65535) return bad_arg("hps_conv1x1_wgrad: more than 65535 pixel slices");
    const int n_ci = ceil_div(Cin, C1_BM), n_co = ceil_div(Cout, C1_BM);
    hipStream_t s = (hipStream_t)stream;
    conv1x1_wgrad_kernel<<<dim3(n_co * n_ci, (unsigned)slices), C1_THREADS, 0, s>>>(x, g, workspace, B, H, W, ipad, Cx, Cin, Cout, stride, gpad,
                                                                                  Ho, Wo, S, n_ci);
    const long n = (long)Cout * Cin;
    conv1x1_wgrad_finish_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(workspace, G, n, (int)slices);
    return check_launch("hps_conv1x1_wgrad");
}

extern "C" int hps_conv1x1_dgrad(const float* g, const float* wt, const float* other, float* dx, int B, int H, int W, int Cin, int Cout,
                                 int stride, int gpad, int dpad, int Cdx, hps_stream_t stream) {
    if (!g || !wt || !dx) return bad_arg("hps_conv1x1_dgrad: null pointer");
    if (stride != 1 && stride != 2) return bad_arg("hps_conv1x1_dgrad: stride 1 or 2 required");
    int Ho, Wo;
    if (!conv1x1_geometry(B, H, W, Cin, Cout, stride, &Ho, &Wo)) return bad_arg("hps_conv1x1_dgrad: geometry");
    if (Cout % 8 != 0) return bad_arg("hps_conv1x1_dgrad: Cout % 8 == 0 required");
    if (gpad < 0 || dpad < 0 || Cdx < Cin) return bad_arg("hps_conv1x1_dgrad: gpad, dpad >= 0 and Cdx >= Cin required");
    if (other == dx) return bad_arg("hps_conv1x1_dgrad: other must not alias dx");
    if (!fits_int((long)B * (H + 2l * dpad) * (W + 2l * dpad)) || !fits_int((long)B * (Ho + 2l * gpad) * (Wo + 2l * gpad)))
        return bad_arg("hps_conv1x1_dgrad: 2^31 frame pixels or more");
    const long total = (long)B * H * W;
    const int nt = Cin > 64 ? 2 : 1;
    const dim3 grid((unsigned)((total + C1_BM - 1) / C1_BM), ceil_div(Cin, 64 * nt));
    hipStream_t s = (hipStream_t)stream;
    if (nt == 2)
        conv1x1_dgrad_kernel<2><<<grid, C1_THREADS, 0, s>>>(g, wt, other, dx, B, H, W, Cin, Cout, stride, gpad, dpad, Cdx, Ho, Wo);
    else
        conv1x1_dgrad_kernel<1><<<grid, C1_THREADS, 0, s>>>(g, wt, other, dx, B, H, W, Cin, Cout, stride, gpad, dpad, Cdx, Ho, Wo);
    return check_launch("hps_conv1x1_dgrad");
}
