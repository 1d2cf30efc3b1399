// Backward of the ResNet-18 encoder (models/resnet.py:62-78, 202-217 under torch autograd) on halo-padded NHWC frames.
//
//   hps_conv_wgrad               G[co][ky][kx][ci] = sum over pixels of g[b,oy,ox,co] * x[b, oy s + ky - pad, ox s + kx - pad, ci]
//   hps_conv_dgrad               dx[b,iy,ix,ci] = sum over taps and co of g[b,oy,ox,co] * wt[ky][kx][co][ci]  (+ another branch's gradient)
//   hps_relu_gate_pad            g <- g * (y > 0) in place, per-channel sums of the gated cotangent
//   hps_maxpool3x3s2_backward    the cotangent goes to the first maximum of each 3x3 window (row-major)
//   hps_global_avgpool_backward  g / (H W) broadcast over the map
//
// Both GEMMs run on v_mfma_f32_32x32x2_f32 straight from global memory, one wave per 64 x 64 (64 x 32) output tile: with the channels
// on the lanes (NHWC) an A or B operand of the instruction is one coalesced 128-byte row per half wave, so neither kernel stages
// anything in LDS.  Every sum has a fixed order: no atomics anywhere, results are bitwise repeatable.
//
// Summation lengths.  An MFMA accumulator is a serial fp32 fma chain.  The weight gradient contracts over B Ho Wo pixels: the chain
// is cut into slices of wgrad_slice_pixels(Ho, Wo) pixels (a rule on the map alone), each slice's partial goes to the workspace and
// the finish pass adds the partials in slice order in float64 and rounds once.  The data gradient contracts over taps x Cout.  Inside
// a slice / over taps x Cout the chain is cut into pieces of 64 products whose partials are added in order in fp32 (see WGRAD_CHAIN).
#include "conv_backward.h"      // f32x16, WGRAD_CHAIN, DGRAD_CHAIN, zero16, mfma_row: shared with csrc/conv1x1_backward.hip

namespace hps {
namespace {

__host__ __device__ inline int wgrad_slice_pixels(int Ho, int Wo) {
    const long p = (long)Ho * Wo;
    return p < 128 ? 128 : (p > 512 ? 512 : (int)p);
}

// ---- weight gradient: one wave per (64 output channels, 32 NT input channels, tap, pixel slice) ----
template <int NT>
__global__ __launch_bounds__(64) void conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                        float* __restrict__ part, int B, int H, int W, int ipad, int Cx, int Cin,
                                                        int Cout, int KH, int KW, int stride, int pad, int gpad, int Ho, int Wo,
                                                        int S, int n_ci_tiles) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int co0 = (blockIdx.x / n_ci_tiles) * 64, ci0 = (blockIdx.x % n_ci_tiles) * (32 * NT);
    const int tap = blockIdx.y, ky = tap / KW, kx = tap % KW;
    const long total = (long)B * Ho * Wo;
    const long pbeg = (long)blockIdx.z * S;
    const long pend = pbeg + S < total ? pbeg + S : total;
    const int Hp = H + 2 * ipad, Wp = W + 2 * ipad, Hg = Ho + 2 * gpad, Wg = Wo + 2 * gpad;
    const long p0 = pbeg + h;                                   // this lane's pixel of the first step (k = lane >> 5)
    int b = (int)(p0 / ((long)Ho * Wo));
    const int rem = (int)(p0 % ((long)Ho * Wo));
    int oy = rem / Wo, ox = rem % Wo;
    const bool a_ok0 = co0 + r < Cout, a_ok1 = co0 + 32 + r < Cout;
    bool b_ok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b_ok[t] = ci0 + 32 * t + r < Cin;
    f32x16 tot[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[0][t] = tot[1][t] = zero16();
    for (long qc = pbeg; qc < pend; qc += WGRAD_CHAIN) {
    const long qe = qc + WGRAD_CHAIN < pend ? qc + WGRAD_CHAIN : pend;
    f32x16 acc[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = zero16();
#pragma unroll 4
    for (long q = qc; q < qe; q += 2) {
        float a0 = 0.0f, a1 = 0.0f, bv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bv[t] = 0.0f;
        if (q + h < pend) {
            const float* gp = g + (((long)b * Hg + oy + gpad) * Wg + ox + gpad) * Cout + co0 + r;
            if (a_ok0) a0 = gp[0];
            if (a_ok1) a1 = gp[32];
            const int iy = oy * stride + ky - pad + ipad, ix = ox * stride + kx - pad + ipad;
            if (iy >= 0 && iy < Hp && ix >= 0 && ix < Wp) {     // (always true with ipad >= pad: the halo holds the zero padding)
                const float* xp = x + (((long)b * Hp + iy) * Wp + ix) * Cx + ci0 + r;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (b_ok[t]) bv[t] = xp[32 * t];
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv[t], acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv[t], acc[1][t], 0, 0, 0);
        }
        ox += 2;
        while (ox >= Wo) { ox -= Wo; ++oy; }
        while (oy >= Ho) { oy -= Ho; ++b; }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        tot[0][t] += acc[0][t];
        tot[1][t] += acc[1][t];
    }
    }
    const long taps = (long)KH * KW;
    float* out = part + (long)blockIdx.z * Cout * taps * Cin;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = co0 + 32 * mt + mfma_row(i, h), ci = ci0 + 32 * t + r;
                if (co < Cout && ci < Cin) out[((long)co * taps + tap) * Cin + ci] = tot[mt][t][i];
            }
}

__global__ __launch_bounds__(256) void conv_wgrad_finish_kernel(const float* __restrict__ part, float* __restrict__ G, long n, int slices) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
#pragma unroll 8
    for (int sl = 0; sl < slices; ++sl) s += (double)part[(long)sl * n + e];
    G[e] = (float)s;
}

// ---- data gradient, gather form: one wave per (64 input pixels, 32 NT input channels) ----
template <int NT>
__global__ __launch_bounds__(64) void conv_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ wt,
                                                        const float* __restrict__ other, float* __restrict__ dx, int B, int H, int W,
                                                        int Cin, int Cout, int KH, int KW, int stride, int pad, int gpad, int dpad,
                                                        int Cdx, int Ho, int Wo) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int ci0 = blockIdx.y * (32 * NT);
    const long total = (long)B * H * W;
    const long q0 = (long)blockIdx.x * 64;
    const int Hg = Ho + 2 * gpad, Wg = Wo + 2 * gpad;
    int pb[2], py[2], px[2];
    bool pv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {                            // the pixels this lane feeds to the A operand (row = lane & 31)
        const long q = q0 + 32 * mt + r;
        pv[mt] = q < total;
        const long qq = pv[mt] ? q : 0;
        pb[mt] = (int)(qq / ((long)H * W));
        const int rem = (int)(qq % ((long)H * W));
        py[mt] = rem / W;
        px[mt] = rem % W;
    }
    bool b_ok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) b_ok[t] = ci0 + 32 * t + r < Cin;
    f32x16 tot[2][NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) tot[0][t] = tot[1][t] = zero16();
    for (int tap = 0; tap < KH * KW; ++tap) {
        const int ky = tap / KW, kx = tap % KW;
        bool ok[2];
        const float* gp[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int ty = py[mt] + pad - ky, tx = px[mt] + pad - kx;
            const int oy = ty / stride, ox = tx / stride;
            ok[mt] = pv[mt] && ty >= 0 && tx >= 0 && oy * stride == ty && ox * stride == tx && oy < Ho && ox < Wo;
            gp[mt] = g + (ok[mt] ? (((long)pb[mt] * Hg + oy + gpad) * Wg + ox + gpad) * Cout : 0) + 4 * h;
        }
        if (!__any(ok[0] || ok[1])) continue;                   // no pixel of the tile meets this tap (wave-uniform)
        const float* wp = wt + ((long)tap * Cout + 4 * h) * Cin + ci0 + r;
        for (int cb = 0; cb < Cout; cb += DGRAD_CHAIN) {
        const int ce = cb + DGRAD_CHAIN < Cout ? cb + DGRAD_CHAIN : Cout;
        f32x16 acc[2][NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[0][t] = acc[1][t] = zero16();
#pragma unroll 2
        for (int co0 = cb; co0 < ce; co0 += 8) {
            // K order inside a step of 8 output channels: lane half h holds channels co0 + 4 h + j, j = 0..3 (one 16-byte load)
            float4 a[2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
                a[mt] = ok[mt] ? *reinterpret_cast<const float4*>(gp[mt] + co0) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            const float av[2][4] = {{a[0].x, a[0].y, a[0].z, a[0].w}, {a[1].x, a[1].y, a[1].z, a[1].w}};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const float bw = b_ok[t] ? wp[(long)(co0 + j) * Cin + 32 * t] : 0.0f;
                    acc[0][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0][j], bw, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1][j], bw, acc[1][t], 0, 0, 0);
                }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            tot[0][t] += acc[0][t];
            tot[1][t] += acc[1][t];
        }
        }
    }
    const int Hd = H + 2 * dpad, Wd = W + 2 * dpad;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const long q = q0 + 32 * mt + mfma_row(i, h);
            if (q >= total) continue;
            const int b = (int)(q / ((long)H * W)), rem = (int)(q % ((long)H * W));
            const long base = (((long)b * Hd + rem / W + dpad) * Wd + rem % W + dpad) * Cdx;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int ci = ci0 + 32 * t + r;
                if (ci < Cin) {
                    float v = tot[mt][t][i];
                    if (other) v += other[base + ci];
                    dx[base + ci] = v;
                }
            }
        }
}

// ---- ReLU gate: 64 pixels x 64 channels per wave, the lane walks its channel's pixels in order ----
constexpr int GATE_PIXELS = 64;

__global__ __launch_bounds__(64) void relu_gate_kernel(float* __restrict__ g, const float* __restrict__ y, double* __restrict__ part,
                                                       int B, int H, int W, int C, int gpad, int ypad) {
    const int c = blockIdx.y * 64 + threadIdx.x;
    if (c >= C) return;
    const long total = (long)B * H * W;
    const long q0 = (long)blockIdx.x * GATE_PIXELS;
    const int n = (int)(q0 + GATE_PIXELS < total ? GATE_PIXELS : total - q0);
    const int Hg = H + 2 * gpad, Wg = W + 2 * gpad, Hy = H + 2 * ypad, Wy = W + 2 * ypad;
    int b = (int)(q0 / ((long)H * W));                          // the chunk's first pixel; the walk below is wave-uniform
    const int rem = (int)(q0 % ((long)H * W));
    int iy = rem / W, ix = rem % W;
    double s = 0.0;
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        const long gi = (((long)b * Hg + iy + gpad) * Wg + ix + gpad) * C + c;
        const long yi = (((long)b * Hy + iy + ypad) * Wy + ix + ypad) * C + c;
        const float v = y[yi] > 0.0f ? g[gi] : 0.0f;
        g[gi] = v;
        s += (double)v;
        if (++ix == W) {
            ix = 0;
            if (++iy == H) { iy = 0; ++b; }
        }
    }
    if (part) part[(long)blockIdx.x * C + c] = s;
}

__global__ __launch_bounds__(64) void relu_gate_finish_kernel(const double* __restrict__ part, float* __restrict__ sums, int C, long chunks) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (long k = 0; k < chunks; ++k) s += part[k * C + c];
    sums[c] = (float)s;
}

// ---- pools ----
__global__ __launch_bounds__(256) void maxpool_backward_kernel(const float* __restrict__ x, const float* __restrict__ gpool,
                                                               float* __restrict__ dx, int B, int H, int W, int C, int gpad, int Ho, int Wo) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * H * W * C) return;
    const int c = (int)(e % C);
    long q = e / C;
    const int ix = (int)(q % W);
    q /= W;
    const int iy = (int)(q % H), b = (int)(q / H);
    const float* xb = x + (long)b * H * W * C + c;
    const int Hg = Ho + 2 * gpad, Wg = Wo + 2 * gpad;
    float s = 0.0f;
    // the windows that hold (iy, ix): 2 o - 1 <= i <= 2 o + 1
    for (int oy = iy / 2; oy <= (iy + 1) / 2; ++oy) {
        if (oy >= Ho) continue;
        for (int ox = ix / 2; ox <= (ix + 1) / 2; ++ox) {
            if (ox >= Wo) continue;
            float best = -INFINITY;
            int by = -1, bx = -1;
            for (int wy = 0; wy < 3; ++wy) {
                const int yy = 2 * oy - 1 + wy;
                if (yy < 0 || yy >= H) continue;
                for (int wx = 0; wx < 3; ++wx) {
                    const int xx = 2 * ox - 1 + wx;
                    if (xx < 0 || xx >= W) continue;
                    const float v = xb[((long)yy * W + xx) * C];
                    if (v > best || by < 0) { best = v; by = yy; bx = xx; }     // strict: the first maximum in row-major order wins
                }
            }
            if (by == iy && bx == ix) s += gpool[(((long)b * Hg + oy + gpad) * Wg + ox + gpad) * C + c];
        }
    }
    dx[e] = s;
}

__global__ __launch_bounds__(256) void avgpool_backward_kernel(const float* __restrict__ gfeat, float* __restrict__ gframe, int B, int H,
                                                               int W, int C, int P) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)B * H * W * C) return;
    const int c = (int)(e % C);
    long q = e / C;
    const int ix = (int)(q % W);
    q /= W;
    const int iy = (int)(q % H), b = (int)(q / H);
    gframe[(((long)b * (H + 2 * P) + iy + P) * (W + 2 * P) + ix + P) * C + c] = gfeat[(long)b * C + c] / (float)(H * W);
}

bool conv_geometry(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* Ho, int* Wo) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0) return false;
    if (H + 2 * pad < KH || W + 2 * pad < KW) return false;
    *Ho = (H + 2 * pad - KH) / stride + 1;
    *Wo = (W + 2 * pad - KW) / stride + 1;
    return true;
}

}  // namespace
}  // namespace hps

using namespace hps;

extern "C" int hps_conv_wgrad_slice_pixels(int Ho, int Wo) { return (Ho < 1 || Wo < 1) ? 0 : wgrad_slice_pixels(Ho, Wo); }

extern "C" size_t hps_conv_wgrad_workspace(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    int Ho, Wo;
    if (!conv_geometry(B, H, W, Cin, Cout, KH, KW, stride, pad, &Ho, &Wo)) return 0;
    const long total = (long)B * Ho * Wo, S = wgrad_slice_pixels(Ho, Wo);
    return (size_t)((total + S - 1) / S) * Cout * KH * KW * Cin * sizeof(float);
}

extern "C" int hps_conv_wgrad(const float* x, const float* g, float* G, float* workspace, int B, int H, int W, int ipad, int Cx,
                              int Cin, int Cout, int KH, int KW, int stride, int pad, int gpad, hps_stream_t stream) {
    if (!x || !g || !G || !workspace) return bad_arg("hps_conv_wgrad: null pointer");
    int Ho, Wo;
    if (!conv_geometry(B, H, W, Cin, Cout, KH, KW, stride, pad, &Ho, &Wo)) return bad_arg("hps_conv_wgrad: geometry");
    if (ipad < pad) return bad_arg("hps_conv_wgrad: the input frame's halo is smaller than the padding");
    if (gpad < 0 || Cx < Cin) return bad_arg("hps_conv_wgrad: gpad >= 0 and Cx >= Cin required");
    const long total = (long)B * Ho * Wo;
    const int S = wgrad_slice_pixels(Ho, Wo);
    const long slices = (total + S - 1) / S;
    if (slices > 65535) return bad_arg("hps_conv_wgrad: more than 65535 pixel slices");
    const int nt = Cin > 32 ? 2 : 1;
    const int n_ci = ceil_div(Cin, 32 * nt), n_co = ceil_div(Cout, 64);
    const dim3 grid(n_co * n_ci, KH * KW, (unsigned)slices);
    hipStream_t s = (hipStream_t)stream;
    if (nt == 2)
        conv_wgrad_kernel<2><<<grid, 64, 0, s>>>(x, g, workspace, B, H, W, ipad, Cx, Cin, Cout, KH, KW, stride, pad, gpad, Ho, Wo, S, n_ci);
    else
        conv_wgrad_kernel<1><<<grid, 64, 0, s>>>(x, g, workspace, B, H, W, ipad, Cx, Cin, Cout, KH, KW, stride, pad, gpad, Ho, Wo, S, n_ci);
    const long n = (long)Cout * KH * KW * Cin;
    conv_wgrad_finish_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(workspace, G, n, (int)slices);
    return check_launch("hps_conv_wgrad");
}

extern "C" int hps_conv_dgrad(const float* g, const float* wt, const float* other, float* dx, int B, int H, int W, int Cin, int Cout,
                              int KH, int KW, int stride, int pad, int gpad, int dpad, int Cdx, hps_stream_t stream) {
    if (!g || !wt || !dx) return bad_arg("hps_conv_dgrad: null pointer");
    int Ho, Wo;
    if (!conv_geometry(B, H, W, Cin, Cout, KH, KW, stride, pad, &Ho, &Wo)) return bad_arg("hps_conv_dgrad: geometry");
    if (Cout % 8 != 0) return bad_arg("hps_conv_dgrad: Cout % 8 == 0 required");
    if (gpad < 0 || dpad < 0 || Cdx < Cin) return bad_arg("hps_conv_dgrad: gpad, dpad >= 0 and Cdx >= Cin required");
    if (other == dx) return bad_arg("hps_conv_dgrad: other must not alias dx");
    const long total = (long)B * H * W;
    const int nt = Cin > 32 ? 2 : 1;
    const dim3 grid((unsigned)((total + 63) / 64), ceil_div(Cin, 32 * nt));
    hipStream_t s = (hipStream_t)stream;
    if (nt == 2)
        conv_dgrad_kernel<2><<<grid, 64, 0, s>>>(g, wt, other, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, gpad, dpad, Cdx, Ho, Wo);
    else
        conv_dgrad_kernel<1><<<grid, 64, 0, s>>>(g, wt, other, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, gpad, dpad, Cdx, Ho, Wo);
    return check_launch("hps_conv_dgrad");
}

extern "C" size_t hps_relu_gate_workspace(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return 0;
    return (size_t)(((long)B * H * W + GATE_PIXELS - 1) / GATE_PIXELS) * C * sizeof(double);
}

extern "C" int hps_relu_gate_pad(float* g, const float* y, double* workspace, float* sums, int B, int H, int W, int C, int gpad, int ypad,
                                 hps_stream_t stream) {
    if (!g || !y) return bad_arg("hps_relu_gate_pad: null pointer");
    if ((sums != nullptr) != (workspace != nullptr)) return bad_arg("hps_relu_gate_pad: sums and workspace go together");
    if (B < 1 || H < 1 || W < 1 || C < 1 || gpad < 0 || ypad < 0) return bad_arg("hps_relu_gate_pad: geometry");
    const long chunks = ((long)B * H * W + GATE_PIXELS - 1) / GATE_PIXELS;
    hipStream_t s = (hipStream_t)stream;
    relu_gate_kernel<<<dim3((unsigned)chunks, ceil_div(C, 64)), 64, 0, s>>>(g, y, workspace, B, H, W, C, gpad, ypad);
    if (sums) relu_gate_finish_kernel<<<ceil_div(C, 64), 64, 0, s>>>(workspace, sums, C, chunks);
    return check_launch("hps_relu_gate_pad");
}

extern "C" int hps_maxpool3x3s2_backward(const float* x, const float* gpool, float* dx, int B, int H, int W, int C, int gpad,
                                         hps_stream_t stream) {
    if (!x || !gpool || !dx) return bad_arg("hps_maxpool3x3s2_backward: null pointer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || gpad < 0) return bad_arg("hps_maxpool3x3s2_backward: geometry");
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const long n = (long)B * H * W * C;
    maxpool_backward_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, gpool, dx, B, H, W, C, gpad, Ho, Wo);
    return check_launch("hps_maxpool3x3s2_backward");
}

extern "C" int hps_global_avgpool_backward(const float* gfeat, float* gframe, int B, int H, int W, int C, int P, hps_stream_t stream) {
    if (!gfeat || !gframe) return bad_arg("hps_global_avgpool_backward: null pointer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || P < 0) return bad_arg("hps_global_avgpool_backward: geometry");
    const long n = (long)B * H * W * C;
    avgpool_backward_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(gfeat, gframe, B, H, W, C, P);
    return check_launch("hps_global_avgpool_backward");
}
