// Training-mode BatchNorm of the ResNet-18 encoder (models/resnet.py: every nn.BatchNorm2d under model.train(); torch's batch_norm
// with training=True) on halo-padded NHWC frames, forward and backward.
//
//   hps_bn_batch_stats           per-channel mean and biased variance over the B H W interior pixels of a raw (pre-BatchNorm) frame
//   hps_bn_train_fold            mean, var, gamma, beta -> fp32 scale / shift, float64 invstd, the running-buffer update
//   hps_bn_apply_act_pad         y = act(z scale + shift [+ residual]), the convolution epilogue as a pass of its own
//   hps_bn_train_backward_sums   d beta = sum g, d gamma = sum g zhat per channel, the ReLU gate g <- g (y > 0) in the same sweep
//   hps_bn_train_backward_dz     dz = gamma invstd (g - d beta / n - zhat d gamma / n), out of place
//
// All four map kernels are bandwidth kernels of one shape.  The interior of a frame row (b, iy) is W C contiguous floats, so a
// workgroup of 256 lanes walks whole rows with 16-byte loads, four independent loads per lane in flight; 256 % (C / 4) == 0 keeps a
// lane on the same four channels for the whole walk (one division per row, none per pixel).  More than 1024 channels (a multiple of
// 1024: the Bottleneck encoder's 2048) are cut into windows of 1024, one per blockIdx.y; up to 1024 channels the walk, and with it
// every sum's order, is what it was.  At most 2048 workgroups per window.  The two
// reductions cut the B H rows into bn_chunks(B H) contiguous chunks -- a rule on the row count alone --, accumulate in float64 per
// lane, add the lanes of a channel in lane order through LDS and the chunks in a fixed order in a finish launch: no atomics, bitwise
// repeatable.  The variance uses sums shifted by a per-channel pivot (the channel's first interior pixel), so |mean| >> std costs
// nothing: s1 = sum (z - K), s2 = sum (z - K)^2, var = (s2 - s1^2 / n) / n.
#include "hps_common.h"

namespace hps {
namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_MAX_CHUNKS = 2048;
constexpr int BN_FIN_CH = 8;                       // channels per finish workgroup; 256 / 8 = 32 chunk slices each

__host__ __device__ inline int bn_chunks(long rows) { return rows < BN_MAX_CHUNKS ? (int)rows : BN_MAX_CHUNKS; }

// first float of the interior of row r = b H + iy of a (B, H + 2 pad, W + 2 pad, C) frame
__device__ __forceinline__ size_t bn_row_base(long r, int H, int W, int C, int pad) {
    const long b = r / H, iy = r - b * H;
    return ((size_t)(b * (H + 2 * pad) + iy + pad) * (size_t)(W + 2 * pad) + (size_t)pad) * (size_t)C;
}

__device__ __forceinline__ float4 ld4(const float* p, int j) { return reinterpret_cast<const float4*>(p)[j]; }

// The lane's place in a row of W pixels x cq channel quads: its quad c4 of the pixel (window blockIdx.y of cw = min(cq, 256) quads), its
// first pixel p0 and the pixels it advances per step; the 16-byte element of pixel px is px cq + c4.  With cq <= 256 that is element
// threadIdx.x + 256 k of the row for k = 0, 1, ...: the walk of a contiguous row.
struct BnLane {
    int cq, cw, q, c4, p0, pstep;
    __device__ __forceinline__ BnLane(int C) {
        cq = C >> 2;
        cw = cq < BN_THREADS ? cq : BN_THREADS;
        q = threadIdx.x % cw;
        c4 = blockIdx.y * cw + q;
        p0 = threadIdx.x / cw;
        pstep = BN_THREADS / cw;
    }
    __device__ __forceinline__ int at(int px) const { return px * cq + c4; }
};

// the lanes of a channel quad (lane % cq) hold 8 doubles each: per value, the sum over those lanes in lane order -> part[chunk][8 cq]
// laid out as [value / 4][channel] (value 0..3: first quantity of channels 4 q .. 4 q + 3, 4..7: second quantity)
__device__ __forceinline__ void bn_block_reduce(const double (&a)[8], double* red, double* part_chunk, int cq, int C, int c0 = 0) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) red[i * BN_THREADS + t] = a[i];
    __syncthreads();
    const int peers = BN_THREADS / cq;
    for (int o = t; o < 8 * cq; o += BN_THREADS) {
        const int i = o / cq, q = o - i * cq;
        double s = 0.0;
        for (int p = 0; p < peers; ++p) s += red[i * BN_THREADS + q + p * cq];
        part_chunk[(i >> 2) * C + c0 + 4 * q + (i & 3)] = s;
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_stats_kernel(const float* __restrict__ z, double* __restrict__ part, int B, int H, int W,
                                                              int C, int pad, int nchunks) {
    __shared__ double red[8 * BN_THREADS];
    const BnLane L(C);
    const int ps = L.pstep;
    const long R = (long)B * H;
    const long r0 = (long)blockIdx.x * R / nchunks, r1 = ((long)blockIdx.x + 1) * R / nchunks;
    const float4 k = ld4(z + bn_row_base(0, H, W, C, pad), L.c4);              // the pivots of this lane's four channels
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto add = [&](const float4& v) {
        const double d0 = (double)v.x - (double)k.x, d1 = (double)v.y - (double)k.y, d2 = (double)v.z - (double)k.z,
                     d3 = (double)v.w - (double)k.w;
        a[0] += d0; a[1] += d1; a[2] += d2; a[3] += d3;
        a[4] = fma(d0, d0, a[4]); a[5] = fma(d1, d1, a[5]); a[6] = fma(d2, d2, a[6]); a[7] = fma(d3, d3, a[7]);
    };
    for (long r = r0; r < r1; ++r) {
        const float* p = z + bn_row_base(r, H, W, C, pad);
        int px = L.p0;
        for (; px + 3 * ps < W; px += 4 * ps) {
            const float4 v0 = ld4(p, L.at(px)), v1 = ld4(p, L.at(px + ps)), v2 = ld4(p, L.at(px + 2 * ps)), v3 = ld4(p, L.at(px + 3 * ps));
            add(v0); add(v1); add(v2); add(v3);
        }
        for (; px < W; px += ps) add(ld4(p, L.at(px)));
    }
    bn_block_reduce(a, red, part + (size_t)blockIdx.x * 2 * C, L.cw, C, 4 * (int)blockIdx.y * L.cw);
}

// the chunks' partials of BN_FIN_CH channels, both quantities: 32 slices (chunk % 32) in chunk order each, then the slices in order;
// four chunks' loads are requested before the first is added (the additions stay in chunk order).
// STATS: mean = K + s1 / n, var = (s2 - s1^2 / n) / n; else out[c] = s1, out[C + c] = s2.
template <bool STATS>
__global__ __launch_bounds__(BN_THREADS) void bn_finish_kernel(const double* __restrict__ part, int nchunks, int C, double n,
                                                               const float* __restrict__ pivot, double* __restrict__ out0,
                                                               double* __restrict__ out1) {
    __shared__ double red[2][BN_THREADS];
    const int t = threadIdx.x, cl = t % BN_FIN_CH, sl = t / BN_FIN_CH, c = blockIdx.x * BN_FIN_CH + cl;
    constexpr int SL = BN_THREADS / BN_FIN_CH;
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        int k = sl;
        for (; k + 3 * SL < nchunks; k += 4 * SL) {
            double u[4], v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                u[i] = part[(size_t)(k + i * SL) * 2 * C + c];
                v[i] = part[(size_t)(k + i * SL) * 2 * C + C + c];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s1 += u[i];
                s2 += v[i];
            }
        }
        for (; k < nchunks; k += SL) {
            s1 += part[(size_t)k * 2 * C + c];
            s2 += part[(size_t)k * 2 * C + C + c];
        }
    }
    red[0][t] = s1;
    red[1][t] = s2;
    __syncthreads();
    if (sl != 0 || c >= C) return;
    s1 = 0.0;
    s2 = 0.0;
    for (int k = 0; k < SL; ++k) {
        s1 += red[0][k * BN_FIN_CH + cl];
        s2 += red[1][k * BN_FIN_CH + cl];
    }
    if (STATS) {
        const double v = (s2 - s1 * s1 / n) / n;
        out0[c] = (double)pivot[c] + s1 / n;
        out1[c] = v > 0.0 ? v : 0.0;
    } else {
        out0[c] = s1;
        out1[c] = s2;
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_fold_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                             double* __restrict__ invstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, double eps, double momentum, double n,
                                                             float* __restrict__ scale, float* __restrict__ shift,
                                                             float* __restrict__ running_mean, float* __restrict__ running_var,
                                                             long long* __restrict__ tracked, int C) {
    const int c = blockIdx.x * BN_THREADS + threadIdx.x;
    if (c == 0 && tracked) *tracked += 1;
    if (c >= C) return;
    const double m = mean[c];
    double is;
    if (var) {
        is = 1.0 / sqrt(var[c] + eps);
        invstd[c] = is;
    } else {
        is = invstd[c];
    }
    const double sc = (double)gamma[c] * is;
    scale[c] = (float)sc;
    shift[c] = (float)((double)beta[c] - m * sc);
    if (running_mean) {
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * m);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var[c] * (n / (n - 1.0))));
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_apply_kernel(const float* z, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, const float* residual, float* y, int B,
                                                              int H, int W, int C, int zpad, int ypad, int relu) {
    const BnLane L(C);
    const int ps = L.pstep;
    const long R = (long)B * H;
    const float4 sc = ld4(scale, L.c4), sh = ld4(shift, L.c4);
    auto act = [&](const float4& a, const float4& r) {
        float4 v = make_float4(a.x * sc.x + sh.x + r.x, a.y * sc.y + sh.y + r.y, a.z * sc.z + sh.z + r.z, a.w * sc.w + sh.w + r.w);
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        return v;
    };
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long r = blockIdx.x; r < R; r += gridDim.x) {
        const float* pz = z + bn_row_base(r, H, W, C, zpad);
        const size_t yo = bn_row_base(r, H, W, C, ypad);
        const float* pr = residual ? residual + yo : nullptr;
        float4* py = reinterpret_cast<float4*>(y + yo);
        int px = L.p0;
        for (; px + 3 * ps < W; px += 4 * ps) {
            float4 a[4], rr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = ld4(pz, L.at(px + u * ps));
#pragma unroll
            for (int u = 0; u < 4; ++u) rr[u] = pr ? ld4(pr, L.at(px + u * ps)) : zero;
#pragma unroll
            for (int u = 0; u < 4; ++u) py[L.at(px + u * ps)] = act(a[u], rr[u]);
        }
        for (; px < W; px += ps) py[L.at(px)] = act(ld4(pz, L.at(px)), pr ? ld4(pr, L.at(px)) : zero);
    }
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_sums_kernel(float* __restrict__ g, const float* __restrict__ z,
                                                                 const float* __restrict__ y, const double* __restrict__ mean,
                                                                 const double* __restrict__ invstd, double* __restrict__ part, int B, int H,
                                                                 int W, int C, int gpad, int zpad, int ypad, int nchunks) {
    __shared__ double red[8 * BN_THREADS];
    const BnLane L(C);
    const int ps = L.pstep, c = 4 * L.c4;
    const long R = (long)B * H;
    const long r0 = (long)blockIdx.x * R / nchunks, r1 = ((long)blockIdx.x + 1) * R / nchunks;
    const double m0 = mean[c], m1 = mean[c + 1], m2 = mean[c + 2], m3 = mean[c + 3];
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    auto add = [&](const float4& gv, const float4& zv) {
        a[0] += (double)gv.x; a[1] += (double)gv.y; a[2] += (double)gv.z; a[3] += (double)gv.w;
        a[4] = fma((double)gv.x, (double)zv.x - m0, a[4]);
        a[5] = fma((double)gv.y, (double)zv.y - m1, a[5]);
        a[6] = fma((double)gv.z, (double)zv.z - m2, a[6]);
        a[7] = fma((double)gv.w, (double)zv.w - m3, a[7]);
    };
    auto gate = [](float4 gv, const float4& yv) {
        gv.x = yv.x > 0.f ? gv.x : 0.f; gv.y = yv.y > 0.f ? gv.y : 0.f; gv.z = yv.z > 0.f ? gv.z : 0.f; gv.w = yv.w > 0.f ? gv.w : 0.f;
        return gv;
    };
    for (long r = r0; r < r1; ++r) {
        float* pg = g + bn_row_base(r, H, W, C, gpad);
        const float* pz = z + bn_row_base(r, H, W, C, zpad);
        const float* py = y ? y + bn_row_base(r, H, W, C, ypad) : nullptr;
        int px = L.p0;
        for (; px + 3 * ps < W; px += 4 * ps) {
            float4 gv[4], zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) gv[u] = ld4(pg, L.at(px + u * ps));
#pragma unroll
            for (int u = 0; u < 4; ++u) zv[u] = ld4(pz, L.at(px + u * ps));
            if (py) {
                float4 yv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) yv[u] = ld4(py, L.at(px + u * ps));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    gv[u] = gate(gv[u], yv[u]);
                    reinterpret_cast<float4*>(pg)[L.at(px + u * ps)] = gv[u];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) add(gv[u], zv[u]);
        }
        for (; px < W; px += ps) {
            float4 gv = ld4(pg, L.at(px));
            const float4 zv = ld4(pz, L.at(px));
            if (py) {
                gv = gate(gv, ld4(py, L.at(px)));
                reinterpret_cast<float4*>(pg)[L.at(px)] = gv;
            }
            add(gv, zv);
        }
    }
    // sum g (z - mean) -> sum g zhat: one multiplication per lane instead of one per element
    a[4] *= invstd[c]; a[5] *= invstd[c + 1]; a[6] *= invstd[c + 2]; a[7] *= invstd[c + 3];
    bn_block_reduce(a, red, part + (size_t)blockIdx.x * 2 * C, L.cw, C, 4 * (int)blockIdx.y * L.cw);
}

__global__ __launch_bounds__(BN_THREADS) void bn_bwd_dz_kernel(const float* __restrict__ g, const float* __restrict__ z,
                                                               const double* __restrict__ mean, const double* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const double* __restrict__ sums,
                                                               float* __restrict__ dz, int B, int H, int W, int C, int gpad, int zpad,
                                                               int dpad, double inv_n) {
    const BnLane L(C);
    const int ps = L.pstep;
    const long R = (long)B * H;
    double m[4], sc[4], k1[4], k2[4];                  // dz = sc (g - k1 - (z - mean) k2), k1 = d beta / n, k2 = d gamma invstd / n
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * L.c4 + i;
        m[i] = mean[c];
        sc[i] = (double)gamma[c] * invstd[c];
        k1[i] = sums[c] * inv_n;
        k2[i] = sums[C + c] * invstd[c] * inv_n;
    }
    auto one = [&](const float4& gv, const float4& zv) {
        return make_float4((float)(sc[0] * ((double)gv.x - k1[0] - ((double)zv.x - m[0]) * k2[0])),
                           (float)(sc[1] * ((double)gv.y - k1[1] - ((double)zv.y - m[1]) * k2[1])),
                           (float)(sc[2] * ((double)gv.z - k1[2] - ((double)zv.z - m[2]) * k2[2])),
                           (float)(sc[3] * ((double)gv.w - k1[3] - ((double)zv.w - m[3]) * k2[3])));
    };
    for (long r = blockIdx.x; r < R; r += gridDim.x) {
        const float* pg = g + bn_row_base(r, H, W, C, gpad);
        const float* pz = z + bn_row_base(r, H, W, C, zpad);
        float4* pd = reinterpret_cast<float4*>(dz + bn_row_base(r, H, W, C, dpad));
        int px = L.p0;
        for (; px + 3 * ps < W; px += 4 * ps) {
            float4 gv[4], zv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) gv[u] = ld4(pg, L.at(px + u * ps));
#pragma unroll
            for (int u = 0; u < 4; ++u) zv[u] = ld4(pz, L.at(px + u * ps));
#pragma unroll
            for (int u = 0; u < 4; ++u) pd[L.at(px + u * ps)] = one(gv[u], zv[u]);
        }
        for (; px < W; px += ps) pd[L.at(px)] = one(ld4(pg, L.at(px)), ld4(pz, L.at(px)));
    }
}

// C a multiple of 4 with 256 % (C / 4) == 0 (4, 8, ..., 1024: a lane stays on its channels) or a multiple of 1024 (windows of 1024
// channels, at most 64 of them), W C / 4 and B H W below 2^31
bool bn_geometry(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 4 || C % 4 != 0 || C > 65536) return false;
    if (BN_THREADS % (C / 4) != 0 && C % (4 * BN_THREADS) != 0) return false;
    return (long)W * (C / 4) < (1L << 31) && (long)B * H * W < (1L << 31);
}

unsigned bn_windows(int C) { return C > 4 * BN_THREADS ? (unsigned)(C / (4 * BN_THREADS)) : 1u; }

dim3 bn_grid(int B, int H, int C) { return dim3((unsigned)bn_chunks((long)B * H), bn_windows(C)); }

}  // namespace
}  // namespace hps

using namespace hps;

static const char* BN_GEOMETRY = "geometry (B, H, W >= 1; C = 4, 8, 16, ..., 1024 or a multiple of 1024; pads >= 0; B H W < 2^31)";

extern "C" size_t hps_bn_batch_stats_workspace(int B, int H, int W, int C) {
    if (!bn_geometry(B, H, W, C)) return 0;
    return (size_t)bn_chunks((long)B * H) * 2 * C * sizeof(double);
}

extern "C" int hps_bn_batch_stats(const float* z, double* workspace, double* mean, double* var, int B, int H, int W, int C, int pad,
                                  hps_stream_t stream) {
    if (!z || !workspace || !mean || !var) return bad_arg("hps_bn_batch_stats: null pointer");
    if (!bn_geometry(B, H, W, C) || pad < 0) return bad_arg(BN_GEOMETRY);
    hipStream_t s = (hipStream_t)stream;
    const int nchunks = bn_chunks((long)B * H);
    bn_stats_kernel<<<dim3(nchunks, bn_windows(C)), BN_THREADS, 0, s>>>(z, workspace, B, H, W, C, pad, nchunks);
    // the pivots: the first interior pixel of the frame
    const float* pivot = z + ((size_t)pad * (W + 2 * pad) + pad) * C;
    bn_finish_kernel<true><<<ceil_div(C, BN_FIN_CH), BN_THREADS, 0, s>>>(workspace, nchunks, C, (double)B * H * W, pivot, mean, var);
    return check_launch("hps_bn_batch_stats");
}

extern "C" int hps_bn_train_fold(const double* mean, const double* var, double* invstd, const float* gamma, const float* beta, double eps,
                                 double momentum, long long n, float* scale, float* shift, float* running_mean, float* running_var,
                                 long long* num_batches_tracked, int C, hps_stream_t stream) {
    if (!mean || !invstd || !gamma || !beta || !scale || !shift) return bad_arg("hps_bn_train_fold: null pointer");
    if (C < 1 || n < 1) return bad_arg("hps_bn_train_fold: C >= 1 and n >= 1 required");
    if ((running_mean != nullptr) != (running_var != nullptr)) return bad_arg("hps_bn_train_fold: running_mean and running_var go together");
    if (running_mean && (!var || n < 2)) return bad_arg("hps_bn_train_fold: the running update needs var and n >= 2");
    if (num_batches_tracked && !running_mean) return bad_arg("hps_bn_train_fold: a counter without running buffers");
    bn_fold_kernel<<<ceil_div(C, BN_THREADS), BN_THREADS, 0, (hipStream_t)stream>>>(mean, var, invstd, gamma, beta, eps, momentum, (double)n,
                                                                                   scale, shift, running_mean, running_var,
                                                                                   num_batches_tracked, C);
    return check_launch("hps_bn_train_fold");
}

extern "C" int hps_bn_apply_act_pad(const float* z, const float* scale, const float* shift, const float* residual, float* y, int B, int H,
                                    int W, int C, int zpad, int ypad, int relu, hps_stream_t stream) {
    if (!z || !scale || !shift || !y) return bad_arg("hps_bn_apply_act_pad: null pointer");
    if (!bn_geometry(B, H, W, C) || zpad < 0 || ypad < 0) return bad_arg(BN_GEOMETRY);
    if (z == y && zpad != ypad) return bad_arg("hps_bn_apply_act_pad: in place needs zpad == ypad");
    bn_apply_kernel<<<bn_grid(B, H, C), BN_THREADS, 0, (hipStream_t)stream>>>(z, scale, shift, residual, y, B, H, W, C, zpad, ypad, relu);
    return check_launch("hps_bn_apply_act_pad");
}

extern "C" size_t hps_bn_train_backward_sums_workspace(int B, int H, int W, int C) { return hps_bn_batch_stats_workspace(B, H, W, C); }

extern "C" int hps_bn_train_backward_sums(float* g, const float* z, const float* y, const double* mean, const double* invstd,
                                          double* workspace, double* sums, int B, int H, int W, int C, int gpad, int zpad, int ypad,
                                          hps_stream_t stream) {
    if (!g || !z || !mean || !invstd || !workspace || !sums) return bad_arg("hps_bn_train_backward_sums: null pointer");
    if (!bn_geometry(B, H, W, C) || gpad < 0 || zpad < 0 || ypad < 0) return bad_arg(BN_GEOMETRY);
    hipStream_t s = (hipStream_t)stream;
    const int nchunks = bn_chunks((long)B * H);
    bn_bwd_sums_kernel<<<dim3(nchunks, bn_windows(C)), BN_THREADS, 0, s>>>(g, z, y, mean, invstd, workspace, B, H, W, C, gpad, zpad, ypad, nchunks);
    bn_finish_kernel<false><<<ceil_div(C, BN_FIN_CH), BN_THREADS, 0, s>>>(workspace, nchunks, C, 1.0, nullptr, sums, sums + C);
    return check_launch("hps_bn_train_backward_sums");
}

extern "C" int hps_bn_train_backward_dz(const float* g, const float* z, const double* mean, const double* invstd, const float* gamma,
                                        const double* sums, float* dz, int B, int H, int W, int C, int gpad, int zpad, int dpad,
                                        hps_stream_t stream) {
    if (!g || !z || !mean || !invstd || !gamma || !sums || !dz) return bad_arg("hps_bn_train_backward_dz: null pointer");
    if (!bn_geometry(B, H, W, C) || gpad < 0 || zpad < 0 || dpad < 0) return bad_arg(BN_GEOMETRY);
    if (dz == g || dz == z) return bad_arg("hps_bn_train_backward_dz: out of place only (the gated cotangent has other readers)");
    bn_bwd_dz_kernel<<<bn_grid(B, H, C), BN_THREADS, 0, (hipStream_t)stream>>>(g, z, mean, invstd, gamma, sums, dz, B, H, W, C, gpad, zpad, dpad,
                                                                           1.0 / ((double)B * H * W));
    return check_launch("hps_bn_train_backward_dz");
}
