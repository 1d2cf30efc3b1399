// Matrix-Fisher negative log-likelihood and the pose / shape training loss (losses/matrix_fisher_loss.py): the log normalising
// constant log c(S) and its gradient (:134-192), matrix_fisher_nll (:195-228) and PoseMFShapeGaussianLoss (:231-301).
//
// The reference evaluates c_bar(S) and the three gradient integrals as (rows x 512) temporaries, with a boolean-mask gather per
// Bessel evaluation (a host round trip each on a GPU) and torch.det(...).cpu() for the proper-SVD sign.  Here one wave64 owns a
// row: every lane evaluates 8 of the 512 trapezoid nodes for all four integrands in one pass and the sums meet in a butterfly
// of shuffles.  The row arithmetic is fp64 -- the fp32 results must be no further from the fp64 reference than the reference's
// own fp32 evaluation is, which an fp32 evaluation of the same rule does not guarantee -- and every output is rounded once.
#include "hps_common.h"

namespace hps {

constexpr int MF_NODES = 512;             // num_traps of the reference's trapezoid rule (:157, :180), end weights 1/2
constexpr int MF_NODES_PER_LANE = MF_NODES / 64;
constexpr int MF_ROWS_PER_BLOCK = 4;      // one wave64 per row, 256-thread workgroups
constexpr int MF_EW_BLOCKS = 512;         // workgroups of the elementwise loss terms (grid-stride, a fixed count: fixed summation order)
constexpr int MF_SLOTS = 8;               // per-workgroup partial sums: pose, shape, joints2D, glob, verts, joints3D, selected count, 0
constexpr int MF_BW_ROWS = 256;           // backward: one thread per pose row

// I0(x) / exp(|x|) by the Numerical Recipes polynomials (:9-11, :30-45), both branches split at |x| <= 3.75.  The large-|x| branch
// is never evaluated at x = 0 (it divides by zero there; the reference masks that value away).
__device__ __forceinline__ double i0_exp_scaled(double x) {
    const double ax = fabs(x);
    if (ax <= 3.75) {
        const double t = ax / 3.75;
        const double y = t * t;
        double z = 0.45813e-2;
        z = z * y + 0.360768e-1;
        z = z * y + 0.2659732;
        z = z * y + 1.2067492;
        z = z * y + 3.0899424;
        z = z * y + 3.5156229;
        z = z * y + 1.0;
        return z / exp(ax);
    }
    const double y = 3.75 / ax;
    double z = 0.392377e-2;
    z = z * y + -0.1647633e-1;
    z = z * y + 0.2635537e-1;
    z = z * y + -0.2057706e-1;
    z = z * y + 0.916281e-2;
    z = z * y + -0.157565e-2;
    z = z * y + 0.225319e-2;
    z = z * y + 0.1328592e-1;
    z = z * y + 0.39894228;
    return z / sqrt(ax);
}

// The gradient integrand of one cyclic shift (s_k, s_a, s_b) of the singular values (:99-131): s_i = max, s_j = min of (s_a, s_b).
__device__ __forceinline__ double mf_shift_integrand(double sk, double sa, double sb, double u) {
    const double si = fmax(sa, sb), sj = fmin(sa, sb);
    return i0_exp_scaled((si - sj) * 0.5 * (1.0 - u)) * i0_exp_scaled((si + sj) * 0.5 * (1.0 + u)) * exp((sj + sk) * (u - 1.0)) * u;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;                                     // butterfly: every lane holds the same bits
}

// One row's normalising constant, wave-cooperative (all 64 lanes call it with the same s).  c_bar = c(S) / exp(tr S) (:159-163);
// with GRAD, dlogc[k] = d log c / d s_k = (1/2) integral_k / c_bar (:182-190).
struct MfRow {
    double c_bar;
    double dlogc[3];
};

template <bool GRAD>
__device__ __forceinline__ MfRow mf_row(double s0, double s1, double s2, int lane) {
    const double h = 2.0 / (MF_NODES - 1);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
    for (int q = 0; q < MF_NODES_PER_LANE; ++q) {
        const int k = q * 64 + lane;
        const double u = (double)k * h + -1.0;
        const double w = (k == 0 || k == MF_NODES - 1) ? 0.5 : 1.0;
        acc[0] += i0_exp_scaled((s1 - s2) * 0.5 * (1.0 - u)) * i0_exp_scaled((s1 + s2) * 0.5 * (1.0 + u)) * exp((s2 + s0) * (u - 1.0)) * w;
        if (GRAD) {
            acc[1] += mf_shift_integrand(s0, s1, s2, u) * w;
            acc[2] += mf_shift_integrand(s1, s2, s0, u) * w;
            acc[3] += mf_shift_integrand(s2, s0, s1, u) * w;
        }
    }
    MfRow r;
    r.c_bar = 0.5 * (wave_sum(acc[0]) * h);
    if (GRAD) {
#pragma unroll
        for (int k = 0; k < 3; ++k) r.dlogc[k] = 0.5 * (wave_sum(acc[1 + k]) * h) / r.c_bar;
    }
    return r;
}

__device__ __forceinline__ double log_c_of(const MfRow& r, double s0, double s1, double s2) { return log(r.c_bar) + (s0 + s1 + s2); }

// det(U V^T) in fp64 (:222: the determinant's VALUE multiplies s3, as in the reference)
__device__ __forceinline__ double det_uvt(const float* __restrict__ u, const float* __restrict__ v) {
    double m[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            m[i * 3 + j] = (double)u[i * 3 + 0] * v[j * 3 + 0] + (double)u[i * 3 + 1] * v[j * 3 + 1] + (double)u[i * 3 + 2] * v[j * 3 + 2];
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// One row of matrix_fisher_nll (:221-228), wave-cooperative.  Returns the NLL; with GRAD also d log c / d s_proper and det.
template <bool GRAD>
__device__ __forceinline__ double mf_nll_row(const float* __restrict__ F, const float* __restrict__ U, const float* __restrict__ S,
                                             const float* __restrict__ V, const float* __restrict__ R, long row, double overreg,
                                             int lane, double* dlogc, double* det_out) {
    const double det = det_uvt(U + row * 9, V + row * 9);
    const double s0 = S[row * 3 + 0], s1 = S[row * 3 + 1], s2 = (double)S[row * 3 + 2] * det;
    const MfRow r = mf_row<GRAD>(s0, s1, s2, lane);
    if (GRAD) {
        dlogc[0] = r.dlogc[0];
        dlogc[1] = r.dlogc[1];
        dlogc[2] = r.dlogc[2];
        *det_out = det;
    }
    double fr = 0.0;                                              // <F, R> = tr(F^T R)
#pragma unroll
    for (int e = 0; e < 9; ++e) fr += (double)F[row * 9 + e] * R[row * 9 + e];
    return -fr + overreg * log_c_of(r, s0, s1, s2);
}

template <bool GRAD>
__global__ __launch_bounds__(256) void mf_log_norm_const_kernel(const float* __restrict__ S, int n, float* __restrict__ log_c,
                                                                 const float* __restrict__ grad_log_c, float* __restrict__ grad_S) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MF_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;                         // whole waves; the kernel has no barrier
    const double s0 = S[row * 3 + 0], s1 = S[row * 3 + 1], s2 = S[row * 3 + 2];
    const MfRow r = mf_row<GRAD>(s0, s1, s2, lane);
    if (lane != 0) return;
    if (log_c) log_c[row] = (float)log_c_of(r, s0, s1, s2);
    if (GRAD) {
        const double g = grad_log_c[row];
#pragma unroll
        for (int k = 0; k < 3; ++k) grad_S[row * 3 + k] = (float)(r.dlogc[k] * g);
    }
}

template <bool GRAD>
__global__ __launch_bounds__(256) void mf_nll_kernel(const float* __restrict__ F, const float* __restrict__ U, const float* __restrict__ S,
                                                      const float* __restrict__ V, const float* __restrict__ R, int n, double overreg,
                                                      float* __restrict__ nll, const float* __restrict__ grad_nll,
                                                      float* __restrict__ grad_F, float* __restrict__ grad_S) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MF_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= n) return;                         // whole waves; the kernel has no barrier
    double dlogc[3] = {0.0, 0.0, 0.0}, det = 1.0;
    const double v = mf_nll_row<GRAD>(F, U, S, V, R, row, overreg, lane, dlogc, &det);
    if (nll && lane == 0) nll[row] = (float)v;
    if (!GRAD) return;
    const double g = grad_nll[row];
    if (grad_F && lane < 9) grad_F[row * 9 + lane] = (float)(-((double)R[row * 9 + lane] * g));
    if (grad_S && lane < 3) {
        const double gs = dlogc[lane] * (overreg * g);           // d nll / d log c = overreg; the s3 entry through s3 * det
        grad_S[row * 3 + lane] = (float)(lane == 2 ? gs * det : gs);
    }
}

// ---- PoseMFShapeGaussianLoss (:231-301) ----
// workspace: [rows x 4 doubles: dlogc (3), det] [workgroups x MF_SLOTS partial doubles] [MF_SLOTS doubles: six terms, selected count, total]
struct MfLossWs {
    double* row;
    double* partial;
    double* fin;
};

__host__ __device__ inline int mf_pose_blocks(long rows) { return (int)((rows + MF_ROWS_PER_BLOCK - 1) / MF_ROWS_PER_BLOCK); }

inline MfLossWs mf_loss_ws(void* base, long rows) {
    MfLossWs w;
    w.row = static_cast<double*>(base);
    w.partial = w.row + rows * 4;
    w.fin = w.partial + (long)(mf_pose_blocks(rows) + MF_EW_BLOCKS) * MF_SLOTS;
    return w;
}

int64_t mf_loss_ws_bytes(int64_t rows) {
    return (int64_t)sizeof(double) * (rows * 4 + (int64_t)(mf_pose_blocks(rows) + MF_EW_BLOCKS) * MF_SLOTS + MF_SLOTS);
}

// Workgroup sums of NV doubles in a fixed order (wave butterflies, then the four waves in order); the result is valid in thread 0.
// Every thread of the workgroup calls it.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV]) {
    __shared__ double red[4][NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// Launch 1: workgroups [0, pose blocks) -- one pose row per wave: the row's NLL, its dlogc and det kept for backward; the others:
// grid-stride partial sums of the five elementwise terms and the number of selected joints2D entries.
__global__ __launch_bounds__(256) void mf_loss_partial_kernel(const hps_mf_loss_args a, MfLossWs ws) {
    const long rows = a.n_pose;
    const int pose_blocks = mf_pose_blocks(rows);
    double* out = ws.partial + (long)blockIdx.x * MF_SLOTS;
    if ((int)blockIdx.x < pose_blocks) {          // workgroup-uniform branch: every thread reaches block_sum's barrier
        const int lane = threadIdx.x & 63;
        const long row = (long)blockIdx.x * MF_ROWS_PER_BLOCK + (threadIdx.x >> 6);
        double v[1] = {0.0};
        if (row < rows) {
            double dlogc[3], det = 1.0;
            const double nll = mf_nll_row<true>(a.pose_F, a.pose_U, a.pose_S, a.pose_V, a.t_pose_rotmats, row, a.overreg, lane, dlogc, &det);
            if (lane < 3) ws.row[row * 4 + lane] = dlogc[lane];
            if (lane == 3) ws.row[row * 4 + 3] = det;
            if (lane == 0) v[0] = nll;
        }
        block_sum<1>(v);
        if (threadIdx.x == 0) {
            out[0] = v[0];
            for (int k = 1; k < MF_SLOTS; ++k) out[k] = 0.0;
        }
        return;
    }
    const long tid = (long)(blockIdx.x - pose_blocks) * 256 + threadIdx.x, stride = (long)MF_EW_BLOCKS * 256;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // shape, joints2D, glob, verts, joints3D, selected joints2D entries
    // shape: -log N(t; loc, scale), torch.distributions.Normal.log_prob: -(t - loc)^2 / (2 scale^2) - log scale - log sqrt(2 pi)
    const double log_sqrt_2pi = 0.91893853320467274178;
    for (long i = tid; i < a.n_shape; i += stride) {
        const double sc = a.shape_scale[i], z = (double)a.t_shape[i] - a.shape_loc[i];
        v[0] -= -(z * z) / (2.0 * (sc * sc)) - log(sc) - log_sqrt_2pi;
    }
    // joints2D: the entries of visible joints, every sample against the image's target normalised by 2 t / img_wh - 1 (:277-283)
    const long nj2 = a.j2d_B * a.Ns * a.K;
    for (long i = tid; i < nj2; i += stride) {
        const long b = i / (a.Ns * a.K), j = i % a.K;
        if (a.t_joints2d_vis[b * a.K + j]) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const double t = (2.0 * a.t_joints2d[(b * a.K + j) * 2 + c]) / a.img_wh - 1.0;
                const double d = (double)a.joints2d[i * 2 + c] - t;
                v[1] += d * d;
            }
            v[5] += 2.0;
        }
    }
    for (long i = tid; i < a.n_glob; i += stride) {
        const double d = (double)a.glob_rotmats[i] - a.t_glob_rotmats[i];
        v[2] += d * d;
    }
    for (long i = tid; i < a.n_verts; i += stride) {
        const double d = (double)a.verts[i] - a.t_verts[i];
        v[3] += d * d;
    }
    for (long i = tid; i < a.n_joints3d; i += stride) {
        const double d = (double)a.joints3d[i] - a.t_joints3d[i];
        v[4] += d * d;
    }
    block_sum<6>(v);
    if (threadIdx.x == 0) {
        out[0] = 0.0;
        for (int k = 0; k < 6; ++k) out[1 + k] = v[k];
        out[7] = 0.0;
    }
}

// Launch 2: one workgroup adds the partials in a fixed order, applies REDUCTION to every term and writes the weighted total.
__global__ __launch_bounds__(256) void mf_loss_finish_kernel(const hps_mf_loss_args a, MfLossWs ws, float* __restrict__ total) {
    const int nblocks = mf_pose_blocks(a.n_pose) + MF_EW_BLOCKS;
    double v[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nblocks; b += 256)
#pragma unroll
        for (int k = 0; k < 7; ++k) v[k] += ws.partial[(long)b * MF_SLOTS + k];
    block_sum<7>(v);
    if (threadIdx.x != 0) return;
    const bool mean = a.reduction == HPS_MF_REDUCTION_MEAN;
    const double count = v[6];
    double term[6];                                                          // a mean over no element is 0 / 0 = NaN, as in torch
    term[0] = mean ? v[0] / (double)a.n_pose : v[0];
    term[1] = mean ? v[1] / (double)a.shape_B : v[1];                        // mean over the batch of the per-item sum over betas
    term[2] = mean ? v[2] / count : v[2];
    term[3] = mean ? v[3] / (double)a.n_glob : v[3];
    term[4] = mean ? v[4] / (double)a.n_verts : v[4];
    term[5] = mean ? v[5] / (double)a.n_joints3d : v[5];
    double t = term[0] * a.weights[0];
    for (int k = 1; k < 6; ++k) t = t + term[k] * a.weights[k];              // (:294-299) left to right; 0 * NaN stays NaN
    for (int k = 0; k < 6; ++k) ws.fin[k] = term[k];
    ws.fin[6] = count;
    ws.fin[7] = t;
    *total = (float)t;
}

// The backward launch: d total / d (every prediction) scaled by grad_total[0], from the workspace of the forward call.
__global__ __launch_bounds__(256) void mf_loss_backward_kernel(const hps_mf_loss_args a, MfLossWs ws, const float* __restrict__ grad_total) {
    const long rows = a.n_pose;
    const int pose_blocks = (int)((rows + MF_BW_ROWS - 1) / MF_BW_ROWS);
    const double g = grad_total[0];
    const bool mean = a.reduction == HPS_MF_REDUCTION_MEAN;
    if ((int)blockIdx.x < pose_blocks) {          // no barrier in this kernel
        const long row = (long)blockIdx.x * MF_BW_ROWS + threadIdx.x;
        if (row >= rows) return;
        const double gr = mean ? (g * a.weights[0]) / (double)rows : g * a.weights[0];
        if (a.g_pose_F)
#pragma unroll
            for (int e = 0; e < 9; ++e) a.g_pose_F[row * 9 + e] = (float)(-((double)a.t_pose_rotmats[row * 9 + e] * gr));
        if (a.g_pose_S) {
            const double gl = a.overreg * gr;
            const double* w = ws.row + row * 4;
            a.g_pose_S[row * 3 + 0] = (float)(w[0] * gl);
            a.g_pose_S[row * 3 + 1] = (float)(w[1] * gl);
            a.g_pose_S[row * 3 + 2] = (float)((w[2] * gl) * w[3]);
        }
        return;
    }
    const long tid = (long)(blockIdx.x - pose_blocks) * 256 + threadIdx.x, stride = (long)MF_EW_BLOCKS * 256;
    const double gs = mean ? (g * a.weights[1]) / (double)a.shape_B : g * a.weights[1];
    for (long i = tid; i < a.n_shape; i += stride) {
        const double sc = a.shape_scale[i], z = (double)a.t_shape[i] - a.shape_loc[i];
        if (a.g_shape_loc) a.g_shape_loc[i] = (float)(gs * (-(z / (sc * sc))));
        if (a.g_shape_scale) a.g_shape_scale[i] = (float)(gs * (1.0 / sc - (z * z) / (sc * sc * sc)));
    }
    // MSE: d/dp = (2 / n) (p - t) g w, n = 1 for 'sum'; joints2D entries of invisible joints get 0
    if (a.g_joints2d) {
        const double c2 = mean ? 2.0 / ws.fin[6] : 2.0, gw = g * a.weights[2];
        const long nj2 = a.j2d_B * a.Ns * a.K;
        for (long i = tid; i < nj2; i += stride) {
            const long b = i / (a.Ns * a.K), j = i % a.K;
            const bool vis = a.t_joints2d_vis[b * a.K + j] != 0;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                float gv = 0.0f;
                if (vis) {
                    const double t = (2.0 * a.t_joints2d[(b * a.K + j) * 2 + c]) / a.img_wh - 1.0;
                    gv = (float)(c2 * ((double)a.joints2d[i * 2 + c] - t) * gw);
                }
                a.g_joints2d[i * 2 + c] = gv;
            }
        }
    }
    const float* const p[3] = {a.glob_rotmats, a.verts, a.joints3d};
    const float* const t[3] = {a.t_glob_rotmats, a.t_verts, a.t_joints3d};
    float* const gout[3] = {a.g_glob_rotmats, a.g_verts, a.g_joints3d};
    const long n[3] = {a.n_glob, a.n_verts, a.n_joints3d};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        if (!gout[m]) continue;
        const double c2 = mean ? 2.0 / (double)n[m] : 2.0, gw = g * a.weights[3 + m];
        for (long i = tid; i < n[m]; i += stride) gout[m][i] = (float)(c2 * ((double)p[m][i] - t[m][i]) * gw);
    }
}

static int check_loss_args(const hps_mf_loss_args* a, const void* ws, const char* who) {
    if (!a || !ws) {
        set_error("bad argument: %s: null pointer", who);
        return HPS_E_BADARG;
    }
    if (a->struct_bytes != (int)sizeof(hps_mf_loss_args)) {
        set_error("bad argument: %s: struct_bytes %d != sizeof(hps_mf_loss_args) %d", who, a->struct_bytes, (int)sizeof(hps_mf_loss_args));
        return HPS_E_BADARG;
    }
    if (!a->pose_F || !a->pose_U || !a->pose_S || !a->pose_V || !a->shape_loc || !a->shape_scale || !a->joints2d || !a->glob_rotmats ||
        !a->verts || !a->joints3d || !a->t_pose_rotmats || !a->t_shape || !a->t_joints2d || !a->t_joints2d_vis || !a->t_glob_rotmats ||
        !a->t_verts || !a->t_joints3d) {
        set_error("bad argument: %s: null pointer", who);
        return HPS_E_BADARG;
    }
    if (a->n_pose < 0 || a->shape_B < 0 || a->n_shape < 0 || a->j2d_B < 0 || a->Ns < 0 || a->K < 0 || a->n_glob < 0 || a->n_verts < 0 ||
        a->n_joints3d < 0 || a->n_pose > (1 << 28)) {
        set_error("bad argument: %s: size out of range", who);
        return HPS_E_BADARG;
    }
    if (a->reduction != HPS_MF_REDUCTION_MEAN && a->reduction != HPS_MF_REDUCTION_SUM) {
        set_error("bad argument: %s: reduction %d (HPS_MF_REDUCTION_MEAN or _SUM)", who, a->reduction);
        return HPS_E_BADARG;
    }
    if ((reinterpret_cast<uintptr_t>(ws) & 7) != 0) {
        set_error("bad argument: %s: workspace not 8-byte aligned", who);
        return HPS_E_BADARG;
    }
    return HPS_OK;
}

}  // namespace hps

using namespace hps;

extern "C" int hps_mf_log_norm_const(const float* S, int n, float* log_c, const float* grad_log_c, float* grad_S, hps_stream_t stream) {
    if (!S || (!log_c && !grad_S)) return bad_arg("hps_mf_log_norm_const: null pointer");
    if (!grad_S != !grad_log_c) return bad_arg("hps_mf_log_norm_const: null pointer (grad_log_c and grad_S go together)");
    if (n < 0) return bad_arg("hps_mf_log_norm_const: n < 0");
    if (n == 0) return HPS_OK;
    const dim3 grid(ceil_div(n, MF_ROWS_PER_BLOCK));
    if (grad_S)
        hipLaunchKernelGGL(mf_log_norm_const_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, S, n, log_c, grad_log_c, grad_S);
    else
        hipLaunchKernelGGL(mf_log_norm_const_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, S, n, log_c, nullptr, nullptr);
    return check_launch("hps_mf_log_norm_const");
}

extern "C" int hps_mf_nll(const float* F, const float* U, const float* S, const float* V, const float* R, int n, double overreg,
                          float* nll, const float* grad_nll, float* grad_F, float* grad_S, hps_stream_t stream) {
    if (!F || !U || !S || !V || !R || (!nll && !grad_F && !grad_S)) return bad_arg("hps_mf_nll: null pointer");
    if ((grad_F || grad_S) && !grad_nll) return bad_arg("hps_mf_nll: null pointer (grad_nll)");
    if (n < 0) return bad_arg("hps_mf_nll: n < 0");
    if (n == 0) return HPS_OK;
    const dim3 grid(ceil_div(n, MF_ROWS_PER_BLOCK));
    if (grad_F || grad_S)
        hipLaunchKernelGGL(mf_nll_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, F, U, S, V, R, n, overreg, nll, grad_nll, grad_F,
                           grad_S);
    else
        hipLaunchKernelGGL(mf_nll_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, F, U, S, V, R, n, overreg, nll, nullptr, nullptr,
                           nullptr);
    return check_launch("hps_mf_nll");
}

extern "C" int hps_mf_loss_forward(const hps_mf_loss_args* a, void* workspace, float* total, hps_stream_t stream) {
    if (const int rc = check_loss_args(a, workspace, "hps_mf_loss_forward")) return rc;
    if (!total) return bad_arg("hps_mf_loss_forward: null pointer");
    const MfLossWs ws = mf_loss_ws(workspace, a->n_pose);
    hipLaunchKernelGGL(mf_loss_partial_kernel, dim3(mf_pose_blocks(a->n_pose) + MF_EW_BLOCKS), dim3(256), 0, (hipStream_t)stream, *a, ws);
    hipLaunchKernelGGL(mf_loss_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, *a, ws, total);
    return check_launch("hps_mf_loss_forward");
}

extern "C" int hps_mf_loss_backward(const hps_mf_loss_args* a, const void* workspace, const float* grad_total, hps_stream_t stream) {
    if (const int rc = check_loss_args(a, workspace, "hps_mf_loss_backward")) return rc;
    if (!grad_total) return bad_arg("hps_mf_loss_backward: null pointer");
    const MfLossWs ws = mf_loss_ws(const_cast<void*>(workspace), a->n_pose);
    const int pose_blocks = (int)((a->n_pose + MF_BW_ROWS - 1) / MF_BW_ROWS);
    hipLaunchKernelGGL(mf_loss_backward_kernel, dim3(pose_blocks + MF_EW_BLOCKS), dim3(256), 0, (hipStream_t)stream, *a, ws, grad_total);
    return check_launch("hps_mf_loss_backward");
}
