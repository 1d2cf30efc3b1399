// Backward of the distribution-prediction head (models/poseMF_shapeGaussian_net.py:95-162) and of rot6d_to_rotmat
// (utils/rigid_transform_utils.py:80-94): the vector-Jacobian products a training step needs (the reference's
// train/train_poseMF_shapeGaussian_net.py:262-349 gets them from torch autograd).
//
// Rules of every kernel here: no floating-point atomics, no host synchronisation, one fixed summation order per output -- results
// are bitwise repeatable; everything that belongs to one image is computed from that image's rows alone with an instruction
// sequence that does not depend on the batch size; sums over the batch run over the images in ascending order.  Reductions are
// accumulated in float64 (the products of two fp32 values are exact there): the whole backward is a few hundred MFLOP of
// latency-bound work, and the summation order then contributes nothing to the error.
#include "hps_common.h"

namespace hps {

constexpr int BW_NT = 256;    // threads per workgroup of the level kernel (four waves, the footprint of joint_level_kernel<128,true,256,4>)
constexpr int BW_TBL = 4;     // images per workgroup
constexpr int BW_HID = 128;   // EMBED_DIM / 2
constexpr int BW_JOINT_TAIL = BW_HID + 9 * BW_HID + 9;   // floats of [g_b1 | g_W2 | g_b2] behind a joint's g_W1

// carve-up of the hps_head_pose_levels_backward workspace; total_in = sum over the joints of in_dim
struct LevelsWs {
    float* gx;   // per joint j a (B, in_dim_j) block at B * in_off[j]: the gradient of the joint's MLP input
    float* xs;   // same layout: the MLP input itself (:126-132), kept for the weight gradient
    float* h;    // (B, NJ, 128) hidden activations
    float* gp;   // (B, NJ, 128) gradient of the hidden pre-activations
    float* gf;   // (B, NJ, 9)   gradient of joint_F
};

int64_t head_levels_backward_ws_bytes(int64_t B, int64_t total_in, int64_t NJ) {
    return B * (2 * total_in + NJ * (2 * BW_HID + 9)) * (int64_t)sizeof(float);
}
int64_t head_trunk_backward_ws_bytes(int64_t B, int64_t wide, int64_t nt) {
    return B * (wide + 2 * nt) * (int64_t)sizeof(float);
}

__device__ __forceinline__ float elu_fwd(float x) { return x > 0.0f ? x : expm1f(x); }
// ELU'(x) from y = ELU(x): 1 for x > 0, exp(x) = y + 1 otherwise
__device__ __forceinline__ float elu_grad_from_out(float y) { return y > 0.0f ? 1.0f : y + 1.0f; }

// Element k of image b's input to joint MLP `joint` (:126-132): cat[embed, U_proper[anc], S_proper[anc], mode[anc]] over the joint's
// P ancestors anc_idx[a_lo ..], the layout of csrc/head.hip's joint_level_body.  One definition for the float64 forward and the backward.
template <typename T>
__device__ __forceinline__ T level_input(const T* __restrict__ embed, int embed_dim, const T* u_proper, const T* s_proper, const T* mode,
                                         const int32_t* __restrict__ anc_idx, int a_lo, int P, size_t b, int NJ, int k) {
    if (k < embed_dim) return embed[b * embed_dim + k];
    int t = k - embed_dim;
    if (t < 9 * P) return u_proper[(b * NJ + anc_idx[a_lo + t / 9]) * 9 + t % 9];
    if (t < 12 * P) { t -= 9 * P; return s_proper[(b * NJ + anc_idx[a_lo + t / 3]) * 3 + t % 3]; }
    t -= 12 * P;
    return mode[(b * NJ + anc_idx[a_lo + t / 9]) * 9 + t % 9];
}

// The hidden layer's sums (:130-132) of BW_TBL images: BW_NT / BW_HID K-slices x BW_HID columns, float64 partial sums of slice ks
// into red[ks][r][n].  xs: the inputs [in_dim][BW_TBL] in LDS (float or double), w1t: the layer's weight transposed (in_dim, BW_HID).
template <typename T>
__device__ __forceinline__ void hidden_slices(const T* xs, const float* __restrict__ w1t, int in_dim, int tid, double* red) {
    const int n = tid % BW_HID, ks = tid / BW_HID;
    const int kchunk = ceil_div(in_dim, BW_NT / BW_HID);
    const int k_lo = min(in_dim, ks * kchunk), k_hi = min(in_dim, k_lo + kchunk);
    const float* w = w1t + n;
    double acc[BW_TBL];
#pragma unroll
    for (int r = 0; r < BW_TBL; ++r) acc[r] = 0.0;
    for (int k = k_lo; k < k_hi; ++k) {
        const double wv = (double)w[(size_t)k * BW_HID];
#pragma unroll
        for (int r = 0; r < BW_TBL; ++r) acc[r] += (double)xs[k * BW_TBL + r] * wv;
    }
#pragma unroll
    for (int r = 0; r < BW_TBL; ++r) red[(ks * BW_TBL + r) * BW_HID + n] = acc[r];
}

// The gradient of joint_F (:130-135) of one joint of one image from the cotangents of everything computed from it (:137-160):
// pose_F, pose_S directly; mode = U_p V_p^T; U_p, S_p, V_p = U, S, V times the constants det U, det V = +-1; and the SVD
// backward of a square matrix with distinct singular values as torch.svd's autograd evaluates it,
//   gF = U [ (E o (U^T gU - gU^T U)) S + S (E o (V^T gV - gV^T V)) + diag(gS) ] V^T,   E_ij = 1 / (s_j^2 - s_i^2), i != j.
// gUp / gSp / gM: what the joint's descendants left on its U_proper / S_proper / mode (gM already includes the caller's).
// gU_raw / gV_raw: the caller's cotangents of the RAW factors pose_U / pose_V (:137; the sampler's, utils/sampling_utils.py:106-111):
// they join gU / gV as they are, with no proper-fix factor.
__device__ __forceinline__ void svd_head_backward(const double* __restrict__ Uf, const double* __restrict__ Sf,
                                                  const double* __restrict__ Vf, double* gUp, const double* gSp, const double* gM,
                                                  const double* gS_raw, const double* gF_direct, const double* gU_raw,
                                                  const double* gV_raw, double* gF) {
    double U[9], V[9], S[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) { U[e] = Uf[e]; V[e] = Vf[e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) S[e] = Sf[e];
    auto det = [](const double* m) {
        return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    };
    const double dU = det(U) < 0.0 ? -1.0 : 1.0, dV = det(V) < 0.0 ? -1.0 : 1.0;
    double gU[9], gV[9];
    // mode = Up Vp^T:  gUp += gM Vp,  gVp = gM^T Up;  Up = U diag(1, 1, dU), Vp = V diag(1, 1, dV)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double cv = j == 2 ? dV : 1.0, cu = j == 2 ? dU : 1.0;
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a += gM[i * 3 + k] * V[k * 3 + j];
                b += gM[k * 3 + i] * U[k * 3 + j];
            }
            gU[i * 3 + j] = (gUp[i * 3 + j] + a * cv) * cu + gU_raw[i * 3 + j];
            gV[i * 3 + j] = (b * cu) * cv + gV_raw[i * 3 + j];
        }
    double gS[3] = {gS_raw[0] + gSp[0], gS_raw[1] + gSp[1], gS_raw[2] + gSp[2] * (dU * dV)};
    double A[9], Bm[9];                                      // U^T gU, V^T gV
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                a += U[k * 3 + i] * gU[k * 3 + j];
                b += V[k * 3 + i] * gV[k * 3 + j];
            }
            A[i * 3 + j] = a;
            Bm[i * 3 + j] = b;
        }
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (i == j) { M[i * 3 + j] = gS[i]; continue; }
            const double E = 1.0 / (S[j] * S[j] - S[i] * S[i]);
            M[i * 3 + j] = (A[i * 3 + j] - A[j * 3 + i]) * E * S[j] + S[i] * ((Bm[i * 3 + j] - Bm[j * 3 + i]) * E);
        }
    double UM[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) UM[i * 3 + j] = U[i * 3 + 0] * M[0 * 3 + j] + U[i * 3 + 1] * M[1 * 3 + j] + U[i * 3 + 2] * M[2 * 3 + j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            gF[i * 3 + j] = gF_direct[i * 3 + j] + UM[i * 3 + 0] * V[j * 3 + 0] + UM[i * 3 + 1] * V[j * 3 + 1] + UM[i * 3 + 2] * V[j * 3 + 2];
}

// One kinematic level of the joint loop (:121-160) backwards: grid = (joints of the level, batch tiles of BW_TBL images).  The
// joint's descendants (deeper levels, earlier launches) have left the gradient of their MLP inputs in ws.gx; this joint sums the
// slots that hold its U_proper / S_proper / mode over its descendants in the fixed order of the descendant table.
__global__ __launch_bounds__(BW_NT) void joint_level_backward_kernel(
    const double* __restrict__ embed, int embed_dim, const int32_t* __restrict__ joint_ids, const int32_t* __restrict__ anc_ptr,
    const int32_t* __restrict__ anc_idx, const int32_t* __restrict__ desc_ptr, const int32_t* __restrict__ desc_joint,
    const int32_t* __restrict__ desc_pos, const int32_t* __restrict__ in_off, const float* const* __restrict__ w1t_ptrs,
    const float* const* __restrict__ b1_ptrs, const float* const* __restrict__ w2_ptrs, const double* __restrict__ u_proper,
    const double* __restrict__ s_proper, const double* __restrict__ mode, const double* __restrict__ pose_u,
    const double* __restrict__ pose_s, const double* __restrict__ pose_v, const float* __restrict__ g_pose_f,
    const float* __restrict__ g_pose_s, const float* __restrict__ g_mode, const float* __restrict__ g_pose_u,
    const float* __restrict__ g_pose_v, LevelsWs ws, int B, int NJ) {
    __builtin_amdgcn_s_setprio(3);                           // a short latency chain, as the forward levels (csrc/head.hip)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NT = BW_NT, TBL = BW_TBL, HID = BW_HID;
    const int joint = joint_ids[blockIdx.x], b0 = blockIdx.y * TBL, tid = threadIdx.x;
    const int a_lo = anc_ptr[joint], P = anc_ptr[joint + 1] - a_lo;
    const int in_dim = embed_dim + 21 * P;
    float* xs = smem;                                        // [in_dim][TBL]
    float* hs = smem + (size_t)((in_dim * TBL + 3) & ~3);    // [HID][TBL] hidden activations
    float* ds = hs + HID * TBL;                              // [HID][TBL] ELU', then the pre-activation gradient
    double* red = reinterpret_cast<double*>(ds + HID * TBL); // [2][TBL][HID] partial sums (float64: 8-byte aligned, the offset is a multiple of 4 floats)
    float* gfs = ds + HID * TBL + 4 * TBL * HID;             // [TBL][12] gradient of joint_F
    const size_t blk = (size_t)B * in_off[joint];            // this joint's block in ws.gx / ws.xs

    // the MLP input cat[embed, U_proper[anc], S_proper[anc], mode[anc]] (:126-132), rows beyond B are zero
    for (int i = tid; i < in_dim * TBL; i += NT) {
        const int r = i / in_dim, k = i - r * in_dim;
        const int b = b0 + r;
        float v = 0.0f;
        if (b < B) {
            v = (float)level_input<double>(embed, embed_dim, u_proper, s_proper, mode, anc_idx, a_lo, P, (size_t)b, NJ, k);
            ws.xs[blk + (size_t)b * in_dim + k] = v;
        }
        xs[k * TBL + r] = v;
    }

    // gradient of joint_F: one lane per image (straight-line code, no divergence)
    if (tid < TBL) {
        const int b = b0 + tid;
        double gF[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) gF[e] = 0.0;
        if (b < B) {
            const size_t o = (size_t)b * NJ + joint;
            double gUp[9], gSp[3], gM[9], gS[3], gFd[9], gUr[9], gVr[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) {
                gUp[e] = 0.0;
                gUr[e] = g_pose_u ? (double)g_pose_u[o * 9 + e] : 0.0;
                gVr[e] = g_pose_v ? (double)g_pose_v[o * 9 + e] : 0.0;
                gM[e] = g_mode ? (double)g_mode[o * 9 + e] : 0.0;
                gFd[e] = g_pose_f ? (double)g_pose_f[o * 9 + e] : 0.0;
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) { gSp[e] = 0.0; gS[e] = g_pose_s ? (double)g_pose_s[o * 3 + e] : 0.0; }
            for (int q = desc_ptr[joint]; q < desc_ptr[joint + 1]; ++q) {
                const int d = desc_joint[q], p = desc_pos[q];
                const int Pd = anc_ptr[d + 1] - anc_ptr[d];
                const float* g = ws.gx + (size_t)B * in_off[d] + (size_t)b * (embed_dim + 21 * Pd) + embed_dim;
#pragma unroll
                for (int e = 0; e < 9; ++e) { gUp[e] += (double)g[9 * p + e]; gM[e] += (double)g[12 * Pd + 9 * p + e]; }
#pragma unroll
                for (int e = 0; e < 3; ++e) gSp[e] += (double)g[9 * Pd + 3 * p + e];
            }
            svd_head_backward(pose_u + o * 9, pose_s + o * 3, pose_v + o * 9, gUp, gSp, gM, gS, gFd, gUr, gVr, gF);
#pragma unroll
            for (int e = 0; e < 9; ++e) ws.gf[o * 9 + e] = (float)gF[e];
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) gfs[tid * 12 + e] = (float)gF[e];
    }
    __syncthreads();

    // hidden layer again (the forward keeps no activations)
    hidden_slices<float>(xs, w1t_ptrs[joint], in_dim, tid, red);
    __syncthreads();
    for (int i = tid; i < HID * TBL; i += NT) {
        const int r = i / HID, c = i % HID;
        const float pre = (float)((double)b1_ptrs[joint][c] + red[r * HID + c] + red[(TBL + r) * HID + c]);
        const float h = elu_fwd(pre);
        hs[c * TBL + r] = h;
        ds[c * TBL + r] = pre > 0.0f ? 1.0f : expf(pre);
        if (b0 + r < B) ws.h[((size_t)(b0 + r) * NJ + joint) * HID + c] = h;
    }
    __syncthreads();

    // output layer and ELU backwards: gp[c] = ELU'(pre[c]) * sum_e W2[e, c] gF[e]; every (c, r) touches its own slot of ds only
    for (int i = tid; i < HID * TBL; i += NT) {
        const int r = i / HID, c = i % HID;
        const float* w2 = w2_ptrs[joint] + c;
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) v += (double)w2[e * HID] * (double)gfs[r * 12 + e];
        const float gp = (float)(v * (double)ds[c * TBL + r]);
        ds[c * TBL + r] = gp;
        if (b0 + r < B) ws.gp[((size_t)(b0 + r) * NJ + joint) * HID + c] = gp;
    }
    __syncthreads();

    // hidden layer backwards: gx[k] = sum_n W1[n, k] gp[n] -- row k of W1^T is contiguous
    for (int k = tid; k < in_dim; k += NT) {
        const float4* row = reinterpret_cast<const float4*>(w1t_ptrs[joint] + (size_t)k * HID);
        double acc[TBL];
#pragma unroll
        for (int r = 0; r < TBL; ++r) acc[r] = 0.0;
        for (int n4 = 0; n4 < HID / 4; ++n4) {
            const float4 w = row[n4];
            const float wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 g = *reinterpret_cast<const float4*>(ds + (n4 * 4 + u) * TBL);
                acc[0] += (double)wv[u] * (double)g.x; acc[1] += (double)wv[u] * (double)g.y;
                acc[2] += (double)wv[u] * (double)g.z; acc[3] += (double)wv[u] * (double)g.w;
            }
        }
#pragma unroll
        for (int r = 0; r < TBL; ++r)
            if (b0 + r < B) ws.gx[blk + (size_t)(b0 + r) * in_dim + k] = (float)acc[r];
    }
}


// ---- the forward again, in float64, for the backward to differentiate at ----
// The gradient's error is the head's second derivative times the error of the forward values it is evaluated at, and
// torch.svd's backward multiplies by 1 / (s_j^2 - s_i^2): a rounding of 2^-23 |F| in the fp32 forward's F is amplified by that
// factor at every joint and handed down the kinematic chain.  The backward therefore starts with this pass: the same function with
// float64 sums and float64 values between the stages, the singular vectors' signs taken from the forward's pose_U, so that only
// the backward's own fp32 roundings remain.

// out[b, n] = act(sum_k in[b, k] wt[k, n] + bias[n] + addend[n]); input column k < K1 from in1 (fp32), the others from in2 (float64);
// wt (K, N) as the forward holds it.  grid = (ceil(N / 256), B).
__global__ __launch_bounds__(256) void refine_linear_kernel(const float* __restrict__ in1, int ld1, int K1, const double* __restrict__ in2,
                                                            int ld2, int K, const float* __restrict__ wt, const float* __restrict__ bias,
                                                            const float* __restrict__ addend, int elu, double* __restrict__ out_d,
                                                            float* __restrict__ out_f, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const size_t b = blockIdx.y;
    if (n >= N) return;
    double acc = (double)bias[n] + (addend ? (double)addend[n] : 0.0);
    for (int k = 0; k < K1; ++k) acc += (double)in1[b * ld1 + k] * (double)wt[(size_t)k * N + n];
    for (int k = K1; k < K; ++k) acc += in2[b * ld2 + (k - K1)] * (double)wt[(size_t)k * N + n];
    if (elu) acc = acc > 0.0 ? acc : expm1(acc);
    out_d[b * N + n] = acc;
    if (out_f) out_f[b * N + n] = (float)acc;
}

// F = U diag(S) V^T of a 3x3 matrix by one-sided Jacobi rotations in float64, singular values in decreasing order; the sign of
// column k of U and V is the one of the forward's (fp32) factor u_pin.  A column pair counts as orthogonal at 4 x 2^-53 relative
// (below that a rotation only moves rounding noise).  The sign is that of <U[:, k], u_pin[:, k]>: for separated singular values the
// two agree to fp32 rounding (|dot| near 1); where a pair of singular values nearly coincides the vectors of the pair are not
// determined, |dot| can be small, and 1 / (s_j^2 - s_i^2) makes the gradient as ill-conditioned in torch's own backward -- the sign
// of the dot is still the closest branch to the forward's.
__device__ void svd3_f64_pinned(const double* F, const float* __restrict__ u_pin, double* U, double* S, double* V) {
    double G[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) { G[e] = F[e]; V[e] = (e % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 40; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
            for (int i = 0; i < 3; ++i) { al += G[i * 3 + p] * G[i * 3 + p]; be += G[i * 3 + q] * G[i * 3 + q]; ga += G[i * 3 + p] * G[i * 3 + q]; }
            if (fabs(ga) <= 4.440892098500626e-16 * sqrt(al * be)) continue;
            rotated = true;
            const double zeta = (be - al) / (2.0 * ga);
            const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double gp = G[i * 3 + p], gq = G[i * 3 + q], vp = V[i * 3 + p], vq = V[i * 3 + q];
                G[i * 3 + p] = c * gp - sn * gq; G[i * 3 + q] = sn * gp + c * gq;
                V[i * 3 + p] = c * vp - sn * vq; V[i * 3 + q] = sn * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    double nrm[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[k] = sqrt(G[k] * G[k] + G[3 + k] * G[3 + k] + G[6 + k] * G[6 + k]);
    // decreasing order (three compare-and-swaps of whole columns)
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int a = pass == 1 ? 1 : 0, b = pass == 1 ? 2 : 1;
        if (nrm[a] < nrm[b]) {
            double t = nrm[a]; nrm[a] = nrm[b]; nrm[b] = t;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                t = G[i * 3 + a]; G[i * 3 + a] = G[i * 3 + b]; G[i * 3 + b] = t;
                t = V[i * 3 + a]; V[i * 3 + a] = V[i * 3 + b]; V[i * 3 + b] = t;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        S[k] = nrm[k];
        double dot = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            U[i * 3 + k] = nrm[k] > 0.0 ? G[i * 3 + k] / nrm[k] : (double)u_pin[i * 3 + k];
            dot += U[i * 3 + k] * (double)u_pin[i * 3 + k];
        }
        if (dot < 0.0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) { U[i * 3 + k] = -U[i * 3 + k]; V[i * 3 + k] = -V[i * 3 + k]; }
        }
    }
}

// One kinematic level of the joint loop (:121-160) in float64, root to leaves: grid = (joints of the level, batch tiles).
__global__ __launch_bounds__(BW_NT) void joint_level_refine_kernel(
    const double* __restrict__ embed, int embed_dim, const int32_t* __restrict__ joint_ids, const int32_t* __restrict__ anc_ptr,
    const int32_t* __restrict__ anc_idx, const float* const* __restrict__ w1t_ptrs, const float* const* __restrict__ b1_ptrs,
    const float* const* __restrict__ w2_ptrs, const float* const* __restrict__ b2_ptrs, float delta_i_weight,
    const float* __restrict__ pose_u_pin, double* u_proper, double* s_proper, double* mode, double* __restrict__ pose_u,
    double* __restrict__ pose_s, double* __restrict__ pose_v, int B, int NJ) {
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(16))) double smem_d[];
    constexpr int NT = BW_NT, TBL = BW_TBL, HID = BW_HID;
    const int joint = joint_ids[blockIdx.x], b0 = blockIdx.y * TBL, tid = threadIdx.x;
    const int a_lo = anc_ptr[joint], P = anc_ptr[joint + 1] - a_lo;
    const int in_dim = embed_dim + 21 * P;
    double* xs = smem_d;                       // [in_dim][TBL]
    double* hs = xs + (size_t)in_dim * TBL;    // [HID][TBL]
    double* red = hs + HID * TBL;              // [2][TBL][HID]
    double* fs = red + 2 * TBL * HID;          // [TBL][9]
    for (int i = tid; i < in_dim * TBL; i += NT) {
        const int r = i / in_dim, k = i - r * in_dim;
        const int b = b0 + r;
        xs[k * TBL + r] = b < B ? level_input<double>(embed, embed_dim, u_proper, s_proper, mode, anc_idx, a_lo, P, (size_t)b, NJ, k) : 0.0;
    }
    __syncthreads();
    hidden_slices<double>(xs, w1t_ptrs[joint], in_dim, tid, red);
    __syncthreads();
    for (int i = tid; i < HID * TBL; i += NT) {
        const int r = i / HID, c = i % HID;
        const double pre = (double)b1_ptrs[joint][c] + red[r * HID + c] + red[(TBL + r) * HID + c];
        hs[c * TBL + r] = pre > 0.0 ? pre : expm1(pre);
    }
    __syncthreads();
    if (tid < 9 * TBL) {
        const int e = tid / TBL, r = tid % TBL;
        const float* w2 = w2_ptrs[joint] + (size_t)e * HID;
        double v = (double)b2_ptrs[joint][e] + (e % 4 == 0 ? (double)delta_i_weight : 0.0);
        for (int k = 0; k < HID; ++k) v += (double)w2[k] * hs[k * TBL + r];
        fs[r * 9 + e] = v;
    }
    __syncthreads();
    if (tid < TBL && b0 + tid < B) {
        const size_t o = (size_t)(b0 + tid) * NJ + joint;
        double U[9], S[3], V[9];
        svd3_f64_pinned(fs + tid * 9, pose_u_pin + o * 9, U, S, V);
        auto det = [](const double* m) {
            return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
        };
        const double dU = det(U) < 0.0 ? -1.0 : 1.0, dV = det(V) < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int e = 0; e < 9; ++e) { pose_u[o * 9 + e] = U[e]; pose_v[o * 9 + e] = V[e]; }
#pragma unroll
        for (int e = 0; e < 3; ++e) { pose_s[o * 3 + e] = S[e]; s_proper[o * 3 + e] = e == 2 ? S[e] * (dU * dV) : S[e]; }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                u_proper[o * 9 + i * 3 + j] = j == 2 ? U[i * 3 + j] * dU : U[i * 3 + j];
                mode[o * 9 + i * 3 + j] = U[i * 3 + 0] * V[j * 3 + 0] + U[i * 3 + 1] * V[j * 3 + 1] + (dU * dV) * U[i * 3 + 2] * V[j * 3 + 2];
            }
    }
}

// g_embed[b, k] = sum over the joints, ascending, of the embedding's slot of their MLP-input gradient
__global__ void embed_grad_kernel(const float* __restrict__ gx, const int32_t* __restrict__ anc_ptr, const int32_t* __restrict__ in_off,
                                  float* __restrict__ g_embed, int embed_dim, int B, int NJ) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (k >= embed_dim) return;
    double v = 0.0;
    for (int j = 0; j < NJ; ++j) {
        const int in_dim = embed_dim + 21 * (anc_ptr[j + 1] - anc_ptr[j]);
        v += (double)gx[(size_t)B * in_off[j] + (size_t)b * in_dim + k];
    }
    g_embed[(size_t)b * embed_dim + k] = (float)v;
}

// sum over the images, ascending, of g[b] * x[b] (x == nullptr: of g[b]): one float64 chain per output (the products are exact in
// float64, so splitting the batch would change nothing but the last bit of the fp32 result), loads in fixed chunks of four images
__device__ __forceinline__ float batch_dot(const float* __restrict__ g, size_t ldg, const float* __restrict__ x, size_t ldx, int B) {
    double acc = 0.0;
    int b = 0;
    for (; b + 4 <= B; b += 4) {
        float gv[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { gv[u] = g[(size_t)(b + u) * ldg]; xv[u] = x ? x[(size_t)(b + u) * ldx] : 1.0f; }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc += (double)gv[u] * (double)xv[u];
    }
    for (; b < B; ++b) acc += (double)g[(size_t)b * ldg] * (x ? (double)x[(size_t)b * ldx] : 1.0);
    return (float)acc;
}

// The four parameter gradients of every fc_pose[j], nn.Linear's layout, into the flat buffer
// [g_W1 (128, in_dim) | g_b1 (128) | g_W2 (9, 128) | g_b2 (9)] of joint j at 128 * in_off[j] + j * BW_JOINT_TAIL.
// grid = (tiles over the joint's outputs, joints); one thread per output.
__global__ __launch_bounds__(256) void joint_wgrad_kernel(const int32_t* __restrict__ anc_ptr, const int32_t* __restrict__ in_off,
                                                          LevelsWs ws, float* __restrict__ g_params, int embed_dim, int B, int NJ) {
    constexpr int HID = BW_HID;
    const int j = blockIdx.y;
    const int in_dim = embed_dim + 21 * (anc_ptr[j + 1] - anc_ptr[j]);
    const int n_w1 = HID * in_dim;
    int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_w1 + BW_JOINT_TAIL) return;
    float* out = g_params + (size_t)HID * in_off[j] + (size_t)j * BW_JOINT_TAIL + i;
    const float* gp = ws.gp + (size_t)j * HID;
    const float* gf = ws.gf + (size_t)j * 9;
    const float* h = ws.h + (size_t)j * HID;
    const size_t ldh = (size_t)NJ * HID, ldf = (size_t)NJ * 9;
    if (i < n_w1) {
        const int n = i / in_dim, k = i - n * in_dim;
        *out = batch_dot(gp + n, ldh, ws.xs + (size_t)B * in_off[j] + k, (size_t)in_dim, B);
        return;
    }
    i -= n_w1;
    if (i < HID) { *out = batch_dot(gp + i, ldh, nullptr, 0, B); return; }
    i -= HID;
    if (i < 9 * HID) { *out = batch_dot(gf + i / HID, ldf, h + i % HID, ldh, B); return; }
    i -= 9 * HID;
    *out = batch_dot(gf + i, ldf, nullptr, 0, B);
}

// gx[b, k] = ( sum_n gy[b, n] W[n, k] + add[b, k] ) * ELU'(from the layer's output y[b, k]);  W (N, K) is nn.Linear's own layout of
// the layer being differentiated.  gy == nullptr or N == 0: no product; add / y == nullptr: no addend / no factor.
// grid = (ceil(K / 256), B): an image's row is computed from that image alone.
__global__ __launch_bounds__(256) void linear_data_backward_kernel(const float* __restrict__ gy, int ldg, const float* __restrict__ W, int ldw,
                                                                   int N, int K, const float* __restrict__ add, int ldadd,
                                                                   const float* __restrict__ y, int ldy, float* __restrict__ gx, int ldgx) {
    __builtin_amdgcn_s_setprio(3);
    const int k = blockIdx.x * 256 + threadIdx.x;
    const size_t b = blockIdx.y;
    if (k >= K) return;
    double acc = 0.0;
    if (gy) {
        const float* g = gy + b * ldg;
        const float* w = W + k;
        int n = 0;
        for (; n + 8 <= N; n += 8) {
            float wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = w[(size_t)(n + u) * ldw];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += (double)g[n + u] * (double)wv[u];
        }
        for (; n < N; ++n) acc += (double)g[n] * (double)w[(size_t)n * ldw];
    }
    if (add) acc += (double)add[b * ldadd + k];
    if (y) acc *= (double)elu_grad_from_out(y[b * ldy + k]);
    gx[b * ldgx + k] = (float)acc;
}

// gradient of the fused fc_shape | fc_glob | fc_cam output (:98-107): what came back through fc_embed's input (:108) plus the
// caller's cotangents; scale = exp(log std) (:101), so g_log_std = g_scale * scale
__global__ void sgc_grad_kernel(const float* __restrict__ g_cat, int ldc, int nf, const float* __restrict__ g_loc,
                                const float* __restrict__ g_scale, const float* __restrict__ scale, const float* __restrict__ g_glob,
                                const float* __restrict__ g_cam, float* __restrict__ g_sgc, int nsh, int ng, int nc, int B) {
    const int nt = 2 * nsh + ng + nc;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * nt) return;
    const size_t b = i / nt;
    const int c = i % nt;
    float v = g_cat[b * ldc + nf + c];
    if (c < nsh) v += g_loc ? g_loc[b * nsh + c] : 0.0f;
    else if (c < 2 * nsh) v += g_scale ? g_scale[b * nsh + (c - nsh)] * scale[b * nsh + (c - nsh)] : 0.0f;
    else if (c < 2 * nsh + ng) v += g_glob ? g_glob[b * ng + (c - 2 * nsh)] : 0.0f;
    else v += g_cam ? g_cam[b * nc + (c - 2 * nsh - ng)] : 0.0f;
    g_sgc[i] = v;
}

// dW[n, k] = sum_b g[b, n] x[b, k] (rows of dW have stride ldw), db[n] = sum_b g[b, n] (db may be nullptr); one thread per output
__global__ __launch_bounds__(256) void linear_wgrad_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ x, int ldx,
                                                           float* __restrict__ dW, int ldw, float* __restrict__ db, int N, int K, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (int64_t)N * K) {
        const int n = (int)(i / K), k = (int)(i % K);
        dW[(size_t)n * ldw + k] = batch_dot(g + n, (size_t)ldg, x + k, (size_t)ldx, B);
    } else if (db && i < (int64_t)N * K + N) {
        const int n = (int)(i - (int64_t)N * K);
        db[n] = batch_dot(g + n, (size_t)ldg, nullptr, 0, B);
    }
}

// utils/rigid_transform_utils.py:80-94 backwards, one thread per matrix: the forward's values again, then the chain
// b3 = b1 x b2, b2 = u / |u|, u = a2 - (b1 . a2) b1, b1 = a1 / |a1|  (norms clamped at 1e-12 as F.normalize does)
__global__ void rot6d_to_rotmat_backward_kernel(const float* __restrict__ x, const float* __restrict__ g_r, float* __restrict__ g_x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* s = x + (size_t)i * 6;
    const float* G = g_r + (size_t)i * 9;
    const double a1[3] = {s[0], s[2], s[4]}, a2[3] = {s[1], s[3], s[5]};
    const double eps = 1e-12;
    const double l1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]), n1 = fmax(l1, eps);
    const double b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    const double d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    const double u[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    const double l2 = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), n2 = fmax(l2, eps);
    const double b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    double gb1[3] = {G[0], G[3], G[6]}, gb2[3] = {G[1], G[4], G[7]};
    const double gb3[3] = {G[2], G[5], G[8]};
    // b3 = b1 x b2:  gb1 += b2 x gb3,  gb2 += gb3 x b1
    gb1[0] += b2[1] * gb3[2] - b2[2] * gb3[1]; gb1[1] += b2[2] * gb3[0] - b2[0] * gb3[2]; gb1[2] += b2[0] * gb3[1] - b2[1] * gb3[0];
    gb2[0] += gb3[1] * b1[2] - gb3[2] * b1[1]; gb2[1] += gb3[2] * b1[0] - gb3[0] * b1[2]; gb2[2] += gb3[0] * b1[1] - gb3[1] * b1[0];
    // b2 = u / max(|u|, eps)
    const double t2 = l2 > eps ? b2[0] * gb2[0] + b2[1] * gb2[1] + b2[2] * gb2[2] : 0.0;
    const double gu[3] = {(gb2[0] - b2[0] * t2) / n2, (gb2[1] - b2[1] * t2) / n2, (gb2[2] - b2[2] * t2) / n2};
    // u = a2 - d b1, d = b1 . a2
    const double gd = -(gu[0] * b1[0] + gu[1] * b1[1] + gu[2] * b1[2]);
    double ga2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ga2[k] = gu[k] + gd * b1[k]; gb1[k] += -d * gu[k] + gd * a2[k]; }
    // b1 = a1 / max(|a1|, eps)
    const double t1 = l1 > eps ? b1[0] * gb1[0] + b1[1] * gb1[1] + b1[2] * gb1[2] : 0.0;
    float* o = g_x + (size_t)i * 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) { o[2 * k] = (float)((gb1[k] - b1[k] * t1) / n1); o[2 * k + 1] = (float)ga2[k]; }
}

}  // namespace hps

using namespace hps;


extern "C" int hps_head_forward_refine(const float* feats, int ldf, const float* fc1_wt, const float* fc1_b, const float* sgc_wt,
                                       const float* sgc_b, const float* sgc_add, const float* embed_wt, const float* embed_b,
                                       const int32_t* level_joints, const int32_t* level_sizes_host, int n_levels,
                                       const int32_t* anc_ptr, const int32_t* anc_idx, const float* const* w1t_ptrs,
                                       const float* const* b1_ptrs, const float* const* w2_ptrs, const float* const* b2_ptrs,
                                       float delta_i_weight, const float* pose_u_pin, float* x_f, float* sgc_f, float* embed_f,
                                       double* x_d, double* sgc_d, double* embed_d, double* u_proper, double* s_proper, double* mode,
                                       double* pose_u, double* pose_s, double* pose_v, int B, int num_feats, int hidden_trunk,
                                       int num_sgc, int embed_dim, int hidden, int num_body_joints, hps_stream_t stream) {
    if (!feats || !fc1_wt || !fc1_b || !sgc_wt || !sgc_b || !sgc_add || !embed_wt || !embed_b || !level_joints || !level_sizes_host ||
        !anc_ptr || !anc_idx || !w1t_ptrs || !b1_ptrs || !w2_ptrs || !b2_ptrs || !pose_u_pin || !x_f || !sgc_f || !embed_f || !x_d ||
        !sgc_d || !embed_d || !u_proper || !s_proper || !mode || !pose_u || !pose_s || !pose_v)
        return bad_arg("hps_head_forward_refine: null pointer");
    if (hidden != BW_HID) { set_error("hps_head_forward_refine: hidden=%d unsupported (128 = EMBED_DIM/2)", hidden); return HPS_E_UNSUPPORTED; }
    if (num_feats <= 0 || hidden_trunk <= 0 || num_sgc <= 0 || embed_dim <= 0 || num_body_joints <= 0 || n_levels < 0 || ldf < num_feats)
        return bad_arg("hps_head_forward_refine: dims");
    if (B <= 0) return HPS_OK;
    if (B > 65535) { set_error("hps_head_forward_refine: B=%d exceeds the grid's 65535 rows; split the batch", B); return HPS_E_UNSUPPORTED; }
    const int NJ = num_body_joints, max_in = embed_dim + 21 * NJ;
    const size_t lds = ((size_t)max_in * BW_TBL + BW_HID * BW_TBL + 2 * BW_TBL * BW_HID + BW_TBL * 9) * sizeof(double);
    if (lds > 64 * 1024) { set_error("hps_head_forward_refine: embed_dim=%d too large", embed_dim); return HPS_E_UNSUPPORTED; }
    hipStream_t s = (hipStream_t)stream;
    const char* who = "hps_head_forward_refine";
    int rc;
    // :95-96, :98-107, :108-110
    hipLaunchKernelGGL(refine_linear_kernel, dim3(ceil_div(hidden_trunk, 256), B), dim3(256), 0, s, feats, ldf, num_feats, (const double*)nullptr,
                       0, num_feats, fc1_wt, fc1_b, (const float*)nullptr, 1, x_d, x_f, hidden_trunk);
    if ((rc = check_launch(who)) != HPS_OK) return rc;
    hipLaunchKernelGGL(refine_linear_kernel, dim3(ceil_div(num_sgc, 256), B), dim3(256), 0, s, (const float*)nullptr, 0, 0, (const double*)x_d,
                       hidden_trunk, hidden_trunk, sgc_wt, sgc_b, sgc_add, 0, sgc_d, sgc_f, num_sgc);
    if ((rc = check_launch(who)) != HPS_OK) return rc;
    hipLaunchKernelGGL(refine_linear_kernel, dim3(ceil_div(embed_dim, 256), B), dim3(256), 0, s, feats, ldf, num_feats, (const double*)sgc_d,
                       num_sgc, num_feats + num_sgc, embed_wt, embed_b, (const float*)nullptr, 1, embed_d, embed_f, embed_dim);
    if ((rc = check_launch(who)) != HPS_OK) return rc;
    int first = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int n_level = level_sizes_host[l];
        if (n_level < 0 || first + n_level > NJ) return bad_arg("hps_head_forward_refine: level size");
        if (n_level > 0) {
            hipLaunchKernelGGL(joint_level_refine_kernel, dim3(n_level, ceil_div(B, BW_TBL)), dim3(BW_NT), lds, s, (const double*)embed_d,
                               embed_dim, level_joints + first, anc_ptr, anc_idx, w1t_ptrs, b1_ptrs, w2_ptrs, b2_ptrs, delta_i_weight,
                               pose_u_pin, u_proper, s_proper, mode, pose_u, pose_s, pose_v, B, NJ);
            if ((rc = check_launch(who)) != HPS_OK) return rc;
        }
        first += n_level;
    }
    return HPS_OK;
}

extern "C" int hps_head_pose_levels_backward_factors(const double* embed, int embed_dim, int hidden, const int32_t* level_joints,
                                             const int32_t* level_sizes_host, int n_levels, const int32_t* anc_ptr,
                                             const int32_t* anc_idx, const int32_t* desc_ptr, const int32_t* desc_joint,
                                             const int32_t* desc_pos, const int32_t* in_off, const float* const* w1t_ptrs,
                                             const float* const* b1_ptrs, const float* const* w2_ptrs, const double* u_proper,
                                             const double* s_proper, const double* mode, const double* pose_u, const double* pose_s,
                                             const double* pose_v, const float* g_pose_f, const float* g_pose_s, const float* g_mode,
                                             const float* g_pose_u, const float* g_pose_v, float* g_embed, float* g_fc_pose, float* workspace, int B, int num_body_joints,
                                             int total_in, hps_stream_t stream) {
    if (!embed || !level_joints || !level_sizes_host || !anc_ptr || !anc_idx || !desc_ptr || !desc_joint || !desc_pos || !in_off ||
        !w1t_ptrs || !b1_ptrs || !w2_ptrs || !u_proper || !s_proper || !mode || !pose_u || !pose_s || !pose_v || !g_embed || !workspace)
        return bad_arg("hps_head_pose_levels_backward_factors: null pointer");
    if (hidden != BW_HID) { set_error("hps_head_pose_levels_backward_factors: hidden=%d unsupported (128 = EMBED_DIM/2)", hidden); return HPS_E_UNSUPPORTED; }
    const int NJ = num_body_joints;
    if (embed_dim <= 0 || NJ <= 0 || n_levels < 0 || total_in < NJ * embed_dim || total_in > NJ * (embed_dim + 21 * NJ))
        return bad_arg("hps_head_pose_levels_backward_factors: dims");
    int n_total = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (level_sizes_host[l] < 0) return bad_arg("hps_head_pose_levels_backward_factors: level size");
        n_total += level_sizes_host[l];
    }
    if (n_total != NJ) return bad_arg("hps_head_pose_levels_backward_factors: the levels must hold every joint once");
    if (B <= 0) return HPS_OK;
    if (B > 65535) { set_error("hps_head_pose_levels_backward_factors: B=%d exceeds the grid's 65535 rows; split the batch", B); return HPS_E_UNSUPPORTED; }
    const int max_in = embed_dim + 21 * NJ;
    const size_t lds = ((size_t)((max_in * BW_TBL + 3) & ~3) + 2 * BW_HID * BW_TBL + 4 * BW_TBL * BW_HID + BW_TBL * 12) * sizeof(float);
    if (lds > 64 * 1024) { set_error("hps_head_pose_levels_backward_factors: embed_dim=%d too large", embed_dim); return HPS_E_UNSUPPORTED; }
    LevelsWs ws;
    ws.gx = workspace;
    ws.xs = ws.gx + (size_t)B * total_in;
    ws.h = ws.xs + (size_t)B * total_in;
    ws.gp = ws.h + (size_t)B * NJ * BW_HID;
    ws.gf = ws.gp + (size_t)B * NJ * BW_HID;
    hipStream_t s = (hipStream_t)stream;
    // leaves first: a level reads what the deeper levels wrote
    int first = n_total;
    for (int l = n_levels - 1; l >= 0; --l) {
        const int n_level = level_sizes_host[l];
        first -= n_level;
        if (n_level == 0) continue;
        hipLaunchKernelGGL(joint_level_backward_kernel, dim3(n_level, ceil_div(B, BW_TBL)), dim3(BW_NT), lds, s, embed, embed_dim,
                           level_joints + first, anc_ptr, anc_idx, desc_ptr, desc_joint, desc_pos, in_off, w1t_ptrs, b1_ptrs, w2_ptrs,
                           u_proper, s_proper, mode, pose_u, pose_s, pose_v, g_pose_f, g_pose_s, g_mode, g_pose_u, g_pose_v, ws, B, NJ);
        const int rc = check_launch("hps_head_pose_levels_backward_factors");
        if (rc != HPS_OK) return rc;
    }
    hipLaunchKernelGGL(embed_grad_kernel, dim3(ceil_div(embed_dim, 256), B), dim3(256), 0, s, ws.gx, anc_ptr, in_off, g_embed, embed_dim,
                       B, NJ);
    int rc = check_launch("hps_head_pose_levels_backward_factors");
    if (rc != HPS_OK || !g_fc_pose) return rc;               // no parameter gradients wanted
    hipLaunchKernelGGL(joint_wgrad_kernel, dim3(ceil_div(BW_HID * max_in + BW_JOINT_TAIL, 256), NJ), dim3(256), 0, s, anc_ptr, in_off, ws,
                       g_fc_pose, embed_dim, B, NJ);
    return check_launch("hps_head_pose_levels_backward_factors");
}

// The entry point without cotangents on the raw factors (pose_U / pose_V not differentiable outputs): NULL = zero for both.
extern "C" int hps_head_pose_levels_backward(const double* embed, int embed_dim, int hidden, const int32_t* level_joints,
                                             const int32_t* level_sizes_host, int n_levels, const int32_t* anc_ptr,
                                             const int32_t* anc_idx, const int32_t* desc_ptr, const int32_t* desc_joint,
                                             const int32_t* desc_pos, const int32_t* in_off, const float* const* w1t_ptrs,
                                             const float* const* b1_ptrs, const float* const* w2_ptrs, const double* u_proper,
                                             const double* s_proper, const double* mode, const double* pose_u, const double* pose_s,
                                             const double* pose_v, const float* g_pose_f, const float* g_pose_s, const float* g_mode,
                                             float* g_embed, float* g_fc_pose, float* workspace, int B, int num_body_joints,
                                             int total_in, hps_stream_t stream) {
    return hps_head_pose_levels_backward_factors(embed, embed_dim, hidden, level_joints, level_sizes_host, n_levels, anc_ptr, anc_idx,
                                                 desc_ptr, desc_joint, desc_pos, in_off, w1t_ptrs, b1_ptrs, w2_ptrs, u_proper, s_proper,
                                                 mode, pose_u, pose_s, pose_v, g_pose_f, g_pose_s, g_mode, nullptr, nullptr, g_embed,
                                                 g_fc_pose, workspace, B, num_body_joints, total_in, stream);
}

extern "C" int hps_head_trunk_backward(const float* feats, int ldf, const float* x, const float* sgc, const float* embed,
                                       const float* shape_scale, const float* fc1_w, const float* sgc_w, const float* embed_w,
                                       const float* g_embed, const float* g_loc, const float* g_scale, const float* g_glob,
                                       const float* g_cam, float* g_feats, float* g_fc1_w, float* g_fc1_b, float* g_sgc_w,
                                       float* g_sgc_b, float* g_embed_w, float* g_embed_b, float* workspace, int B, int num_feats,
                                       int hidden, int num_shape, int num_glob, int num_cam, int embed_dim, hps_stream_t stream) {
    if (!feats || !x || !sgc || !embed || !shape_scale || !fc1_w || !sgc_w || !embed_w || !workspace)
        return bad_arg("hps_head_trunk_backward: null pointer");
    const int n_param_out = !!g_fc1_w + !!g_fc1_b + !!g_sgc_w + !!g_sgc_b + !!g_embed_w + !!g_embed_b;
    if (n_param_out != 0 && n_param_out != 6) return bad_arg("hps_head_trunk_backward: the parameter gradients are all NULL or all given");
    if (num_feats <= 0 || hidden <= 0 || num_shape <= 0 || num_glob <= 0 || num_cam <= 0 || embed_dim <= 0 || ldf < num_feats)
        return bad_arg("hps_head_trunk_backward: dims");
    if (B <= 0) return HPS_OK;
    if (B > 65535) { set_error("hps_head_trunk_backward: B=%d exceeds the grid's 65535 rows; split the batch", B); return HPS_E_UNSUPPORTED; }
    const int nt = 2 * num_shape + num_glob + num_cam, ncat = num_feats + nt;
    float* ge = workspace;                                    // (B, embed_dim)  gradient of fc_embed's pre-activation
    float* g_cat = ge + (size_t)B * embed_dim;                // (B, ncat)       gradient of cat[feats, shape_params, glob, cam] (:108)
    float* g_sgc = g_cat + (size_t)B * ncat;                  // (B, nt)
    float* g_pre1 = g_sgc + (size_t)B * nt;                   // (B, hidden)     gradient of fc1's pre-activation
    hipStream_t s = (hipStream_t)stream;
    const char* who = "hps_head_trunk_backward";
    int rc;
    auto data = [&](const float* gy, int ldg, const float* W, int ldw, int N, int K, const float* add, int ldadd, const float* y, int ldy,
                    float* gx, int ldgx) {
        hipLaunchKernelGGL(linear_data_backward_kernel, dim3(ceil_div(K, 256), B), dim3(256), 0, s, gy, ldg, W, ldw, N, K, add, ldadd, y,
                           ldy, gx, ldgx);
        return check_launch(who);
    };
    auto wgrad = [&](const float* g, int ldg, const float* xin, int ldx, float* dW, int ldw, float* db, int N, int K) {
        const int64_t n_out = (int64_t)N * K + (db ? N : 0);
        hipLaunchKernelGGL(linear_wgrad_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, g, ldg, xin, ldx, dW, ldw, db, N, K, B);
        return check_launch(who);
    };
    // embed = ELU(fc_embed(cat))                                                                        (:108-110)
    if ((rc = data(nullptr, 0, nullptr, 0, 0, embed_dim, g_embed, embed_dim, embed, embed_dim, ge, embed_dim)) != HPS_OK) return rc;
    if ((rc = data(ge, embed_dim, embed_w, ncat, embed_dim, ncat, nullptr, 0, nullptr, 0, g_cat, ncat)) != HPS_OK) return rc;
    // shape_params | glob | cam                                                                         (:98-107)
    hipLaunchKernelGGL(sgc_grad_kernel, dim3(ceil_div(B * nt, 256)), dim3(256), 0, s, g_cat, ncat, num_feats, g_loc, g_scale, shape_scale,
                       g_glob, g_cam, g_sgc, num_shape, num_glob, num_cam, B);
    if ((rc = check_launch(who)) != HPS_OK) return rc;
    // x = ELU(fc1(feats))                                                                               (:95-96)
    if ((rc = data(g_sgc, nt, sgc_w, hidden, nt, hidden, nullptr, 0, x, hidden, g_pre1, hidden)) != HPS_OK) return rc;
    if (g_feats && (rc = data(g_pre1, hidden, fc1_w, num_feats, hidden, num_feats, g_cat, ncat, nullptr, 0, g_feats, num_feats)) != HPS_OK)
        return rc;
    if (!n_param_out) return HPS_OK;
    // parameter gradients
    if ((rc = wgrad(g_pre1, hidden, feats, ldf, g_fc1_w, num_feats, g_fc1_b, hidden, num_feats)) != HPS_OK) return rc;
    if ((rc = wgrad(g_sgc, nt, x, hidden, g_sgc_w, hidden, g_sgc_b, nt, hidden)) != HPS_OK) return rc;
    if ((rc = wgrad(ge, embed_dim, feats, ldf, g_embed_w, ncat, g_embed_b, embed_dim, num_feats)) != HPS_OK) return rc;
    return wgrad(ge, embed_dim, sgc, nt, g_embed_w + num_feats, ncat, nullptr, embed_dim, nt);
}

extern "C" int hps_rot6d_to_rotmat_backward(const float* x6, const float* g_rotmat, float* g_x6, int n, hps_stream_t stream) {
    if (!x6 || !g_rotmat || !g_x6) return bad_arg("hps_rot6d_to_rotmat_backward: null pointer");
    if (n <= 0) return HPS_OK;
    hipLaunchKernelGGL(rot6d_to_rotmat_backward_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, x6, g_rotmat, g_x6, n);
    return check_launch("hps_rot6d_to_rotmat_backward");
}
