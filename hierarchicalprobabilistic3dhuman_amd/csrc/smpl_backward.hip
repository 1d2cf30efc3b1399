// SMPL backward on gfx950: the reverse of the three forward stages (smpl.hip / blend_gemm.hip), in reverse order:
//   hps_smpl_lbs_backward        skinning: g_vposed, and the 6890 -> 24 x 12 reduction g_A as an fp32-MFMA product
//   hps_smpl_blend_backward      g_xt = bmat . g_vposed^T, the forward blend's FLOPs with the long axis contracted
//   hps_smpl_pose_prep_backward  forward kinematics leaves -> root, rest joints, Rodrigues
// Differentiates smplx 0.1.26 lbs / batch_rigid_transform / batch_rodrigues as reached from models/smpl_official.py:27-41 (the
// reference runs them under autograd in train/train_poseMF_shapeGaussian_net.py:268-271, :304-308).
// Every sum over vertices or coordinates is per-workgroup partials in a caller-provided workspace plus a fixed-order finish: no
// floating-point atomics, bitwise repeatable, and the geometry of the split depends on the model alone, never on M.
#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BWD_MAXJ = 32;

// ---------------------------------------------------------------------------------------------
// LBS backward.  A workgroup owns LB_CH consecutive vertices for its whole life and walks a range of meshes, LB_G at a time.
//   phase 1 (lane = vertex, four meshes each): gV' = gV + C^T gJ, T = sum_k w A, g_vposed = T.R^T gV' written over v_posed by the lane
//            that read it; gV' and [v_posed; 1] go to LDS.
//   phase 2 (wave = mesh pair): g_A[j] = sum_v W[v, j] (gV'_v (x) [v_posed_v; 1]) as a 32 x 32 MFMA tile -- rows = joints, columns =
//            2 meshes x 12 entries of the 3 x 4 transform, contraction over the chunk's vertices.  The dense skinning-weight
//            fragment W is mesh independent: built once per workgroup from (w_idx, w_val) and kept in LDS (16 KB).  The 32 - J
//            rows behind the joints carry ones for every (32 - J)-th vertex pair: their translation columns add up to sum_v gV'_v
//            (g_transl) in chains of 128 / (32 - J) terms instead of one chain of 128 -- 6890 terms of mixed sign want short chains.
// A chunk's partial goes to partials[chunk][mesh][J x 12 | (32 - J) x 3]; lbs_backward_finish_kernel adds the chunks in chunk order
// (g_transl: all its rows and chunks in float64, rounded once).
// The kernel moves 36 bytes per vertex and mesh and is bound by how many of them are in flight: the next group's cotangents,
// vertices and transforms are requested into registers before this group's MFMA phase (all four meshes of a lane at once -- read
// through vp_in, written through vp_out, the same buffer: a lane's store never precedes its own read of that vertex and no other
// lane touches it), the group's joint cotangents go through LDS (a lane that gathered its regressor entries from global memory
// waited for two dependent round trips per entry, and almost every wave holds such a lane), and the chunk's skinning weights reach
// the lanes through LDS, not as 512 scalar loads each.
// ---------------------------------------------------------------------------------------------
constexpr int LB_CH = 128, LB_G = 8, LB_MAXR = 96;      // (LB_MAXR: regressor rows whose cotangents a group stages in LDS)

template <int K>
__global__ __launch_bounds__(256) void lbs_backward_kernel(const float* __restrict__ vp_in, float* __restrict__ vp_out, int ld,
                                                           const float* __restrict__ a,
                                                           const int32_t* __restrict__ w_idx, const float* __restrict__ w_val, int J,
                                                           const float* __restrict__ gV, const float* __restrict__ gJ, int gj_pitch,
                                                           const int32_t* __restrict__ ct_ptr, const int32_t* __restrict__ ct_row,
                                                           const float* __restrict__ ct_val, float* __restrict__ partials, int M, int V,
                                                           int groups_per_block, int n_rows) {
    __shared__ __attribute__((aligned(16))) float sA[LB_G * BWD_MAXJ * 12];
    __shared__ __attribute__((aligned(16))) float sGv[LB_G][LB_CH][4];   // gV' (x, y, z, 0); first: the chunk's w_idx
    __shared__ __attribute__((aligned(16))) float sP[LB_G][LB_CH][4];    // v_posed (x, y, z, 1); first: the chunk's w_val
    __shared__ float sGJ[LB_G][LB_MAXR * 3];                             // g_joints rows behind the kinematic joints
    __shared__ float sRow[LB_CH / 2][64];                                // MFMA row operand (skinning weights, ones rows)
    constexpr int HG = LB_G / 2;                                          // meshes per lane
    constexpr int AQ = LB_G * BWD_MAXJ * 12 / 4 / 256;                    // float4 of A per lane (J = 32: all of them)
    constexpr int JQ = LB_MAXR * 3 / 32;                                  // g_joints floats per lane (32 lanes per mesh)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int il = lane & 31, kl = lane >> 5;
    const int chunk = blockIdx.x, v0 = chunk * LB_CH;
    const int n_groups = ceil_div(M, LB_G);
    const int g_begin = blockIdx.y * groups_per_block, g_end = min(n_groups, g_begin + groups_per_block);
    if (g_begin >= g_end) return;
    const int a_stride = J * 12;

    // the chunk's skinning weights -> LDS (coalesced), vertices behind V as (0, 0.0f)
    int* sI = reinterpret_cast<int*>(&sGv[0][0][0]);
    float* sW = &sP[0][0][0];
    {
        const int n = min(LB_CH, V - v0) * K;
        for (int i = tid; i < LB_CH * K; i += 256) {
            sI[i] = i < n ? w_idx[(size_t)v0 * K + i] : 0;
            sW[i] = i < n ? w_val[(size_t)v0 * K + i] : 0.0f;
        }
    }
    __syncthreads();
    // MFMA row operand, in LDS as the lanes read it: sRow[s][lane] = W[v0 + 2 s + kl][joint il]; rows J + t: 1 where s % (32 - J) == t
    // (the same for every wave: wave w builds steps 16 w .. 16 w + 15)
    const int n_ones = 32 - J;
    for (int s = wave * (LB_CH / 8); s < (wave + 1) * (LB_CH / 8); ++s) {
        const int q = 2 * s + kl;
        float x = 0.0f;
        if (il >= J) x = (v0 + q < V && s % n_ones == il - J) ? 1.0f : 0.0f;
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) x += (sI[q * K + k] == il) ? sW[q * K + k] : 0.0f;
        }
        sRow[s][lane] = x;
    }

    // phase 1 identity: vertex vl of the chunk, meshes half * HG + i
    const int vl = tid & (LB_CH - 1), half = tid >> 7;
    const int v = v0 + vl;
    const bool vlive = v < V;
    int idx[K];
    float w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { idx[k] = sI[vl * K + k] * 12; w[k] = sW[vl * K + k]; }
    // the vertex's regressor entries: the first two in registers (SMPL: 276 entries on 198 vertices), the rest read when used
    int ce0 = 0, ce1 = 0, row0 = 0, row1 = 0;
    float val0 = 0.0f, val1 = 0.0f;
    if (gJ && vlive) {
        ce0 = ct_ptr[v]; ce1 = ct_ptr[v + 1];
        if (ce1 > ce0) { row0 = ct_row[ce0] * 3; val0 = ct_val[ce0]; }
        if (ce1 > ce0 + 1) { row1 = ct_row[ce0 + 1] * 3; val1 = ct_val[ce0 + 1]; }
    }

    // phase 2 identity: column il = mesh (il / 12) of the wave's pair, entry e = il % 12 = 4 r + c of the 3 x 4 transform
    const bool cvalid = il < 24;
    const int cm = cvalid ? il / 12 : 0, ce = cvalid ? il % 12 : 0;
    const float* gsrc = &sGv[2 * wave + cm][kl][ce >> 2];
    const float* psrc = &sP[2 * wave + cm][kl][ce & 3];
    const float cmask = cvalid ? 1.0f : 0.0f;

    // one group's inputs in registers, requested a group ahead
    f3 rg[HG], rp[HG];
    float4 ra[AQ];
    float rj[JQ];
    auto request = [&](int grp) {
        const int m0 = grp * LB_G;
        const int n4 = min(LB_G, M - m0) * a_stride >> 2;
        const float4* asrc = reinterpret_cast<const float4*>(a + (size_t)m0 * a_stride);
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int i = tid + 256 * q;
            ra[q] = i < n4 ? asrc[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < HG; ++i) {
            const int m = min(m0 + half * HG + i, M - 1);            // clamp: loads stay in range, uses are predicated
            const int vc = vlive ? v : V - 1;
            rp[i] = reinterpret_cast<const f3*>(vp_in + (size_t)m * ld)[vc];
            if (gV) rg[i] = reinterpret_cast<const f3*>(gV)[(size_t)m * V + vc];
            else { rg[i].x = 0.f; rg[i].y = 0.f; rg[i].z = 0.f; }
        }
        if (gJ) {                                                    // 32 lanes per mesh: its n_rows x 3 contiguous floats
            const float* src = gJ + (size_t)min(m0 + (tid >> 5), M - 1) * gj_pitch + J * 3;
#pragma unroll
            for (int q = 0; q < JQ; ++q) {
                const int j = (tid & 31) + 32 * q;
                rj[q] = j < n_rows * 3 ? src[j] : 0.0f;
            }
        }
    };

    request(g_begin);
    for (int grp = g_begin; grp < g_end; ++grp) {
        const int m0 = grp * LB_G;
        const int nm = min(LB_G, M - m0);
        __syncthreads();       // every wave is through the previous group's phase 2 (and, the first time, through the weights in LDS)
#pragma unroll
        for (int q = 0; q < AQ; ++q) reinterpret_cast<float4*>(sA)[tid + 256 * q] = ra[q];
        if (gJ) {
#pragma unroll
            for (int q = 0; q < JQ; ++q) sGJ[tid >> 5][(tid & 31) + 32 * q] = rj[q];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < HG; ++i) {
            const int ml = half * HG + i, m = m0 + ml;
            const bool on = vlive && m < M;
            float gx = rg[i].x, gy = rg[i].y, gz = rg[i].z;
            if (ce1 > ce0) {                                         // + C^T g_joints, entries in row order (few vertices carry any)
                const float* s0 = &sGJ[ml][row0];
                gx = __builtin_fmaf(val0, s0[0], gx); gy = __builtin_fmaf(val0, s0[1], gy); gz = __builtin_fmaf(val0, s0[2], gz);
                if (ce1 > ce0 + 1) {
                    const float* s1 = &sGJ[ml][row1];
                    gx = __builtin_fmaf(val1, s1[0], gx); gy = __builtin_fmaf(val1, s1[1], gy); gz = __builtin_fmaf(val1, s1[2], gz);
                }
                for (int e = ce0 + 2; e < ce1; ++e) {
                    const float cv = ct_val[e];
                    const float* se = &sGJ[ml][ct_row[e] * 3];
                    gx = __builtin_fmaf(cv, se[0], gx); gy = __builtin_fmaf(cv, se[1], gy); gz = __builtin_fmaf(cv, se[2], gz);
                }
            }
            if (!on) { gx = 0.f; gy = 0.f; gz = 0.f; }
            const float* Am = sA + ml * a_stride;
            float T[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float4* A4 = reinterpret_cast<const float4*>(Am + idx[k]);
                const float4 r0 = A4[0], r1 = A4[1], r2 = A4[2];
                T[0] = __builtin_fmaf(w[k], r0.x, T[0]); T[1] = __builtin_fmaf(w[k], r0.y, T[1]); T[2] = __builtin_fmaf(w[k], r0.z, T[2]);
                T[3] = __builtin_fmaf(w[k], r1.x, T[3]); T[4] = __builtin_fmaf(w[k], r1.y, T[4]); T[5] = __builtin_fmaf(w[k], r1.z, T[5]);
                T[6] = __builtin_fmaf(w[k], r2.x, T[6]); T[7] = __builtin_fmaf(w[k], r2.y, T[7]); T[8] = __builtin_fmaf(w[k], r2.z, T[8]);
            }
            if (on) {
                f3 o;
                o.x = __builtin_fmaf(T[6], gz, __builtin_fmaf(T[3], gy, T[0] * gx));
                o.y = __builtin_fmaf(T[7], gz, __builtin_fmaf(T[4], gy, T[1] * gx));
                o.z = __builtin_fmaf(T[8], gz, __builtin_fmaf(T[5], gy, T[2] * gx));
                reinterpret_cast<f3*>(vp_out + (size_t)m * ld)[v] = o;
            }
            *reinterpret_cast<float4*>(&sGv[ml][vl][0]) = make_float4(gx, gy, gz, 0.0f);
            *reinterpret_cast<float4*>(&sP[ml][vl][0]) = make_float4(on ? rp[i].x : 0.f, on ? rp[i].y : 0.f, on ? rp[i].z : 0.f, on ? 1.0f : 0.f);
        }
        // the padding behind the last vertex of every row (the blend backward multiplies it with the zero columns of bmat)
        if (chunk == (int)gridDim.x - 1) {
            const int npad = ld - 3 * V;
            for (int i = tid; i < nm * npad; i += 256) vp_out[(size_t)(m0 + i / npad) * ld + 3 * V + i % npad] = 0.0f;
        }
        if (grp + 1 < g_end) request(grp + 1);     // in flight under the MFMA phase
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < LB_CH / 2; ++s) {
            const float b = gsrc[s * 8] * psrc[s * 8] * cmask;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sRow[s][lane], b, acc, 0, 0, 0);
        }
        const int m = m0 + 2 * wave + cm;
        if (cvalid && m < M) {
            float* dst = partials + ((size_t)chunk * M + m) * (size_t)(J * 12 + n_ones * 3);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * kl;
                if (row < J) dst[row * 12 + ce] = acc[r];
                else if ((ce & 3) == 3) dst[J * 12 + (row - J) * 3 + (ce >> 2)] = acc[r];
            }
        }
    }
}

// g_A[m][j][e] = sum over chunks, in chunk order; the ones rows' translation columns (+ the kinematic joints' cotangents) -> g_transl
__global__ __launch_bounds__(256) void lbs_backward_finish_kernel(const float* __restrict__ partials, int n_chunks,
                                                                  float* __restrict__ gA, float* __restrict__ g_transl,
                                                                  const float* __restrict__ gJ, int gj_pitch, int M, int J) {
    const int n_ones = 32 - J, per = J * 12 + n_ones * 3, outs = J * 12 + 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)M * outs) return;
    const int m = (int)(i / outs), e = (int)(i % outs);
    if (e < J * 12) {
        float s = 0.0f;
#pragma unroll 8                               // (eight loads in flight; the additions stay in chunk order)
        for (int c = 0; c < n_chunks; ++c) s += partials[((size_t)c * M + m) * per + e];
        gA[(size_t)m * J * 12 + e] = s;
    } else if (g_transl) {
        const int c3 = e - J * 12;
        double s = 0.0;
#pragma unroll 2
        for (int c = 0; c < n_chunks; ++c) {
#pragma unroll 8
            for (int t = 0; t < n_ones; ++t) s += (double)partials[((size_t)c * M + m) * per + J * 12 + t * 3 + c3];
        }
        if (gJ)
            for (int j = 0; j < J; ++j) s += (double)gJ[(size_t)m * gj_pitch + j * 3 + c3];
        g_transl[(size_t)m * 3 + c3] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------
// Blend backward:  g_xt[k, m] = sum_n bmat[k, n] g[m, n].  Both operands are contiguous along the contracted axis, so a chunk of
// either is rows of BB_BK floats that go to LDS with a pitch of 36 floats: every lane then reads its v_mfma_f32_32x32x2_f32
// fragments as conflict-free 16-byte rows (lane (i, kl) holds n = 8 q + 4 kl .. + 3 of row i: four MFMA steps per read; the
// assignment of n to the instruction's two k slots is free as long as both operands use the same one).
// Workgroup tile: up to 224 rows of bmat (7 MFMA tiles) x 128 meshes (wave = 32 meshes), one slice of BB_SL columns: the
// contraction is cut into slices of a FIXED length, whatever M, and blend_backward_reduce_kernel adds the slices in slice order.
// Next chunk's operands are fetched into registers under this chunk's 112 MFMAs per wave.
// ---------------------------------------------------------------------------------------------
constexpr int BB_SL = 512, BB_BK = 32, BB_LD = 36, BB_ROWS = 224, BB_RT = BB_ROWS / 32, BB_BM = 128;

__global__ __launch_bounds__(256) void blend_backward_kernel(const float* __restrict__ bmat, const float* __restrict__ g,
                                                             float* __restrict__ partials, int M, int kp, int mp, int np,
                                                             int ld_g) {
    __shared__ __attribute__((aligned(16))) float sB[BB_ROWS][BB_LD];
    __shared__ __attribute__((aligned(16))) float sG[BB_BM][BB_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int il = lane & 31, kl = lane >> 5;
    const int m0 = blockIdx.x * BB_BM, slice = blockIdx.y, row0 = blockIdx.z * BB_ROWS;
    const int n_begin = slice * BB_SL, n_end = min(np, n_begin + BB_SL);
    const int nchunks = (n_end - n_begin) / BB_BK;

    // staging: a chunk row is 8 float4; thread t moves float4 (t & 7) of rows (t >> 3) + 32 i
    const int sc = (tid & 7) * 4, sr = tid >> 3;
    float4 rb[BB_RT], rg[BB_BM / 32];
    auto fetch = [&](int n0) {
#pragma unroll
        for (int i = 0; i < BB_RT; ++i) {
            const int row = row0 + sr + 32 * i;
            rb[i] = row < kp ? *reinterpret_cast<const float4*>(bmat + (size_t)row * np + n0 + sc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < BB_BM / 32; ++i) {
            const int m = m0 + sr + 32 * i;
            rg[i] = m < M ? *reinterpret_cast<const float4*>(g + (size_t)m * ld_g + n0 + sc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };

    f32x16 acc[BB_RT];
#pragma unroll
    for (int t = 0; t < BB_RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    fetch(n_begin);
    for (int c = 0; c < nchunks; ++c) {
        __syncthreads();                       // every wave has read the previous chunk
#pragma unroll
        for (int i = 0; i < BB_RT; ++i) *reinterpret_cast<float4*>(&sB[sr + 32 * i][sc]) = rb[i];
#pragma unroll
        for (int i = 0; i < BB_BM / 32; ++i) *reinterpret_cast<float4*>(&sG[sr + 32 * i][sc]) = rg[i];
        __syncthreads();
        if (c + 1 < nchunks) fetch(n_begin + (c + 1) * BB_BK);
#pragma unroll
        for (int q = 0; q < BB_BK / 8; ++q) {
            const float4 gv = *reinterpret_cast<const float4*>(&sG[wave * 32 + il][8 * q + 4 * kl]);
            float4 bv[BB_RT];
#pragma unroll
            for (int t = 0; t < BB_RT; ++t) bv[t] = *reinterpret_cast<const float4*>(&sB[32 * t + il][8 * q + 4 * kl]);
#pragma unroll
            for (int t = 0; t < BB_RT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].x, gv.x, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].y, gv.y, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].z, gv.z, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv[t].w, gv.w, acc[t], 0, 0, 0);
            }
        }
    }
    // C layout of a 32 x 32 tile: column (mesh) = lane & 31, row (k) = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int m = m0 + wave * 32 + il;
#pragma unroll
    for (int t = 0; t < BB_RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = row0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * kl;
            if (row < kp) partials[((size_t)slice * kp + row) * mp + m] = acc[t][r];
        }
}

__global__ __launch_bounds__(256) void blend_backward_reduce_kernel(const float* __restrict__ partials, float* __restrict__ g_xt,
                                                                    int n_slices, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int c = 0; c < n_slices; ++c) s += partials[(size_t)c * n + i];
    g_xt[i] = s;
}

// ---------------------------------------------------------------------------------------------
// Pose prep backward: 32 lanes per mesh (lane = joint), 8 meshes per workgroup, like pose_prep_kernel, whose forward it recomputes
// (rotations, rest joints, world transforms).  Then, with g_G the cotangent of a joint's world transform [G.R | G.t]:
//   A.R = G.R, A.t = G.t - G.R J, posed = G.t          g_G.R = g_A.R - g_A.t (x) J,  g_G.t = g_A.t + g_posed,  g_J = -G.R^T g_A.t
//   G.R = Gp.R R, G.t = Gp.R rel + Gp.t  (leaves -> root, one level per step; a parent adds its children in index order)
//                                                      g_R = Gp.R^T g_G.R,  g_rel = Gp.R^T g_G.t,
//                                                      g_Gp.R += g_G.R R^T + g_G.t (x) rel,  g_Gp.t += g_G.t
//   rel = J - J_parent                                 g_J += g_rel - sum over children g_rel_child
//   pose feature row nb + 9 (j - 1) + e = R_j[e] - I   g_R += g_xt rows
//   J = j_template + j_shapedirs beta                  g_betas = g_xt[:nb] + j_shapedirs^T g_J
// and, for axis-angle input, through smplx batch_rodrigues with its angle = ||r + 1e-8|| (finite at r = 0: sin(angle) / angle).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pose_prep_backward_kernel(
    const float* __restrict__ glob, const float* __restrict__ body, int is_rotmat, const float* __restrict__ betas, int nb,
    const float* __restrict__ j_template, const float* __restrict__ j_shapedirs, const int32_t* __restrict__ parents,
    const int32_t* __restrict__ depth, int J, const float* __restrict__ gA, const float* __restrict__ gJ, int gj_pitch,
    const float* __restrict__ g_xt, int mp, float* __restrict__ g_glob, float* __restrict__ g_body, float* __restrict__ g_betas,
    int M) {
    __shared__ float sG[8][BWD_MAXJ][12];   // world transforms
    __shared__ float sJ[8][BWD_MAXJ][3];    // rest joints, later their cotangents
    __shared__ float sC[8][BWD_MAXJ][12];   // a joint's contribution to its parent's g_G
    __shared__ float sRel[8][BWD_MAXJ][3];  // g_rel
    __shared__ float sBeta[8][16];
    __shared__ int sPar[BWD_MAXJ];

    const int g = threadIdx.x >> 5, j = threadIdx.x & 31;
    const int m = blockIdx.x * 8 + g;
    const bool live = (m < M) && (j < J);

    if (m < M && j < nb && j < 16) sBeta[g][j] = betas[(size_t)m * nb + j];
    if (threadIdx.x < BWD_MAXJ) sPar[threadIdx.x] = threadIdx.x < J ? parents[threadIdx.x] : -2;
    __syncthreads();

    float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    float Jr[3] = {0.f, 0.f, 0.f};
    float rv[3] = {0.f, 0.f, 0.f};
    int par = -1, dep = 0;
    if (live) {
        par = sPar[j];
        dep = depth[j];
        if (is_rotmat) {
            const float* src = (j == 0) ? glob + (size_t)m * 9 : body + ((size_t)m * (J - 1) + (j - 1)) * 9;
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = src[e];
        } else {
            const float* src = (j == 0) ? glob + (size_t)m * 3 : body + ((size_t)m * (J - 1) + (j - 1)) * 3;
            rv[0] = src[0]; rv[1] = src[1]; rv[2] = src[2];
            rodrigues_dev(rv[0], rv[1], rv[2], R);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = j_template[j * 3 + c];
            for (int l = 0; l < nb; ++l) acc += j_shapedirs[(j * 3 + c) * nb + l] * sBeta[g][l];
            Jr[c] = acc;
            sJ[g][j][c] = acc;
        }
    }
    int max_depth = (j < J) ? depth[j] : 0;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) max_depth = max(max_depth, __shfl_xor(max_depth, d));
    max_depth = __builtin_amdgcn_readfirstlane(max_depth);
    __syncthreads();

    // forward chain (pose_prep_kernel's arithmetic)
    float T[12], rel[3] = {Jr[0], Jr[1], Jr[2]};
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.0f;
    if (live) {
        if (par >= 0) { rel[0] -= sJ[g][par][0]; rel[1] -= sJ[g][par][1]; rel[2] -= sJ[g][par][2]; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            T[r * 4 + 0] = R[r * 3 + 0]; T[r * 4 + 1] = R[r * 3 + 1]; T[r * 4 + 2] = R[r * 3 + 2];
            T[r * 4 + 3] = rel[r];
        }
        if (dep == 0) {
#pragma unroll
            for (int e = 0; e < 12; ++e) sG[g][j][e] = T[e];
        }
    }
    for (int lvl = 1; lvl <= max_depth; ++lvl) {
        __syncthreads();
        if (live && dep == lvl) {
            float P[12], Gn[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) P[e] = sG[g][par][e];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Gn[r * 4 + c] = P[r * 4 + 0] * T[0 * 4 + c] + P[r * 4 + 1] * T[1 * 4 + c] + P[r * 4 + 2] * T[2 * 4 + c];
                Gn[r * 4 + 3] = P[r * 4 + 0] * T[3] + P[r * 4 + 1] * T[7] + P[r * 4 + 2] * T[11] + P[r * 4 + 3];
            }
#pragma unroll
            for (int e = 0; e < 12; ++e) { T[e] = Gn[e]; sG[g][j][e] = Gn[e]; }
        }
    }
    __syncthreads();
    // T = world transform G_j.  Own cotangent: g_G (3 x 4, row-major like T) and the direct part of g_J
    float gG[12], gJr[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 12; ++e) gG[e] = 0.0f;
    if (live) {
        const float* ga = gA + ((size_t)m * J + j) * 12;
        float gt[3] = {ga[3], ga[7], ga[11]};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) gG[r * 4 + c] = ga[r * 4 + c] - gt[r] * Jr[c];
            gG[r * 4 + 3] = gt[r] + (gJ ? gJ[(size_t)m * gj_pitch + j * 3 + r] : 0.0f);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gJr[c] = -(T[0 * 4 + c] * gt[0] + T[1 * 4 + c] * gt[1] + T[2 * 4 + c] * gt[2]);
    }
    // leaves -> root
    float gR[9], grel[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 9; ++e) gR[e] = 0.0f;
    for (int lvl = max_depth; lvl >= 0; --lvl) {
        if (live && dep == lvl) {
            if (lvl < max_depth) {       // the children (level lvl + 1) have written their contributions
                for (int c = 0; c < J; ++c)
                    if (sPar[c] == j) {
#pragma unroll
                        for (int e = 0; e < 12; ++e) gG[e] += sC[g][c][e];
                    }
            }
            if (par >= 0) {
                float P[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) P[e] = sG[g][par][e];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        gR[r * 3 + c] = P[0 * 4 + r] * gG[0 * 4 + c] + P[1 * 4 + r] * gG[1 * 4 + c] + P[2 * 4 + r] * gG[2 * 4 + c];
                    grel[r] = P[0 * 4 + r] * gG[3] + P[1 * 4 + r] * gG[7] + P[2 * 4 + r] * gG[11];
                }
                // to the parent: g_G.R R^T + g_G.t (x) rel | g_G.t
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        sC[g][j][r * 4 + c] = gG[r * 4 + 0] * R[c * 3 + 0] + gG[r * 4 + 1] * R[c * 3 + 1] + gG[r * 4 + 2] * R[c * 3 + 2] +
                                              gG[r * 4 + 3] * rel[c];
                    sC[g][j][r * 4 + 3] = gG[r * 4 + 3];
                }
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) gR[r * 3 + c] = gG[r * 4 + c];
                    grel[r] = gG[r * 4 + 3];
                }
            }
        }
        __syncthreads();
    }
    if (live) {
        sRel[g][j][0] = grel[0]; sRel[g][j][1] = grel[1]; sRel[g][j][2] = grel[2];
    }
    __syncthreads();
    if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) gJr[c] += grel[c];
        for (int c = 0; c < J; ++c)
            if (sPar[c] == j) { gJr[0] -= sRel[g][c][0]; gJr[1] -= sRel[g][c][1]; gJr[2] -= sRel[g][c][2]; }
        sJ[g][j][0] = gJr[0]; sJ[g][j][1] = gJr[1]; sJ[g][j][2] = gJr[2];
        // pose feature rows of the blend operand
        if (j >= 1 && g_xt) {
#pragma unroll
            for (int e = 0; e < 9; ++e) gR[e] += g_xt[(size_t)(nb + 9 * (j - 1) + e) * mp + m];
        }
        float* dst;
        if (is_rotmat) {
            dst = (j == 0) ? g_glob + (size_t)m * 9 : g_body + ((size_t)m * (J - 1) + (j - 1)) * 9;
            if ((j == 0) ? (g_glob != nullptr) : (g_body != nullptr)) {
#pragma unroll
                for (int e = 0; e < 9; ++e) dst[e] = gR[e];
            }
        } else if ((j == 0) ? (g_glob != nullptr) : (g_body != nullptr)) {
            dst = (j == 0) ? g_glob + (size_t)m * 3 : g_body + ((size_t)m * (J - 1) + (j - 1)) * 3;
            // R = I + s K + c K K, K = [d]_x, d = r / angle, angle = ||r + 1e-8||, s = sin(angle), c = 1 - cos(angle)
            const float ex = rv[0] + 1e-8f, ey = rv[1] + 1e-8f, ez = rv[2] + 1e-8f;
            const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
            const float dx = rv[0] / angle, dy = rv[1] / angle, dz = rv[2] / angle;
            const float s = sinf(angle), co = cosf(angle), c = 1.0f - co;
            const float k[9] = {0.f, -dz, dy, dz, 0.f, -dx, -dy, dx, 0.f};
            float k2[9];
            mat3_mul(k, k, k2);
            float gs = 0.f, gc = 0.f;
#pragma unroll
            for (int e = 0; e < 9; ++e) { gs += gR[e] * k[e]; gc += gR[e] * k2[e]; }
            // g_K = s g_R + c (g_R K^T + K^T g_R)
            float gk[9];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int cc = 0; cc < 3; ++cc) {
                    float t = 0.f;
#pragma unroll
                    for (int q = 0; q < 3; ++q) t += gR[r * 3 + q] * k[cc * 3 + q] + k[q * 3 + r] * gR[q * 3 + cc];
                    gk[r * 3 + cc] = s * gR[r * 3 + cc] + c * t;
                }
            const float gd[3] = {gk[7] - gk[5], gk[2] - gk[6], gk[3] - gk[1]};
            float g_angle = gs * co + gc * s;
            g_angle -= (gd[0] * rv[0] + gd[1] * rv[1] + gd[2] * rv[2]) / (angle * angle);
            dst[0] = gd[0] / angle + g_angle * (ex / angle);
            dst[1] = gd[1] / angle + g_angle * (ey / angle);
            dst[2] = gd[2] / angle + g_angle * (ez / angle);
        }
    }
    __syncthreads();
    if (m < M && g_betas && j < nb) {
        float acc = g_xt ? g_xt[(size_t)j * mp + m] : 0.0f;
        for (int q = 0; q < J; ++q)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc += j_shapedirs[(q * 3 + c) * nb + j] * sJ[g][q][c];
        g_betas[(size_t)m * nb + j] = acc;
    }
}

int64_t lbs_backward_ws_bytes(int64_t M, int64_t V, int64_t J) {
    return ((V + LB_CH - 1) / LB_CH) * M * (J * 12 + (32 - J) * 3) * (int64_t)sizeof(float);
}
int64_t blend_backward_ws_bytes(int64_t M, int64_t kp, int64_t np) {
    return ((np + BB_SL - 1) / BB_SL) * kp * ((M + 127) / 128 * 128) * (int64_t)sizeof(float);
}

template <int K>
static int launch_lbs_backward(float* v_posed, int ld, const float* a, const int32_t* w_idx, const float* w_val, int J,
                               const float* gV, const float* gJ, int gj_pitch, const int32_t* ct_ptr, const int32_t* ct_row,
                               const float* ct_val, float* ws, int M, int V, hipStream_t s) {
    const int n_chunks = ceil_div(V, LB_CH), n_groups = ceil_div(M, LB_G);
    // about eight workgroups per CU when there are that many mesh groups (each keeps its vertex chunk and walks its meshes)
    int splits = ceil_div(2048, n_chunks);
    if (splits > n_groups) splits = n_groups;
    if (splits > 65535) splits = 65535;
    const int gpb = ceil_div(n_groups, splits);
    hipLaunchKernelGGL(lbs_backward_kernel<K>, dim3(n_chunks, ceil_div(n_groups, gpb)), dim3(256), 0, s, v_posed, v_posed, ld, a, w_idx, w_val,
                       J, gV, gJ, gj_pitch, ct_ptr, ct_row, ct_val, ws, M, V, gpb, gj_pitch / 3 - J);
    return check_launch("hps_smpl_lbs_backward");
}

}  // namespace hps

using namespace hps;

extern "C" int hps_smpl_lbs_backward(float* v_posed, int ld_vposed, const float* a, const int32_t* w_idx, const float* w_val,
                                     int K, int num_joints, const float* g_verts, const float* g_joints, int n_rows,
                                     const int32_t* csrt_ptr, const int32_t* csrt_row, const float* csrt_val, float* g_a,
                                     float* g_transl, float* workspace, int M, int V, hps_stream_t stream) {
    if (!v_posed || !a || !w_idx || !w_val || !g_a || !workspace) return bad_arg("hps_smpl_lbs_backward: null pointer");
    if (!g_verts && !g_joints) return bad_arg("hps_smpl_lbs_backward: neither g_verts nor g_joints");
    if (g_joints && (!csrt_ptr || !csrt_row || !csrt_val || n_rows < 0))
        return bad_arg("hps_smpl_lbs_backward: g_joints needs the transposed CSR matrix");
    if (num_joints < 1 || num_joints >= BWD_MAXJ) return bad_arg("hps_smpl_lbs_backward: num_joints must be 1..31");
    if (g_joints && n_rows > LB_MAXR) {
        set_error("hps_smpl_lbs_backward: at most %d regressor rows (got %d)", LB_MAXR, n_rows);
        return HPS_E_UNSUPPORTED;
    }
    if (V <= 0 || ld_vposed < 3 * V) return bad_arg("hps_smpl_lbs_backward: ld_vposed < 3 V");
    if (M <= 0) return HPS_OK;
    const int pitch = (num_joints + n_rows) * 3;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    switch (K) {
        case 4: rc = launch_lbs_backward<4>(v_posed, ld_vposed, a, w_idx, w_val, num_joints, g_verts, g_joints, pitch, csrt_ptr, csrt_row, csrt_val, workspace, M, V, s); break;
        case 8: rc = launch_lbs_backward<8>(v_posed, ld_vposed, a, w_idx, w_val, num_joints, g_verts, g_joints, pitch, csrt_ptr, csrt_row, csrt_val, workspace, M, V, s); break;
        case 12: rc = launch_lbs_backward<12>(v_posed, ld_vposed, a, w_idx, w_val, num_joints, g_verts, g_joints, pitch, csrt_ptr, csrt_row, csrt_val, workspace, M, V, s); break;
        case 24: rc = launch_lbs_backward<24>(v_posed, ld_vposed, a, w_idx, w_val, num_joints, g_verts, g_joints, pitch, csrt_ptr, csrt_row, csrt_val, workspace, M, V, s); break;
        default:
            set_error("hps_smpl_lbs_backward: K must be 4, 8, 12 or 24 (got %d)", K);
            return HPS_E_UNSUPPORTED;
    }
    if (rc != HPS_OK) return rc;
    const size_t n = (size_t)M * (num_joints * 12 + 3);
    hipLaunchKernelGGL(lbs_backward_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, workspace, ceil_div(V, LB_CH),
                       g_a, g_transl, g_joints, pitch, M, num_joints);
    return check_launch("hps_smpl_lbs_backward");
}

extern "C" int hps_smpl_blend_backward(const float* bmat, const float* g_vposed, float* g_xt, float* workspace, int M, int kp,
                                       int mp, int np, int ld_g, hps_stream_t stream) {
    if (!bmat || !g_vposed || !g_xt || !workspace) return bad_arg("hps_smpl_blend_backward: null pointer");
    if (kp <= 0 || kp % 16 != 0) return bad_arg("hps_smpl_blend_backward: kp must be a positive multiple of 16");
    if (mp % BB_BM != 0 || mp < M || np <= 0 || np % 128 != 0)
        return bad_arg("hps_smpl_blend_backward: mp/np must be multiples of 128, mp covering M");
    if (ld_g < np || ld_g % 4 != 0) return bad_arg("hps_smpl_blend_backward: ld_g must be a multiple of 4 and >= np");
    if ((((size_t)bmat | (size_t)g_vposed) & 15) != 0) return bad_arg("hps_smpl_blend_backward: operands must be 16-byte aligned");
    if (M <= 0) return HPS_OK;
    // (the reduction reads every column of the partial sums: the started 128-mesh tiles must be all of mp)
    if (ceil_div(M, BB_BM) * BB_BM != mp) return bad_arg("hps_smpl_blend_backward: mp must be M rounded up to 128");
    const int n_slices = ceil_div(np, BB_SL);
    if (n_slices > 65535) return bad_arg("hps_smpl_blend_backward: np too large");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(blend_backward_kernel, dim3(ceil_div(M, BB_BM), n_slices, ceil_div(kp, BB_ROWS)), dim3(256), 0, s, bmat,
                       g_vposed, workspace, M, kp, mp, np, ld_g);
    int rc = check_launch("hps_smpl_blend_backward");
    if (rc != HPS_OK) return rc;
    const size_t n = (size_t)kp * mp;
    hipLaunchKernelGGL(blend_backward_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, workspace, g_xt, n_slices, n);
    return check_launch("hps_smpl_blend_backward");
}

extern "C" int hps_smpl_pose_prep_backward(const float* glob, const float* body, int is_rotmat, const float* betas, int num_betas,
                                           const float* j_template, const float* j_shapedirs, const int32_t* parents,
                                           const int32_t* depth, int num_joints, const float* g_a, const float* g_joints,
                                           int n_rows, const float* g_xt, int mp, float* g_glob, float* g_body, float* g_betas,
                                           int M, hps_stream_t stream) {
    if (!glob || !body || !betas || !j_template || !j_shapedirs || !parents || !depth || !g_a)
        return bad_arg("hps_smpl_pose_prep_backward: null pointer");
    if (num_joints < 1 || num_joints > BWD_MAXJ || num_betas < 0 || num_betas > 16)
        return bad_arg("hps_smpl_pose_prep_backward: num_joints must be 1..32 and num_betas 0..16");
    if (n_rows < 0 || (g_xt && mp < M)) return bad_arg("hps_smpl_pose_prep_backward: n_rows / mp out of range");
    if (M <= 0) return HPS_OK;
    hipLaunchKernelGGL(pose_prep_backward_kernel, dim3(ceil_div(M, 8)), dim3(256), 0, (hipStream_t)stream, glob, body, is_rotmat,
                       betas, num_betas, j_template, j_shapedirs, parents, depth, num_joints, g_a, g_joints,
                       (num_joints + n_rows) * 3, g_xt, mp, g_glob, g_body, g_betas, M);
    return check_launch("hps_smpl_pose_prep_backward");
}
