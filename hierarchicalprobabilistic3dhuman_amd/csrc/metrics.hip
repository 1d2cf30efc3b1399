// Evaluation metrics on the device: per-point L2 errors between predicted and target
// point sets (6890 vertices or 14 joints), raw, after scale-and-translation correction
// (utils/eval_utils.py:70-89) or after Procrustes alignment (utils/eval_utils.py:11-59), as used by
// metrics/eval_metrics_tracker.py:89-269.  Streaming reductions: HBM bound.
//
// A "set" is one (P,3) point cloud.  pred holds S sets; set s is compared with target set s / group
// (group = 1: one target per prediction; group = N: N samples of one frame share its target).
#include "hps_common.h"

namespace hps {

constexpr int NSTAT = 17;  // sum p (3), sum t (3), sum |p|^2, sum |t|^2, sum p_a t_b (9)

// one set, one 256-thread workgroup: the 17 float64 statistics of (p, t) -> st[0 .. NSTAT).  The body of pointset_stats_kernel and of
// train_stats_kernel alike (one definition, one body of machine code -- see pointset_error_lane: the same bits).
__device__ __noinline__ void pointset_stats_set(const float* __restrict__ p, const float* __restrict__ t, int P, double* __restrict__ st) {
    double acc[NSTAT];
#pragma unroll
    for (int i = 0; i < NSTAT; ++i) acc[i] = 0.0;
    // four of the lane's points (and their targets) requested before the first is used -- 12-byte records, one dwordx3 load each;
    // the sums keep their order (same bits).  As a plain loop every point was a dependent round trip: 27 per lane for 6 890 points.
    auto add = [&](const f3 pp, const f3 tt) {
        const double px = pp.x, py = pp.y, pz = pp.z;
        const double tx = tt.x, ty = tt.y, tz = tt.z;
        acc[0] += px; acc[1] += py; acc[2] += pz;
        acc[3] += tx; acc[4] += ty; acc[5] += tz;
        acc[6] += px * px + py * py + pz * pz;
        acc[7] += tx * tx + ty * ty + tz * tz;
        acc[8] += px * tx; acc[9] += px * ty; acc[10] += px * tz;
        acc[11] += py * tx; acc[12] += py * ty; acc[13] += py * tz;
        acc[14] += pz * tx; acc[15] += pz * ty; acc[16] += pz * tz;
    };
    const f3* p3 = reinterpret_cast<const f3*>(p);
    const f3* t3 = reinterpret_cast<const f3*>(t);
    int i = threadIdx.x;
    for (; i + 3 * 256 < P; i += 4 * 256) {
        f3 pp[4], tt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { pp[q] = p3[i + q * 256]; tt[q] = t3[i + q * 256]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) add(pp[q], tt[q]);
    }
    for (; i < P; i += 256) add(p3[i], t3[i]);
    __shared__ double red[4][NSTAT];
#pragma unroll
    for (int i = 0; i < NSTAT; ++i) {
        double v = acc[i];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSTAT)
        st[threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

__global__ __launch_bounds__(256) void pointset_stats_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             int group, int P, double* __restrict__ stats) {
    const int s = blockIdx.x;
    pointset_stats_set(pred + (size_t)s * P * 3, target + (size_t)(s / group) * P * 3, P, stats + (size_t)s * NSTAT);
}

// symmetric 3x3 eigen-decomposition by cyclic Jacobi (double): A = V diag(w) V^T, columns of V
__device__ void jacobi_eig3(double A[3][3], double V[3][3], double w[3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (fabs(A[p][q]) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(tt * tt + 1.0), sn = tt * c;
                for (int k = 0; k < 3; ++k) {           // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {           // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - sn * vkq; V[k][q] = sn * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) w[i] = A[i][i];
}

// per set: similarity transform q = M p + t as 12 floats (row-major 3x4).  mode 0 identity, 1 scale+translation,
// 2 Procrustes (rotation from the SVD of K = X1 X2^T with the det fix, scale = tr(R K) / var1, t = mu2 - s R mu1).
// (one lane per set; st is read only when mode != 0)
__device__ __noinline__ void pointset_transform_set(const double* __restrict__ st, int P, int mode, float* __restrict__ o) {
    double M[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, tr[3] = {0, 0, 0};
    if (mode != 0) {
        const double n = (double)P;
        const double mp[3] = {st[0] / n, st[1] / n, st[2] / n}, mt[3] = {st[3] / n, st[4] / n, st[5] / n};
        const double var_p = st[6] - n * (mp[0] * mp[0] + mp[1] * mp[1] + mp[2] * mp[2]);
        const double var_t = st[7] - n * (mt[0] * mt[0] + mt[1] * mt[1] + mt[2] * mt[2]);
        if (mode == 1) {
            const double sc = sqrt(var_t / n) / sqrt(var_p / n);                 // eval_utils.py:80-87
            for (int i = 0; i < 3; ++i) { M[i][i] = sc; tr[i] = mt[i] - sc * mp[i]; }
        } else {
            double K[3][3];                                                     // K = X1 X2^T  (:33)
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) K[a][b] = st[8 + a * 3 + b] - n * mp[a] * mt[b];
            // SVD K = U S V^T from the eigen-decomposition of K^T K; R = V Z U^T (:37-44)
            double A[3][3], V[3][3], w[3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) A[a][b] = K[0][a] * K[0][b] + K[1][a] * K[1][b] + K[2][a] * K[2][b];
            jacobi_eig3(A, V, w);
            int o[3] = {0, 1, 2};                                               // sort eigenvalues descending
            for (int i = 0; i < 2; ++i)
                for (int j = 0; j < 2 - i; ++j)
                    if (w[o[j]] < w[o[j + 1]]) { const int tmp = o[j]; o[j] = o[j + 1]; o[j + 1] = tmp; }
            double v0[3], v1[3], v2[3], u0[3], u1[3], u2[3];
            for (int k = 0; k < 3; ++k) { v0[k] = V[k][o[0]]; v1[k] = V[k][o[1]]; }
            v2[0] = v0[1] * v1[2] - v0[2] * v1[1]; v2[1] = v0[2] * v1[0] - v0[0] * v1[2]; v2[2] = v0[0] * v1[1] - v0[1] * v1[0];
            for (int k = 0; k < 3; ++k) u0[k] = K[k][0] * v0[0] + K[k][1] * v0[1] + K[k][2] * v0[2];
            double nrm = sqrt(u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2]);
            for (int k = 0; k < 3; ++k) u0[k] /= (nrm > 0 ? nrm : 1.0);
            for (int k = 0; k < 3; ++k) u1[k] = K[k][0] * v1[0] + K[k][1] * v1[1] + K[k][2] * v1[2];
            const double d01 = u0[0] * u1[0] + u0[1] * u1[1] + u0[2] * u1[2];
            for (int k = 0; k < 3; ++k) u1[k] -= d01 * u0[k];
            nrm = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
            for (int k = 0; k < 3; ++k) u1[k] /= (nrm > 0 ? nrm : 1.0);
            u2[0] = u0[1] * u1[2] - u0[2] * u1[1]; u2[1] = u0[2] * u1[0] - u0[0] * u1[2]; u2[2] = u0[0] * u1[1] - u0[1] * u1[0];
            // with det U = det V = +1 the third "singular value" u2^T K v2 carries the sign of det K, and the
            // reference's Z = diag(1,1,sign(det(U V^T))) on a positive-singular-value SVD gives the same R: V U^T
            double R[3][3];
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) R[a][b] = v0[a] * u0[b] + v1[a] * u1[b] + v2[a] * u2[b];
            double trRK = 0.0;
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) trRK += R[a][b] * K[b][a];
            const double sc = trRK / var_p;                                     // :47
            for (int a = 0; a < 3; ++a) {
                for (int b = 0; b < 3; ++b) M[a][b] = sc * R[a][b];
                tr[a] = mt[a] - (M[a][0] * mp[0] + M[a][1] * mp[1] + M[a][2] * mp[2]);   // :50
            }
        }
    }
    for (int a = 0; a < 3; ++a) { o[a * 4] = (float)M[a][0]; o[a * 4 + 1] = (float)M[a][1]; o[a * 4 + 2] = (float)M[a][2]; o[a * 4 + 3] = (float)tr[a]; }
}

__global__ void pointset_transform_kernel(const double* __restrict__ stats, int S, int P, int mode, float* __restrict__ xf) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    pointset_transform_set(stats + (size_t)s * NSTAT, P, mode, xf + (size_t)s * 12);
}

// One lane's float64 sum over its points of || M p + t - target || for ONE transform (xf: 12 floats); optional transformed points out.
// __noinline__ on purpose, here and on the two functions above: hipcc's SLP vectoriser pairs the rows' products differently from one
// unroll slot to the next (qz as a packed multiply, a horizontal add and one FMA; qx, qy as a packed multiply and two packed FMAs in
// either operand order), so the rounding of a point depends on the code around it.  Only ONE body of machine code, called by
// pointset_error_kernel and by train_error_kernel alike, gives both the same bits.
__device__ __noinline__ double pointset_error_lane(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ xf, int P,
                                                   float* __restrict__ transformed) {
    float M[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) M[i] = xf[i];
    double acc = 0.0;
    const f3* p3 = reinterpret_cast<const f3*>(p);
    const f3* t3 = reinterpret_cast<const f3*>(t);
    auto one = [&](int i, const f3 pp, const f3 tt) {
        const float px = pp.x, py = pp.y, pz = pp.z;
        const float qx = M[0] * px + M[1] * py + M[2] * pz + M[3];
        const float qy = M[4] * px + M[5] * py + M[6] * pz + M[7];
        const float qz = M[8] * px + M[9] * py + M[10] * pz + M[11];
        if (transformed) {
            float* o = transformed + (size_t)i * 3;
            o[0] = qx; o[1] = qy; o[2] = qz;
        }
        const float dx = qx - tt.x, dy = qy - tt.y, dz = qz - tt.z;
        acc += (double)sqrtf(dx * dx + dy * dy + dz * dz);
    };
    // four points in flight per lane (see pointset_stats_set); same order of additions
    int i = threadIdx.x;
    for (; i + 3 * 256 < P; i += 4 * 256) {
        f3 pp[4], tt[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { pp[q] = p3[i + q * 256]; tt[q] = t3[i + q * 256]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) one(i + q * 256, pp[q], tt[q]);
    }
    for (; i < P; i += 256) one(i, p3[i], t3[i]);
    return acc;
}

// per set, one 256-thread workgroup: the error sums of NM transforms (xf: NM consecutive 3x4 matrices) -- pointset_error_kernel's body
// with NM = 1, train_error_kernel's with NM = 3 (raw, SC and PA of one set in one workgroup: the set comes from HBM once, the second
// and third walk find it in the cache).  Each transform's lane sums are reduced by the same tree.
template <int NM>
__device__ __forceinline__ void pointset_error_set(const float* __restrict__ p, const float* __restrict__ t, const float* __restrict__ xf,
                                                   int P, double (&sum)[NM], float* __restrict__ transformed) {
    double acc[NM];
    for (int m = 0; m < NM; ++m) acc[m] = pointset_error_lane(p, t, xf + m * 12, P, m == 0 ? transformed : nullptr);
    __shared__ double red[NM][4];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        double v = acc[m];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[m][threadIdx.x >> 6] = v;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < NM; ++m) sum[m] = red[m][0] + red[m][1] + red[m][2] + red[m][3];      // meaningful in lane 0
}

__global__ __launch_bounds__(256) void pointset_error_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const float* __restrict__ xf, int group, int P,
                                                             double* __restrict__ err_sum, float* __restrict__ transformed) {
    const int s = blockIdx.x;
    double sum[1];
    pointset_error_set<1>(pred + (size_t)s * P * 3, target + (size_t)(s / group) * P * 3, xf + (size_t)s * 12, P, sum,
                          transformed ? transformed + (size_t)s * P * 3 : nullptr);
    if (threadIdx.x == 0) err_sum[s] = sum[0];
}

// ---- float64 sums of float tensors (result checksums): two launches for up to four tensors, fixed summation order ----
constexpr int SUM_BLOCKS = 128;
struct SumJobs {
    const float* x[4];
    long n[4];
    int take_abs[4];
};

// block (b, j): elements b * 256 + t, + SUM_BLOCKS * 256, ... of tensor j, each lane in index order, then a fixed tree
__global__ __launch_bounds__(256) void sums_partial_kernel(const SumJobs jobs, double* __restrict__ partial) {
    const int j = blockIdx.y;
    const float* x = jobs.x[j];
    const long n = jobs.n[j];
    const bool a = jobs.take_abs[j] != 0;
    double acc = 0.0;
    // eight of the lane's elements requested before the first is added (the additions stay in index order: the same bits).  As a
    // plain loop every element was a dependent L2 round trip: 53 of them per lane for bench.py's largest tensor, 23-64 us per step
    // inside the timed loop for 14 MB of reads.
    constexpr long STRIDE = (long)SUM_BLOCKS * 256;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 7 * STRIDE < n; i += 8 * STRIDE) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = x[i + q * STRIDE];
#pragma unroll
        for (int q = 0; q < 8; ++q) acc += (double)(a ? fabsf(v[q]) : v[q]);
    }
    for (; i < n; i += STRIDE) {
        const float v = x[i];
        acc += (double)(a ? fabsf(v) : v);
    }
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[j * SUM_BLOCKS + blockIdx.x] = red[0];
}

__global__ void sums_final_kernel(const double* __restrict__ partial, int count, double first, double* __restrict__ out,
                                  double* __restrict__ accumulate) {
    const int j = threadIdx.x;
    if (j == 0) {
        out[0] = first;
        if (accumulate) accumulate[0] += first;
    }
    if (j < count) {
        double t = 0.0;
        for (int b = 0; b < SUM_BLOCKS; ++b) t += partial[j * SUM_BLOCKS + b];
        out[1 + j] = t;
        if (accumulate) accumulate[1 + j] += t;       // one lane per entry: running total = total + this call's sum, as a caller's add would form it
    }
}

// ---- training loss-and-metrics tracker (metrics/train_loss_and_metrics_tracker.py:113-196): hps_train_metrics_update ----
// Families: 0 vertices (PVE, PVE-SC, PVE-PA), 1 reposed vertices (PVE-T, PVE-T-SC), 2 joints (MPJPE, MPJPE-SC, MPJPE-PA); gridDim.y of
// the error launch has a fourth row for the 2-D joints.  Workspace, B = args.B:
//   double stats[3][B][17] | double part[3][B][3] (family, set, mode) | double j2d[B][3] (L2E, samples L2E, visible count) |
//   float xf[3][B][3][12]
constexpr int TM_FAMILIES = 3;
constexpr int TM_WS_DOUBLES = TM_FAMILIES * NSTAT + TM_FAMILIES * 3 + 3;      // per set
constexpr int TM_WS_FLOATS = TM_FAMILIES * 3 * 12;                            // per set
constexpr int TM_SRC = 12;                                                    // ten metric columns, the visible count, the status words

int64_t train_metrics_ws_bytes(int64_t B) { return B * (TM_WS_DOUBLES * (int64_t)sizeof(double) + TM_WS_FLOATS * (int64_t)sizeof(float)); }

struct TrainMetrics {
    const float* pred[TM_FAMILIES];
    const float* target[TM_FAMILIES];
    int points[TM_FAMILIES];
    int modes[TM_FAMILIES];          // bit m: mode m (raw, SC, PA) of the family is tracked
    const float *pred_j2d, *target_j2d, *pred_j2d_samples;
    const uint8_t* vis;
    const float* loss;
    const int32_t* status;
    int B, K, N, num_status, batch_size, mask, split;
    float img_wh;
    double *stats, *part, *j2d, *sums;
    float* xf;
};

__global__ __launch_bounds__(256) void train_stats_kernel(const TrainMetrics a) {
    const int s = blockIdx.x, f = blockIdx.y;
    if (!(a.modes[f] & 6)) return;                           // neither SC nor PA: nobody reads the statistics (uniform per workgroup)
    const int P = a.points[f];
    pointset_stats_set(a.pred[f] + (size_t)s * P * 3, a.target[f] + (size_t)s * P * 3, P, a.stats + ((size_t)f * a.B + s) * NSTAT);
}

// one lane per (family, set, mode): the mode's transform where it is tracked, the identity where it is not (the error pass applies three)
__global__ void train_transform_kernel(const TrainMetrics a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)TM_FAMILIES * a.B * 3) return;
    const int m = (int)(i % 3), f = (int)(i / 3 / a.B);
    const long fs = i / 3;                                   // f * B + s
    if (!a.modes[f]) return;
    pointset_transform_set(a.stats + (size_t)fs * NSTAT, a.points[f], (a.modes[f] >> m & 1) ? m : 0, a.xf + (size_t)i * 12);
}

// undo_keypoint_normalisation (utils/joints2d_utils.py:9) and the distance to the target, fp32
__device__ __forceinline__ float j2d_error(const float* __restrict__ pn, const float* __restrict__ tg, float half_wh) {
    const float du = (pn[0] + 1.0f) * half_wh - tg[0], dv = (pn[1] + 1.0f) * half_wh - tg[1];
    return sqrtf(du * du + dv * dv);
}

__global__ __launch_bounds__(256) void train_error_kernel(const TrainMetrics a) {
    const int s = blockIdx.x, f = blockIdx.y;
    if (f < TM_FAMILIES) {
        if (!a.modes[f]) return;
        const int P = a.points[f];
        double sum[3];
        pointset_error_set<3>(a.pred[f] + (size_t)s * P * 3, a.target[f] + (size_t)s * P * 3, a.xf + ((size_t)f * a.B + s) * 36, P, sum, nullptr);
        if (threadIdx.x < 3 && (a.modes[f] >> threadIdx.x & 1)) a.part[((size_t)f * a.B + s) * 3 + threadIdx.x] = sum[threadIdx.x];
        return;
    }
    // 2-D joints of image s: every joint for joints2D-L2E (:176-181), the visible ones of every sample for joints2Dsamples-L2E (:183-196)
    const bool mode_on = a.mask >> 8 & 1, samples_on = a.mask >> 9 & 1;
    if (!mode_on && !samples_on) return;
    const float half_wh = a.img_wh / 2.0f;
    const int K = a.K;
    const float* tg = a.target_j2d + (size_t)s * K * 2;
    double acc[3] = {0.0, 0.0, 0.0};
    if (mode_on)
        for (int k = threadIdx.x; k < K; k += 256) acc[0] += (double)j2d_error(a.pred_j2d + ((size_t)s * K + k) * 2, tg + k * 2, half_wh);
    if (samples_on) {
        const uint8_t* vis = a.vis + (size_t)s * K;
        const float* ps = a.pred_j2d_samples + (size_t)s * a.N * K * 2;
        const long NK = (long)a.N * K;
        for (long i = threadIdx.x; i < NK; i += 256) {
            const int k = (int)(i % K);
            if (vis[k]) {
                acc[1] += (double)j2d_error(ps + i * 2, tg + k * 2, half_wh);
                acc[2] += 1.0;
            }
        }
    }
    __shared__ double red[3][4];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        double v = acc[m];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[m][threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3 && (threadIdx.x == 0 ? mode_on : samples_on))
        a.j2d[(size_t)s * 3 + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

// One workgroup.  Source c < 10: metric c's per-set values; 10: the visible counts; 11: the status words as 0 / 1.  The sets are staged
// through LDS 256 at a time and lane c adds its column in set-index order; then one lane per slot does sums[split][slot] += value.
__global__ __launch_bounds__(256) void train_finish_kernel(const TrainMetrics a) {
    __shared__ double col[TM_SRC][256];
    const int t = threadIdx.x;
    auto on = [&](int c) { return c < 10 ? (a.mask >> c & 1) != 0 : c == 10 ? (a.mask >> 9 & 1) != 0 : a.status != nullptr; };
    auto rows = [&](int c) { return c == 11 ? a.num_status : a.B; };
    auto value = [&](int c, int s) -> double {
        if (c < 3) return a.part[((size_t)0 * a.B + s) * 3 + c];
        if (c < 5) return a.part[((size_t)1 * a.B + s) * 3 + (c - 3)];
        if (c < 8) return a.part[((size_t)2 * a.B + s) * 3 + (c - 5)];
        if (c < 11) return a.j2d[(size_t)s * 3 + (c - 8)];
        return a.status[s] != 0 ? 1.0 : 0.0;
    };
    double total = 0.0;
    const int n_rows = a.status && a.num_status > a.B ? a.num_status : a.B;
    for (int base = 0; base < n_rows; base += 256) {
        for (int c = 0; c < TM_SRC; ++c)
            if (on(c) && base + t < rows(c)) col[c][t] = value(c, base + t);
        __syncthreads();
        if (t < TM_SRC && on(t)) {
            const int n = min(256, rows(t) - base);
            for (int r = 0; r < n; ++r) total += col[t][r];
        }
        __syncthreads();
    }
    double* out = a.sums + (size_t)a.split * HPS_TRAIN_METRICS_NSLOT;
    if (t < TM_SRC) {
        if (on(t)) out[2 + t] += total;                      // slots 2..11 the metrics, 12 the visible count, 13 the status count
    } else if (t == 64) {
        out[0] += (double)a.loss[0] * (double)a.batch_size;  // :114, loss.item() * batch_size
    } else if (t == 65) {
        out[1] += (double)a.batch_size;
    }
}

}  // namespace hps

using namespace hps;

extern "C" int hps_sizeof_train_metrics_args(void) { return (int)sizeof(hps_train_metrics_args); }

extern "C" int hps_train_metrics_update(const hps_train_metrics_args* args, hps_stream_t stream) {
    if (!args) return bad_arg("hps_train_metrics_update: null pointer (args)");
    if (args->struct_bytes != (int)sizeof(hps_train_metrics_args)) return bad_arg("hps_train_metrics_update: struct_bytes is not sizeof(hps_train_metrics_args)");
    const hps_train_metrics_args& g = *args;
    if (g.B < 1 || g.batch_size < 1) return bad_arg("hps_train_metrics_update: B and batch_size must be at least 1");
    if (g.split != 0 && g.split != 1) return bad_arg("hps_train_metrics_update: split must be 0 (train) or 1 (val)");
    if (g.mask < 0 || g.mask > HPS_TRAIN_METRIC_ALL) return bad_arg("hps_train_metrics_update: mask has bits outside the ten metrics");
    if (!g.loss || !g.workspace || !g.sums) return bad_arg("hps_train_metrics_update: null pointer (loss / workspace / sums)");
    if (((uintptr_t)g.workspace & 7) || ((uintptr_t)g.sums & 7)) return bad_arg("hps_train_metrics_update: workspace and sums must be 8-byte aligned");
    if (g.status ? g.num_status < 1 : g.num_status != 0) return bad_arg("hps_train_metrics_update: num_status must be the length of status (0 without it)");
    TrainMetrics a{};
    const float* pred[3] = {g.pred_verts, g.pred_reposed, g.pred_joints3d};
    const float* target[3] = {g.target_verts, g.target_reposed, g.target_joints3d};
    const int points[3] = {g.P, g.P, g.J}, first_bit[3] = {0, 3, 5}, n_modes[3] = {3, 2, 3};
    for (int f = 0; f < 3; ++f) {
        a.pred[f] = pred[f]; a.target[f] = target[f]; a.points[f] = points[f];
        a.modes[f] = (g.mask >> first_bit[f]) & ((1 << n_modes[f]) - 1);
        if (a.modes[f] && (!pred[f] || !target[f])) return bad_arg("hps_train_metrics_update: null pointer for a tracked point-set metric");
        if (a.modes[f] && points[f] < 1) return bad_arg("hps_train_metrics_update: P / J must be at least 1 for a tracked point-set metric");
    }
    const bool mode_on = g.mask & HPS_TRAIN_METRIC_J2D, samples_on = g.mask & HPS_TRAIN_METRIC_J2D_SAMPLES;
    if ((mode_on || samples_on) && (!g.target_joints2d || g.K < 1 || !(g.img_wh > 0.0f))) return bad_arg("hps_train_metrics_update: 2-D metrics need target_joints2d, K >= 1 and img_wh > 0");
    if (mode_on && !g.pred_joints2d) return bad_arg("hps_train_metrics_update: null pointer (pred_joints2d)");
    if (samples_on && (!g.pred_joints2d_samples || !g.vis || g.N < 1)) return bad_arg("hps_train_metrics_update: joints2Dsamples-L2E needs pred_joints2d_samples, vis and N >= 1");
    a.pred_j2d = g.pred_joints2d; a.target_j2d = g.target_joints2d; a.pred_j2d_samples = g.pred_joints2d_samples;
    a.vis = g.vis; a.loss = g.loss; a.status = g.status;
    a.B = g.B; a.K = g.K; a.N = g.N; a.num_status = g.num_status; a.batch_size = g.batch_size; a.mask = g.mask; a.split = g.split;
    a.img_wh = g.img_wh;
    a.stats = (double*)g.workspace;
    a.part = a.stats + (size_t)g.B * TM_FAMILIES * NSTAT;
    a.j2d = a.part + (size_t)g.B * TM_FAMILIES * 3;
    a.xf = (float*)(a.j2d + (size_t)g.B * 3);
    a.sums = g.sums;
    hipStream_t s = (hipStream_t)stream;
    const long lanes = (long)TM_FAMILIES * g.B * 3;
    if ((lanes + 63) / 64 > 0x7fffffffL) return bad_arg("hps_train_metrics_update: B too large");
    hipLaunchKernelGGL(train_stats_kernel, dim3(g.B, TM_FAMILIES), dim3(256), 0, s, a);
    hipLaunchKernelGGL(train_transform_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, a);
    hipLaunchKernelGGL(train_error_kernel, dim3(g.B, TM_FAMILIES + 1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(train_finish_kernel, dim3(1), dim3(256), 0, s, a);
    return check_launch("hps_train_metrics_update");
}

extern "C" int hps_sums_f64(const float* const* xs, const int64_t* ns, const int32_t* take_abs, int count, double first,
                            double* partial_ws, double* out, double* accumulate, hps_stream_t stream) {
    if (!xs || !ns || !take_abs || !partial_ws || !out) return bad_arg("hps_sums_f64: null pointer");
    if (count < 1 || count > 4) return bad_arg("hps_sums_f64: 1..4 tensors");
    SumJobs jobs;
    for (int j = 0; j < 4; ++j) {
        jobs.x[j] = j < count ? xs[j] : nullptr;
        jobs.n[j] = j < count ? (long)ns[j] : 0;
        jobs.take_abs[j] = j < count ? take_abs[j] : 0;
        if (j < count && (!xs[j] || ns[j] < 0)) return bad_arg("hps_sums_f64: tensor");
    }
    hipLaunchKernelGGL(sums_partial_kernel, dim3(SUM_BLOCKS, count), dim3(256), 0, (hipStream_t)stream, jobs, partial_ws);
    hipLaunchKernelGGL(sums_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_ws, count, first, out, accumulate);
    return check_launch("hps_sums_f64");
}

extern "C" int hps_pointset_errors(const float* pred, const float* target, int S, int group, int P, int mode,
                                   double* stats_ws, float* xf_ws, double* err_sum, float* transformed,
                                   hps_stream_t stream) {
    if (!pred || !target || !stats_ws || !xf_ws || !err_sum) return bad_arg("hps_pointset_errors: null pointer");
    if (group < 1 || P < 1 || mode < 0 || mode > 2) return bad_arg("hps_pointset_errors: group / P / mode");
    if (S <= 0) return HPS_OK;
    hipStream_t s = (hipStream_t)stream;
    if (mode != 0) hipLaunchKernelGGL(pointset_stats_kernel, dim3(S), dim3(256), 0, s, pred, target, group, P, stats_ws);
    hipLaunchKernelGGL(pointset_transform_kernel, dim3(ceil_div(S, 64)), dim3(64), 0, s, stats_ws, S, P, mode, xf_ws);
    hipLaunchKernelGGL(pointset_error_kernel, dim3(S), dim3(256), 0, s, pred, target, xf_ws, group, P, err_sum, transformed);
    return check_launch("hps_pointset_errors");
}
