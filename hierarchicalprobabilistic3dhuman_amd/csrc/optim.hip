// The optimiser step and what it does to the kernel-side weights (run_train.py:97: optim.Adam(pose_shape_model.parameters(), lr=1e-4);
// train/train_poseMF_shapeGaussian_net.py:346-349: optimiser.zero_grad(), loss.backward(), optimiser.step()).
//
//   hps_adam_step        torch's _single_tensor_adam for EVERY tensor of a step in one launch: a table with one entry per tensor and a
//                        workgroup -> (tensor, chunk) map, both built on the host per step (gradient pointers change).  float64 per
//                        element from the fp32 values, each of p, m, v rounded once (as hps_bn_train_backward_dz does); a streaming
//                        kernel: 16-byte accesses, four per array and lane in flight; no atomics, no reduction -- an element's result
//                        depends on its own four inputs and its tensor's coefficients only.
//   hps_weights_refresh  the derived tensors of a prepared state (resnet.py _ConvBN, PoseMFShapeGaussianNet.prepare) written again
//                        IN PLACE from the stepped parameters: a launch list in the style of hps_encoder_run, every pointer fixed for
//                        the life of the state.  Up to 16 independent ops share one launch (the ops travel as kernel arguments).
//
// Compiled with -ffp-contract=off (build.py): the fold repeats torch's float64 operations one by one (beta - mean * scale is a
// product and a difference, two roundings), a contracted multiply-add would round once.
#include "hps_common.h"

using namespace hps;

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                   // 16-byte accesses per array and lane
constexpr int kChunk = kThreads * kUnroll * 4;               // elements of one workgroup: HPS_ADAM_CHUNK
static_assert(kChunk == HPS_ADAM_CHUNK, "include/hps.h: HPS_ADAM_CHUNK");

struct AdamCoef {
    double lr_wd, wd, one_minus_b1, b2, one_minus_b2, step_size, bc2_sqrt, eps;
    int l2, decoupled;
};

__device__ __forceinline__ AdamCoef adam_coef(const hps_adam_entry& e) {
    AdamCoef c;
    c.wd = e.weight_decay;
    c.lr_wd = 1.0 - e.lr * e.weight_decay;
    c.one_minus_b1 = 1.0 - e.beta1;
    c.b2 = e.beta2;
    c.one_minus_b2 = 1.0 - e.beta2;
    c.step_size = e.lr / e.bias_correction1;
    c.bc2_sqrt = e.bias_correction2_sqrt;
    c.eps = e.eps;
    c.l2 = e.weight_decay != 0.0 && !e.decoupled;
    c.decoupled = e.weight_decay != 0.0 && e.decoupled;
    return c;
}

// torch/optim/adam.py _single_tensor_adam, one element
__device__ __forceinline__ void adam_elem(float& p32, float g32, float& m32, float& v32, const AdamCoef& c) {
    double p = p32, g = g32, m = m32, v = v32;
    if (c.l2) g = g + c.wd * p;                              // grad.add(param, alpha=weight_decay)
    if (c.decoupled) p = p * c.lr_wd;                        // param.mul_(1 - lr * weight_decay)
    m = m + c.one_minus_b1 * (g - m);                        // exp_avg.lerp_(grad, 1 - beta1)
    v = c.b2 * v + c.one_minus_b2 * g * g;                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const double denom = sqrt(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);                       // param.addcdiv_(exp_avg, denom, value=-step_size)
    p32 = (float)p;
    m32 = (float)m;
    v32 = (float)v;
}

// 16-byte pieces in the global address space: the pointers come out of the table, where the compiler cannot see what they point at
// (generic pointers would make every access a flat_ instruction)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) v4f global_v4f;
typedef __attribute__((address_space(1))) float global_f;

__device__ __forceinline__ void adam_vec(v4f& p, const v4f& g, v4f& m, v4f& v, const AdamCoef& c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = p[k], mk = m[k], vk = v[k];
        adam_elem(pk, g[k], mk, vk, c);
        p[k] = pk, m[k] = mk, v[k] = vk;
    }
}

__device__ __forceinline__ void adam_scalar(global_f* p, const global_f* g, global_f* m, global_f* v, int i, const AdamCoef& c) {
    float pk = p[i], mk = m[i], vk = v[i];
    adam_elem(pk, g[i], mk, vk, c);
    p[i] = pk, m[i] = mk, v[i] = vk;
}

__global__ __launch_bounds__(kThreads) void adam_kernel(const hps_adam_entry* __restrict__ table, const int32_t* __restrict__ block_map) {
    const int tensor = block_map[2 * blockIdx.x], chunk = block_map[2 * blockIdx.x + 1];
    const hps_adam_entry e = table[tensor];
    const AdamCoef c = adam_coef(e);
    const int64_t base = (int64_t)chunk * kChunk;
    const int64_t left64 = e.numel - base;
    if (left64 <= 0) return;
    const int left = left64 < kChunk ? (int)left64 : kChunk;              // elements of this workgroup
    global_f* p = (global_f*)(uintptr_t)(e.param + base);
    const global_f* g = (const global_f*)(uintptr_t)(e.grad + base);
    global_f* m = (global_f*)(uintptr_t)(e.exp_avg + base);
    global_f* v = (global_f*)(uintptr_t)(e.exp_avg_sq + base);
    const int tid = threadIdx.x;
    // base is a multiple of 16 KiB: the chunk's alignment is the tensor's
    const bool aligned = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
    if (!aligned) {
        for (int i = tid; i < left; i += kThreads) adam_scalar(p, g, m, v, i, c);
        return;
    }
    global_v4f* p4 = (global_v4f*)p;
    const global_v4f* g4 = (const global_v4f*)g;
    global_v4f* m4 = (global_v4f*)m;
    global_v4f* v4 = (global_v4f*)v;
    v4f rp[kUnroll], rg[kUnroll], rm[kUnroll], rv[kUnroll];
    if (left == kChunk) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = u * kThreads + tid;
            rp[u] = p4[i], rg[u] = g4[i], rm[u] = m4[i], rv[u] = v4[i];
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int i = u * kThreads + tid;
            adam_vec(rp[u], rg[u], rm[u], rv[u], c);
            p4[i] = rp[u], m4[i] = rm[u], v4[i] = rv[u];
        }
        return;
    }
    const int nvec = left >> 2;                                            // whole 16-byte pieces, then up to three elements
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int i = u * kThreads + tid;
        if (i < nvec) rp[u] = p4[i], rg[u] = g4[i], rm[u] = m4[i], rv[u] = v4[i];
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
        const int i = u * kThreads + tid;
        if (i < nvec) {
            adam_vec(rp[u], rg[u], rm[u], rv[u], c);
            p4[i] = rp[u], m4[i] = rm[u], v4[i] = rv[u];
        }
    }
    const int i = 4 * nvec + tid;
    if (tid < 4 && i < left) adam_scalar(p, g, m, v, i, c);
}

// ---- hps_weights_refresh ----
constexpr int kBatch = 16;                                   // ops per launch

struct RefreshBatch {
    hps_refresh_op ops[kBatch];
    int start[kBatch + 1];                                   // first workgroup of op k; [n ..] = the grid
};

// Winograd F(2x2, 3x3) filter transform (resnet.py:85-92)
__device__ const double kG3[4][3] = {{1.0, 0.0, 0.0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0.0, 0.0, 1.0}};
// ... and the stem's F(2, 4) rows for the even phases (resnet.py _STEM_G4)
__device__ const double kG4[5][4] = {{0.5, 0.0, 0.0, 0.0},
                                     {-0.5, -0.5, -0.5, -0.5},
                                     {-1.0 / 6.0, 1.0 / 6.0, -1.0 / 6.0, 1.0 / 6.0},
                                     {1.0 / 6.0, 1.0 / 3.0, 2.0 / 3.0, 4.0 / 3.0},
                                     {0.0, 0.0, 0.0, 1.0}};

__host__ __device__ inline long long refresh_threads(const hps_refresh_op& o) {
    switch (o.kind) {
        case HPS_REFRESH_PERMUTE: return (long long)o.n[0] * o.n[1] * o.n[2] * o.n[3];
        case HPS_REFRESH_FOLD: return o.n[0];
        case HPS_REFRESH_WINO_U: return 16ll * o.n[0] * o.n[1];
        default: return 81ll * 1152;
    }
}

__global__ __launch_bounds__(kThreads) void refresh_kernel(const RefreshBatch b) {
    int k = 0;
    while (k + 1 < kBatch && (int)blockIdx.x >= b.start[k + 1]) ++k;
    const hps_refresh_op& o = b.ops[k];
    const long long t64 = (long long)(blockIdx.x - b.start[k]) * kThreads + threadIdx.x;
    if (t64 >= refresh_threads(o)) return;
    const int t = (int)t64;
    if (o.kind == HPS_REFRESH_PERMUTE) {
        // dst[sum i_k dstride_k] = src[sum i_k sstride_k] (* scale[i_scale_dim] in float64, rounded once)
        int r = t;
        const int i3 = r % o.n[3];
        r /= o.n[3];
        const int i2 = r % o.n[2];
        r /= o.n[2];
        const int i1 = r % o.n[1];
        const int i0 = r / o.n[1];
        const long long so = (long long)i0 * o.sstride[0] + (long long)i1 * o.sstride[1] + (long long)i2 * o.sstride[2] + (long long)i3 * o.sstride[3];
        const long long to = (long long)i0 * o.dstride[0] + (long long)i1 * o.dstride[1] + (long long)i2 * o.dstride[2] + (long long)i3 * o.dstride[3];
        float val = o.src[so];
        if (o.aux0) {
            const int is = o.scale_dim == 0 ? i0 : o.scale_dim == 1 ? i1 : o.scale_dim == 2 ? i2 : i3;
            val = (float)((double)val * (double)o.aux0[is]);
        }
        o.dst[to] = val;
    } else if (o.kind == HPS_REFRESH_FOLD) {
        // _ConvBN.fold: src = gamma, aux0 = beta, aux1 = running_mean, aux2 = running_var.  The bit-equality with _ConvBN.fold (the device
        // tests compare the fp32 results exactly) rests on rsqrt(double) here and torch.rsqrt on a float64 device tensor ending in the
        // same OCML routine (v_rsq_f64 and one refinement; not correctly rounded).  The host restatement uses the CPU's rsqrt and cannot
        // check that: if a torch or ROCm upgrade breaks the bit-equal fold test, look here first -- the two float64 values may then
        // differ in their last place, which reaches fp32 only where the product sits on a rounding tie.
        const double inv_std = rsqrt((double)o.aux2[t] + o.eps);
        const double scale = (double)o.src[t] * inv_std;
        const double prod = (double)o.aux1[t] * scale;
        o.dst[t] = (float)scale;
        o.dst2[t] = (float)((double)o.aux0[t] - prod);
    } else if (o.kind == HPS_REFRESH_WINO_U) {
        // [cin / 8][cout / 64][position 4a + b][(cin % 8) / 4][cout % 64][cin % 4] <- G g G^T
        const int cout = o.n[0], cin = o.n[1], nct = cout >> 6;
        const int j = t & 3, n = (t >> 2) & 63, kq = (t >> 8) & 1, p = (t >> 9) & 15;
        const int ct = (t >> 13) % nct, chunk = (t >> 13) / nct;
        const int c = chunk * 8 + kq * 4 + j, co = ct * 64 + n, a = p >> 2, bb = p & 3;
        const float* g = o.src + ((long long)co * cin + c) * 9;
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double row = 0.0;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) row += (double)g[i * 3 + jj] * kG3[bb][jj];
            s += kG3[a][i] * row;
        }
        o.dst[t] = (float)s;
    } else {
        // the stem's 81 positions (resnet.py _stem_winograd_filters); the 256 floats of slack behind them are not touched
        const int pos = t / 1152, r = t % 1152, half = r / 576;
        int q = r % 576, c, con;
        if (q < 512) {
            c = 8 * (q >> 8) + 2 * (q & 3) + ((q >> 7) & 1);
            con = (q >> 2) & 31;
        } else {
            q -= 512;
            c = 16 + (q >> 5);
            con = q & 31;
        }
        const int co = half * 32 + con;
        int ry, rx, local;
        if (pos < 25) ry = 0, rx = 0, local = pos;
        else if (pos < 45) ry = 0, rx = 1, local = pos - 25;
        else if (pos < 65) ry = 1, rx = 0, local = pos - 45;
        else ry = 1, rx = 1, local = pos - 65;
        const int nx = rx == 0 ? 5 : 4, ty = ry == 0 ? 4 : 3, tx = rx == 0 ? 4 : 3;
        const int i = local / nx, jx = local % nx;
        const float* w = o.src + ((long long)co * 18 + c) * 49;
        double s = 0.0;
        for (int a = 0; a < ty; ++a) {
            double row = 0.0;
            for (int bb = 0; bb < tx; ++bb)
                row += (double)w[(ry + 2 * a) * 7 + rx + 2 * bb] * (rx == 0 ? kG4[jx][bb] : kG3[jx][bb]);
            s += (ry == 0 ? kG4[i][a] : kG3[i][a]) * row;
        }
        o.dst[t] = (float)s;
    }
}

int refresh_check(const hps_refresh_op& o) {
    if (o.kind != HPS_REFRESH_PERMUTE && o.kind != HPS_REFRESH_FOLD && o.kind != HPS_REFRESH_WINO_U && o.kind != HPS_REFRESH_STEM_U)
        return bad_arg("hps_weights_refresh: unknown op kind");
    if (!o.src || !o.dst) return bad_arg("hps_weights_refresh: null pointer");
    if (o.kind == HPS_REFRESH_FOLD && (!o.aux0 || !o.aux1 || !o.aux2 || !o.dst2)) return bad_arg("hps_weights_refresh: null pointer (fold)");
    if (o.kind == HPS_REFRESH_PERMUTE) {
        long long total = 1;
        for (int k = 0; k < 4; ++k) {
            if (o.n[k] <= 0 || o.sstride[k] < 0 || o.dstride[k] < 0) return bad_arg("hps_weights_refresh: extent / stride");
            total *= o.n[k];
        }
        if (total >= (1ll << 31)) return bad_arg("hps_weights_refresh: extent");
        if (o.aux0 && (o.scale_dim < 0 || o.scale_dim > 3)) return bad_arg("hps_weights_refresh: scale_dim");
    } else if (o.kind == HPS_REFRESH_FOLD) {
        if (o.n[0] <= 0) return bad_arg("hps_weights_refresh: channels");
    } else if (o.kind == HPS_REFRESH_WINO_U) {
        if (o.n[0] <= 0 || o.n[1] <= 0 || o.n[0] % 64 || o.n[1] % 8 || 16ll * o.n[0] * o.n[1] >= (1ll << 31))
            return bad_arg("hps_weights_refresh: the Winograd form needs Cout % 64 == 0 and Cin % 8 == 0");
    } else if (o.n[0] != 64 || o.n[1] != 18) {
        return bad_arg("hps_weights_refresh: the stem's Winograd form is 18 -> 64 channels");
    }
    return HPS_OK;
}

}  // namespace

extern "C" int hps_sizeof_adam_entry(void) { return (int)sizeof(hps_adam_entry); }
extern "C" int hps_sizeof_refresh_op(void) { return (int)sizeof(hps_refresh_op); }

extern "C" int hps_adam_step(const hps_adam_entry* table, int n_tensors, const int32_t* block_map, int n_blocks, hps_stream_t stream) {
    if (n_tensors < 0 || n_blocks < 0) return bad_arg("hps_adam_step: negative count");
    if (n_tensors == 0 || n_blocks == 0) return HPS_OK;                   // nothing to step: nothing is launched
    if (!table || !block_map) return bad_arg("hps_adam_step: null pointer");
    adam_kernel<<<dim3(n_blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(table, block_map);
    return check_launch("hps_adam_step");
}

extern "C" int hps_weights_refresh(const hps_refresh_op* ops, int n_ops, hps_stream_t stream) {
    if (!ops && n_ops > 0) return bad_arg("hps_weights_refresh: null op list");
    for (int i = 0; i < n_ops; ++i) {                                     // the whole list before any launch
        const int rc = refresh_check(ops[i]);
        if (rc != HPS_OK) return rc;
    }
    int i = 0;
    while (i < n_ops) {
        RefreshBatch b;
        int n = 0, blocks = 0;
        for (; i < n_ops && n < kBatch; ++i) {
            const hps_refresh_op& o = ops[i];
            // an op whose source / auxiliary POINTER equals a destination pointer of an earlier op of this launch (the scaled data-gradient
            // filter reads the fold) starts the next one; that is the whole test -- no ranges, no offsets, no write-after-read
            bool hazard = false;
            for (int k = 0; k < n && !hazard; ++k) {
                const float* w0 = b.ops[k].dst;
                const float* w1 = b.ops[k].dst2;
                for (const float* r : {o.src, o.aux0, o.aux1, o.aux2}) hazard = hazard || (r && (r == w0 || r == w1));
            }
            if (hazard) break;
            b.ops[n] = o;
            b.start[n] = blocks;
            blocks += (int)((refresh_threads(o) + kThreads - 1) / kThreads);
            ++n;
        }
        for (int k = n; k <= kBatch; ++k) b.start[k] = blocks;
        for (int k = n; k < kBatch; ++k) b.ops[k] = b.ops[0];
        refresh_kernel<<<dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(b);
        const int rc = check_launch("hps_weights_refresh");
        if (rc != HPS_OK) return rc;
    }
    return HPS_OK;
}
