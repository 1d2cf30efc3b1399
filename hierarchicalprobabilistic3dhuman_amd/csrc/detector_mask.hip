// The mask branch of the person detector (detection.MaskRCNNBoxDetector.mask_branch; include/hps.h): the mask predictor in one launch
// (transposed convolution 2x2 / 2 + ReLU + the 1x1 logit of the detection's own class + sigmoid, on the fp32 matrix instructions) and
// the paste of the 28 x 28 masks into the photograph.  The semantics restate torchvision 0.7.0 as we understand it; they have not been
// run against torchvision.  fp32, no atomics, a fixed summation order, nothing allocated, no host synchronisation.  This file is
// compiled with -ffp-contract=off: the paste's box arithmetic rounds every operation once, as the float32 tensor code it restates.
#include <cmath>

#include "hps_common.h"

namespace hps {

constexpr int MASK_BINS = HPS_DET_MASK_BINS, MASK_C = HPS_DET_MASK_CHANNELS, MASK_OUT = HPS_DET_MASK_SIZE;
constexpr int MASK_PIX = MASK_BINS * MASK_BINS, MASK_FRAME = MASK_BINS + 2;
constexpr int MASK_TILE = 32;                                   // pixels per workgroup: one column block of the 32x32x2 instruction

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MaskPredict {
    const float* x;
    const float* wd;
    const float* bd;
    const float* wl;
    const float* bl;
    const long long* labels;
    const float* scores;
    float* probs;
    float* logits;
    int K, NC;
};

// blockIdx.y = detection, blockIdx.x = a tile of 32 of its 196 pixels (the last tile holds 4), wave = tap (dy, dx).  Per wave the
// product  Y^T (256 co x 32 pixels) = Wd_tap^T (256 co x 256 ci) X^T (256 ci x 32 pixels)  as 8 row blocks of v_mfma_f32_32x32x2_f32:
// the A operand is the weight (lane l: co = 32 t + (l & 31), ci = 2 s + (l >> 5), read as two 16-byte loads per step from the
// kernel-side form), the B operand the pixel tile in LDS.  A result column (a pixel) lies on a lane with its 16 rows (co) in the lane's
// registers, so the sum over co runs in registers, row block by row block, and ends with one exchange between the lane halves.
__global__ __launch_bounds__(256) void det_mask_predict_kernel(const MaskPredict T) {
    __shared__ float xs[MASK_C * MASK_TILE];                    // [ci][pixel]
    __shared__ float sbd[MASK_C], swl[MASK_C];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, half = lane >> 5;
    const int dy = wave >> 1, dx = wave & 1;
    const int p = blockIdx.x * MASK_TILE + (lane & 31);
    const int oy = 2 * (p / MASK_BINS) + dy, ox = 2 * (p % MASK_BINS) + dx;
    const size_t o = (size_t)k * (MASK_OUT * MASK_OUT) + (size_t)oy * MASK_OUT + ox;
    const long long label = T.labels[k];
    const bool on = label >= 1 && label < (long long)T.NC && (!T.scores || T.scores[k] > -INFINITY);      // uniform over the workgroup
    if (!on) {
        if (half == 0 && p < MASK_PIX) {
            T.probs[o] = 0.0f;
            if (T.logits) T.logits[o] = 0.0f;
        }
        return;
    }
    for (int it = 0; it < MASK_TILE * (MASK_C / 4) / 256; ++it) {
        const int idx = tid + 256 * it;
        const int px = idx & (MASK_TILE - 1), c4 = idx / MASK_TILE;
        const int q = blockIdx.x * MASK_TILE + px;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q < MASK_PIX)
            v = *reinterpret_cast<const float4*>(T.x + (((size_t)k * MASK_FRAME + q / MASK_BINS + 1) * MASK_FRAME + q % MASK_BINS + 1) * MASK_C + 4 * c4);
        xs[(4 * c4 + 0) * MASK_TILE + px] = v.x;
        xs[(4 * c4 + 1) * MASK_TILE + px] = v.y;
        xs[(4 * c4 + 2) * MASK_TILE + px] = v.z;
        xs[(4 * c4 + 3) * MASK_TILE + px] = v.w;
    }
    sbd[tid] = T.bd[tid];
    swl[tid] = T.wl[(size_t)label * MASK_C + tid];
    __syncthreads();

    f32x16 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
    const float4* wp = reinterpret_cast<const float4*>(T.wd) + ((size_t)wave * (MASK_C / 2) * 64 + lane) * 2;
    const float* xb = xs + half * MASK_TILE + (lane & 31);
#pragma unroll 4
    for (int s = 0; s < MASK_C / 2; ++s) {
        const float4 a0 = wp[(size_t)s * 128], a1 = wp[(size_t)s * 128 + 1];
        const float b = xb[2 * s * MASK_TILE];
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b, acc[1], 0, 0, 0);
        acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b, acc[2], 0, 0, 0);
        acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b, acc[3], 0, 0, 0);
        acc[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b, acc[4], 0, 0, 0);
        acc[5] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b, acc[5], 0, 0, 0);
        acc[6] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b, acc[6], 0, 0, 0);
        acc[7] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b, acc[7], 0, 0, 0);
    }

    // the logit of class ``label``: per row block the 16 rows of this lane half in register order, the 8 blocks in order, the halves
    float part = 0.0f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int co = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * half;
            s = __builtin_fmaf(fmaxf(acc[t][r] + sbd[co], 0.0f), swl[co], s);
        }
        part += s;
    }
    const float logit = (part + __shfl_xor(part, 32)) + T.bl[label];
    if (half == 0 && p < MASK_PIX) {
        T.probs[o] = 1.0f / (1.0f + expf(-logit));
        if (T.logits) T.logits[o] = logit;
    }
}

struct Paste {
    const float* probs;
    const float* boxes;
    void* out;
    long long total;
    int n, H, W, binary;
    float threshold;
};

struct PasteBox {
    int x0, y0, w, h, xa, xb, ya, yb;                            // corner, resized size, the written rectangle [xa, xb) x [ya, yb)
    float sx, sy;
};

// float -> int toward zero; values beyond +-2^29 (no image has them) are held there so that the integer arithmetic cannot overflow
__device__ __forceinline__ int paste_trunc(float v) { return (int)fminf(fmaxf(v, -536870912.0f), 536870912.0f); }

// expand_boxes and the integer box of paste_mask_in_image, one float32 operation at a time
__device__ __forceinline__ PasteBox paste_box(float4 b, int H, int W) {
    const float scale = (float)(30.0 / 28.0);
    float w_half = (b.z - b.x) * 0.5f, h_half = (b.w - b.y) * 0.5f;
    const float x_c = (b.z + b.x) * 0.5f, y_c = (b.w + b.y) * 0.5f;
    w_half *= scale;
    h_half *= scale;
    const int x0 = paste_trunc(x_c - w_half), y0 = paste_trunc(y_c - h_half);
    const int x1 = paste_trunc(x_c + w_half), y1 = paste_trunc(y_c + h_half);
    PasteBox P;
    P.x0 = x0; P.y0 = y0;
    P.w = max(x1 - x0 + 1, 1); P.h = max(y1 - y0 + 1, 1);
    P.xa = max(x0, 0); P.xb = min(x1 + 1, W);
    P.ya = max(y0, 0); P.yb = min(y1 + 1, H);
    P.sx = 30.0f / (float)P.w; P.sy = 30.0f / (float)P.h;
    return P;
}

// the 30 x 30 padded mask: a ring of zeros round the 28 x 28 probabilities
__device__ __forceinline__ float paste_tap(const float* m, int i, int j) {
    return (i >= 1 && i <= MASK_OUT && j >= 1 && j <= MASK_OUT) ? m[(i - 1) * MASK_OUT + (j - 1)] : 0.0f;
}

__device__ __forceinline__ float paste_value(const float* m, const PasteBox& P, int y, int x) {
    if (x < P.xa || x >= P.xb || y < P.ya || y >= P.yb) return 0.0f;
    const float fy = fmaxf(((float)(y - P.y0) + 0.5f) * P.sy - 0.5f, 0.0f), fx = fmaxf(((float)(x - P.x0) + 0.5f) * P.sx - 0.5f, 0.0f);
    const int i0 = min((int)fy, MASK_OUT + 1), j0 = min((int)fx, MASK_OUT + 1);
    const int i1 = min(i0 + 1, MASK_OUT + 1), j1 = min(j0 + 1, MASK_OUT + 1);
    const float ly = fy - (float)i0, lx = fx - (float)j0;
    const float hy = 1.0f - ly, hx = 1.0f - lx;
    const float a = paste_tap(m, i0, j0), b = paste_tap(m, i0, j1), c = paste_tap(m, i1, j0), d = paste_tap(m, i1, j1);
    return hy * (hx * a + lx * b) + ly * (hx * c + lx * d);
}

// A thread owns V consecutive elements of the flat (n, H, W) output, V * sizeof(element) = 16 bytes: one 16-byte store wherever the
// group is whole (the output's base is 16-byte aligned), element stores in the last group.  Every element is written.
template <typename E, int V>
__global__ __launch_bounds__(256) void det_paste_masks_kernel(const Paste T) {
    const long long e0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e0 >= T.total) return;
    const long long plane = (long long)T.H * T.W;
    int k = (int)(e0 / plane);
    const long long rem = e0 - (long long)k * plane;
    int y = (int)(rem / T.W), x = (int)(rem - (long long)y * T.W);
    PasteBox P = paste_box(reinterpret_cast<const float4*>(T.boxes)[k], T.H, T.W);
    const float* m = T.probs + (size_t)k * (MASK_OUT * MASK_OUT);
    alignas(16) E v[V];
    const int count = (int)(T.total - e0 < V ? T.total - e0 : V);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        v[i] = (E)0;
        if (i < count) {
            const float f = paste_value(m, P, y, x);
            if (T.binary) v[i] = (E)(f > T.threshold ? 1 : 0);
            else v[i] = (E)f;
            if (++x == T.W) {
                x = 0;
                if (++y == T.H) {
                    y = 0;
                    ++k;
                    if (i + 1 < count) {
                        P = paste_box(reinterpret_cast<const float4*>(T.boxes)[k], T.H, T.W);
                        m = T.probs + (size_t)k * (MASK_OUT * MASK_OUT);
                    }
                }
            }
        }
    }
    E* out = reinterpret_cast<E*>(T.out) + e0;
    if (count == V) {
        *reinterpret_cast<uint4*>(out) = *reinterpret_cast<const uint4*>(v);
    } else {
        for (int i = 0; i < count; ++i) out[i] = v[i];
    }
}

static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace hps

using namespace hps;

extern "C" int hps_sizeof_det_mask_predict_args(void) { return (int)sizeof(hps_det_mask_predict_args); }
extern "C" int hps_sizeof_det_paste_masks_args(void) { return (int)sizeof(hps_det_paste_masks_args); }

extern "C" int hps_det_mask_predict(const hps_det_mask_predict_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_mask_predict: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_mask_predict_args)) return bad_arg("hps_det_mask_predict: struct_bytes does not match this library");
    if (a->K == 0) return HPS_OK;
    if (a->K < 0 || a->K > 65535) return bad_arg("hps_det_mask_predict: 0 to 65535 detections per launch");
    if (a->NC < 2 || a->NC > (1 << 20)) return bad_arg("hps_det_mask_predict: NC out of range (at least 2)");
    if (!a->x || !a->wd || !a->bd || !a->wl || !a->bl || !a->labels || !a->probs) return bad_arg("hps_det_mask_predict: null pointer");
    if (!aligned(a->x, 16) || !aligned(a->wd, 16) || !aligned(a->bd, 4) || !aligned(a->wl, 4) || !aligned(a->bl, 4) || !aligned(a->labels, 8) ||
        !aligned(a->scores, 4) || !aligned(a->probs, 4) || !aligned(a->logits, 4))
        return bad_arg("hps_det_mask_predict: unaligned pointer (x / wd 16 bytes, labels 8)");
    MaskPredict T;
    T.x = a->x; T.wd = a->wd; T.bd = a->bd; T.wl = a->wl; T.bl = a->bl; T.labels = (const long long*)a->labels; T.scores = a->scores;
    T.probs = a->probs; T.logits = a->logits; T.K = a->K; T.NC = a->NC;
    hipLaunchKernelGGL(det_mask_predict_kernel, dim3((unsigned)ceil_div(MASK_PIX, MASK_TILE), (unsigned)a->K), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_mask_predict");
}

extern "C" int hps_det_paste_masks(const hps_det_paste_masks_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_paste_masks: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_paste_masks_args)) return bad_arg("hps_det_paste_masks: struct_bytes does not match this library");
    if (a->n == 0) return HPS_OK;
    if (a->n < 0 || a->H < 1 || a->W < 1 || a->H > 32767 || a->W > 32767) return bad_arg("hps_det_paste_masks: n >= 0, image size 1 to 32767");
    if (a->binary != 0 && a->binary != 1) return bad_arg("hps_det_paste_masks: binary is 0 or 1");
    if (a->binary && !(a->threshold > 0.0f && a->threshold < 1.0f)) return bad_arg("hps_det_paste_masks: threshold must lie in (0, 1)");
    if (!a->probs || !a->boxes || !a->out) return bad_arg("hps_det_paste_masks: null pointer");
    if (!aligned(a->probs, 4) || !aligned(a->boxes, 16) || !aligned(a->out, 16)) return bad_arg("hps_det_paste_masks: unaligned pointer (boxes / out 16 bytes)");
    Paste T;
    T.probs = a->probs; T.boxes = a->boxes; T.out = a->out; T.n = a->n; T.H = a->H; T.W = a->W; T.binary = a->binary; T.threshold = a->threshold;
    T.total = (long long)a->n * a->H * a->W;
    const int V = a->binary ? 16 : 4;
    const long long groups = (T.total + V - 1) / V, blocks = (groups + 255) / 256;
    if (blocks > 0x7fffffffLL) return bad_arg("hps_det_paste_masks: output too large");
    if (a->binary)
        hipLaunchKernelGGL((det_paste_masks_kernel<unsigned char, 16>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T);
    else
        hipLaunchKernelGGL((det_paste_masks_kernel<float, 4>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_paste_masks");
}
