// Device-side batch preparation for the datasets (data/on_the_fly_smpl_train_dataset.py:72-94, data/ssp3d_eval_dataset.py:49-80,
// data/pw3d_eval_dataset.py:42-60, utils/image_utils.py:145-229, utils/label_conversions.py:94-101): what the reference's __getitem__
// does on the host in NumPy and OpenCV -- uint8 textures and photographs to float32, cv2.resize, the bounding-box crop of
// cv2.warpAffine, joint heat maps -- from the raw uint8 data, where it is consumed.  Only the decoded bytes cross to the device.
//
// cv2.resize and cv2.warpAffine are restated from OpenCV's sources as we understand them (integer arithmetic throughout; the warp's
// positions are csrc/cv_warp.h's, shared with hps_vis_uncrop); they have NOT been run against OpenCV itself.
//
// Bandwidth-bound sweeps: no LDS, no atomics, nothing allocated, bitwise repeatable.  Compiled with -ffp-contract=off: the crop's
// matrix and the joints repeat NumPy's float64 operations one by one, and the heat map the float32 ones.
#include <cmath>

#include "cv_warp.h"
#include "hps_common.h"

namespace hps {

constexpr int DL_MAX = HPS_FRONTEND_MAX_IMAGES;

// ---------------------------------------------------------------------------------------------------------------------------------
// texture gather
// ---------------------------------------------------------------------------------------------------------------------------------
struct GatherTable {
    const uint8_t* src[DL_MAX];
    float* out;
    long long n;                       // elements (= bytes) per texture
};

constexpr int GATHER_UNROLL = 4;

// A lane turns 4 consecutive bytes (one dword load) into one float4 (one 16-byte store): a wave reads 256 and writes 1 024 contiguous
// bytes per step.  The output is 4/5 of the traffic, so it is the store that is 16 bytes wide; a lane that read 16 bytes would have to
// write four float4 that lie 64 bytes apart from its neighbours'.  A texture whose source is not 4-byte or whose destination is not
// 16-byte aligned (odd sizes), and the last 1 to 3 bytes, go element by element.
__global__ __launch_bounds__(256) void texture_gather_kernel(const GatherTable T) {
    const int b = blockIdx.y;
    const uint8_t* __restrict__ src = T.src[b];
    float* __restrict__ dst = T.out + (size_t)b * T.n;
    const bool vec = (((uintptr_t)src & 3) | ((uintptr_t)dst & 15)) == 0;
#pragma unroll
    for (int it = 0; it < GATHER_UNROLL; ++it) {
        const long long e = (((long long)blockIdx.x * GATHER_UNROLL + it) * 256 + threadIdx.x) * 4;
        if (e >= T.n) return;
        if (vec && e + 4 <= T.n) {
            const unsigned w = *reinterpret_cast<const unsigned*>(src + e);
            float4 v;
            v.x = (float)(w & 255u) / 255.0f;
            v.y = (float)((w >> 8) & 255u) / 255.0f;
            v.z = (float)((w >> 16) & 255u) / 255.0f;
            v.w = (float)(w >> 24) / 255.0f;
            *reinterpret_cast<float4*>(dst + e) = v;
        } else {
            for (long long k = e; k < e + 4 && k < T.n; ++k) dst[k] = (float)src[k] / 255.0f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// cv2.resize(INTER_LINEAR) of uint8
// ---------------------------------------------------------------------------------------------------------------------------------
struct U8Image {
    const uint8_t* src;
    int H, W;
};

struct ResizeTable {
    U8Image im[DL_MAX];
    float* out;
    int oh, ow;
};

struct ResizeTap {
    int i0, i1, c0, c1;
};

__device__ __forceinline__ int coef11(float v) {           // saturate_cast<short>(v * INTER_RESIZE_COEF_SCALE), round half to even
    return (int)fminf(fmaxf(rintf(v * 2048.0f), -32768.0f), 32767.0f);
}

// Output index d of `dst` on an axis of `src` pixels.  Columns: a position left of the first or at / right of the last pixel becomes
// that pixel with fraction 0.  Rows: the two rows are clamped and the fraction is kept (both coefficients then weigh one row).
__device__ __forceinline__ ResizeTap resize_tap(int d, int dst, int src, bool column) {
    const double scale = (double)src / (double)dst;
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    ResizeTap t;
    if (column) {
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= src - 1) { f = 0.0f; s = src - 1; }
        t.i0 = s;
        t.i1 = min(s + 1, src - 1);
    } else {
        t.i0 = min(max(s, 0), src - 1);
        t.i1 = min(max(s + 1, 0), src - 1);
    }
    t.c0 = coef11(1.0f - f);
    t.c1 = coef11(f);
    return t;
}

// Lanes along an output row, four rows per workgroup, blockIdx.z = image.
__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(const ResizeTable T) {
    const int b = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= T.ow || i >= T.oh) return;
    const U8Image I = T.im[b];
    const ResizeTap tx = resize_tap(j, T.ow, I.W, true), ty = resize_tap(i, T.oh, I.H, false);
    const uint8_t* r0 = I.src + (size_t)ty.i0 * I.W * 3;
    const uint8_t* r1 = I.src + (size_t)ty.i1 * I.W * 3;
    const size_t plane = (size_t)T.oh * T.ow;
    float* o = T.out + (size_t)b * 3 * plane + (size_t)i * T.ow + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = (int)r0[tx.i0 * 3 + c] * tx.c0 + (int)r0[tx.i1 * 3 + c] * tx.c1;
        const int h1 = (int)r1[tx.i0 * 3 + c] * tx.c0 + (int)r1[tx.i1 * 3 + c] * tx.c1;
        const int level = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
        o[c * plane] = (float)(level & 255) / 255.0f;      // uchar(...)
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the evaluation crop: cv2.warpAffine of uint8
// ---------------------------------------------------------------------------------------------------------------------------------
struct EvalCropImage {
    const uint8_t* rgb;
    const uint8_t* seg;
    int H, W;
    float a00, a11, a02, a12;          // image_utils.py:191-194, formed on the host
};

struct EvalCropTable {
    EvalCropImage im[DL_MAX];
    const double* keypoints;
    float* rgb;
    float* seg;
    double* joints;
    int* positions;
    int wh, K;
};

__device__ __forceinline__ int to_int16_range(double v) {
    return (int)fmin(fmax(v, -32768.0), 32767.0);
}

__global__ __launch_bounds__(256) void eval_crop_u8_kernel(const EvalCropTable T) {
    const int b = blockIdx.z;
    const EvalCropImage I = T.im[b];
    if (T.joints && blockIdx.x == 0 && blockIdx.y == 0) {
        const int k = threadIdx.y * 64 + threadIdx.x;
        if (k < T.K) {
            // np.einsum('ij,kj->ki', affine_trans, [x, y, 1]) in float64: (a0 x + a1 y) + a2, the off-diagonal entries zero
            const double* p = T.keypoints + ((size_t)b * T.K + k) * 3;
            const double x = p[0], y = p[1];
            const double u = ((double)I.a00 * x + 0.0 * y) + (double)I.a02 * 1.0;
            const double v = (0.0 * x + (double)I.a11 * y) + (double)I.a12 * 1.0;
            const size_t at = ((size_t)b * T.K + k) * 2;
            T.joints[at] = u;
            T.joints[at + 1] = v;
            T.positions[at] = to_int16_range(u);            // astype(np.int16): toward zero
            T.positions[at + 1] = to_int16_range(v);
        }
    }
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= T.wh || i >= T.wh) return;
    const WarpInverse A = warp_invert((double)I.a00, 0.0, (double)I.a02, 0.0, (double)I.a11, (double)I.a12);
    const WarpFixed p = warp_fixed(A, j, i);
    const size_t plane = (size_t)T.wh * T.wh, at = (size_t)i * T.wh + j;
    if (T.seg) {
        int nx, ny;
        warp_nearest(p, nx, ny);
        const bool in = I.seg && nx >= 0 && nx < I.W && ny >= 0 && ny < I.H;
        T.seg[(size_t)b * plane + at] = in ? (float)I.seg[(size_t)ny * I.W + nx] : 0.0f;
    }
    int sx, sy, fx, fy;
    warp_linear(p, sx, sy, fx, fy);
    const int w00 = (32 - fy) * (32 - fx), w01 = (32 - fy) * fx, w10 = fy * (32 - fx), w11 = fy * fx;
    const bool x0 = sx >= 0 && sx < I.W, x1 = sx + 1 >= 0 && sx + 1 < I.W;
    const bool y0 = sy >= 0 && sy < I.H, y1 = sy + 1 >= 0 && sy + 1 < I.H;
    const uint8_t* r0 = I.rgb + ((size_t)(y0 ? sy : 0) * I.W) * 3;
    const uint8_t* r1 = I.rgb + ((size_t)(y1 ? sy + 1 : 0) * I.W) * 3;
    const int c0 = (x0 ? sx : 0) * 3, c1 = (x1 ? sx + 1 : 0) * 3;
    float* o = T.rgb + (size_t)b * 3 * plane + at;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int t00 = (y0 && x0) ? (int)r0[c0 + c] : 0, t01 = (y0 && x1) ? (int)r0[c1 + c] : 0;
        const int t10 = (y1 && x0) ? (int)r1[c0 + c] : 0, t11 = (y1 && x1) ? (int)r1[c1 + c] : 0;
        const int level = (t00 * w00 + t01 * w01 + t10 * w10 + t11 * w11 + 512) >> 10;
        o[c * plane] = (float)level / 255.0f;
    }
}

__global__ __launch_bounds__(256) void keypoints_scale_round_kernel(const double* __restrict__ keypoints, const double* __restrict__ scale,
                                                                   double* __restrict__ joints, int* __restrict__ positions, int n, int K) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= n) return;
    const int b = m / K;
    const double u = keypoints[(size_t)m * 3] * scale[2 * b], v = keypoints[(size_t)m * 3 + 1] * scale[2 * b + 1];
    joints[2 * (size_t)m] = u;
    joints[2 * (size_t)m + 1] = v;
    positions[2 * (size_t)m] = to_int16_range(rint(u));     // .round(): half to even
    positions[2 * (size_t)m + 1] = to_int16_range(rint(v));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// heat maps
// ---------------------------------------------------------------------------------------------------------------------------------
struct HeatmapArgs {
    const int* positions;
    const double* keypoints;
    float* out;
    double threshold;
    int maps, K, wh, use_threshold;
    float std;
    unsigned always_visible;
};

__device__ __forceinline__ float heat(int x, int u, float row, float std) {
    const float c = ((float)x - (float)u) / std;
    return expf(-((c * c) / 2.0f) - row);
}

// A lane writes four consecutive pixels of a row: one float4 where the side is a multiple of 4 (every row is then 16-byte aligned).
__global__ __launch_bounds__(256) void eval_heatmaps_kernel(const HeatmapArgs A) {
    const int m = blockIdx.z;
    const int x = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= A.wh || y >= A.wh) return;
    const int k = m % A.K;
    const int u = A.positions[2 * (size_t)m], v = A.positions[2 * (size_t)m + 1];
    float vis = 1.0f;
    if (A.use_threshold)
        vis = (A.keypoints[(size_t)m * 3 + 2] > A.threshold || ((A.always_visible >> k) & 1u)) ? 1.0f : 0.0f;
    const float r = ((float)y - (float)v) / A.std;
    const float row = (r * r) / 2.0f;
    float* o = A.out + ((size_t)m * A.wh + y) * A.wh + x;
    if ((A.wh & 3) == 0) {
        float4 h;
        h.x = heat(x, u, row, A.std) * vis;
        h.y = heat(x + 1, u, row, A.std) * vis;
        h.z = heat(x + 2, u, row, A.std) * vis;
        h.w = heat(x + 3, u, row, A.std) * vis;
        *reinterpret_cast<float4*>(o) = h;
    } else {
        for (int d = 0; d < 4 && x + d < A.wh; ++d) o[d] = heat(x + d, u, row, A.std) * vis;
    }
}

}  // namespace hps

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------------------
using namespace hps;

extern "C" int hps_sizeof_texture_gather_args(void) { return (int)sizeof(hps_texture_gather_args); }
extern "C" int hps_sizeof_resize_bilinear_u8_args(void) { return (int)sizeof(hps_resize_bilinear_u8_args); }
extern "C" int hps_sizeof_eval_crop_u8_args(void) { return (int)sizeof(hps_eval_crop_u8_args); }
extern "C" int hps_sizeof_eval_heatmaps_args(void) { return (int)sizeof(hps_eval_heatmaps_args); }

extern "C" int hps_texture_gather(const hps_texture_gather_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_texture_gather: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_texture_gather_args)) return bad_arg("hps_texture_gather: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > DL_MAX) return bad_arg("hps_texture_gather: 1 to HPS_FRONTEND_MAX_IMAGES samples per launch");
    if (a->Ht < 1 || a->Wt < 1 || a->Ht > 32767 || a->Wt > 32767) return bad_arg("hps_texture_gather: texture size out of range (1 to 32767)");
    if (a->n_grey < 0 || a->n_nongrey < 0 || (a->n_grey > 0 && !a->grey) || (a->n_nongrey > 0 && !a->nongrey))
        return bad_arg("hps_texture_gather: a bank with textures needs its pointer");
    if (!a->out) return bad_arg("hps_texture_gather: null pointer (out)");
    if ((uintptr_t)a->out & 3) return bad_arg("hps_texture_gather: out must be 4-byte aligned");
    GatherTable T;
    T.n = (long long)a->Ht * a->Wt * 3;
    for (int b = 0; b < a->B; ++b) {
        const int n = a->is_grey[b] ? a->n_grey : a->n_nongrey;
        if (a->idx[b] < 0 || a->idx[b] >= n) return bad_arg("hps_texture_gather: a texture index is outside its bank");
        T.src[b] = (a->is_grey[b] ? a->grey : a->nongrey) + (size_t)a->idx[b] * (size_t)T.n;
    }
    for (int b = a->B; b < DL_MAX; ++b) T.src[b] = T.src[0];
    T.out = a->out;
    const long long steps = (T.n + 4LL * 256 * GATHER_UNROLL - 1) / (4LL * 256 * GATHER_UNROLL);
    hipLaunchKernelGGL(texture_gather_kernel, dim3((unsigned)steps, (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_texture_gather");
}

extern "C" int hps_resize_bilinear_u8(const hps_resize_bilinear_u8_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_resize_bilinear_u8: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_resize_bilinear_u8_args)) return bad_arg("hps_resize_bilinear_u8: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > DL_MAX) return bad_arg("hps_resize_bilinear_u8: 1 to HPS_FRONTEND_MAX_IMAGES images per launch");
    if (!a->out) return bad_arg("hps_resize_bilinear_u8: null pointer (out)");
    if ((uintptr_t)a->out & 3) return bad_arg("hps_resize_bilinear_u8: out must be 4-byte aligned");
    if (a->out_w < 1 || a->out_h < 1 || a->out_w > 32767 || a->out_h > 32767) return bad_arg("hps_resize_bilinear_u8: output size out of range");
    ResizeTable T;
    for (int b = 0; b < a->B; ++b) {
        const hps_u8_image& s = a->image[b];
        if (!s.src) return bad_arg("hps_resize_bilinear_u8: null pointer (image source)");
        if (s.H < 1 || s.W < 1 || s.H > 32767 || s.W > 32767) return bad_arg("hps_resize_bilinear_u8: image size out of range (1 to 32767)");
        T.im[b].src = s.src;
        T.im[b].H = s.H;
        T.im[b].W = s.W;
    }
    for (int b = a->B; b < DL_MAX; ++b) T.im[b] = T.im[0];
    T.out = a->out;
    T.oh = a->out_h;
    T.ow = a->out_w;
    const dim3 grid((unsigned)ceil_div(a->out_w, 64), (unsigned)ceil_div(a->out_h, 4), (unsigned)a->B);
    hipLaunchKernelGGL(resize_bilinear_u8_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, T);
    return check_launch("hps_resize_bilinear_u8");
}

extern "C" int hps_eval_crop_u8(const hps_eval_crop_u8_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_eval_crop_u8: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_eval_crop_u8_args)) return bad_arg("hps_eval_crop_u8: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > DL_MAX) return bad_arg("hps_eval_crop_u8: 1 to HPS_FRONTEND_MAX_IMAGES images per launch");
    if (!a->rgb) return bad_arg("hps_eval_crop_u8: null pointer (rgb)");
    if (a->out_wh < 1 || a->out_wh > 32767) return bad_arg("hps_eval_crop_u8: out_wh out of range (1 to 32767)");
    if (!(a->scale_factor > 0.0) || !std::isfinite(a->scale_factor)) return bad_arg("hps_eval_crop_u8: scale_factor must be positive and finite");
    const bool with_joints = a->keypoints != nullptr;
    if ((a->joints != nullptr) != with_joints || (a->positions != nullptr) != with_joints)
        return bad_arg("hps_eval_crop_u8: keypoints, joints and positions come together");
    if (with_joints && (a->K < 1 || a->K > 256)) return bad_arg("hps_eval_crop_u8: 1 to 256 joints");
    if (((uintptr_t)a->rgb | (uintptr_t)a->seg | (uintptr_t)a->positions) & 3) return bad_arg("hps_eval_crop_u8: rgb / seg / positions must be 4-byte aligned");
    if (((uintptr_t)a->keypoints | (uintptr_t)a->joints) & 7) return bad_arg("hps_eval_crop_u8: keypoints / joints must be 8-byte aligned");
    EvalCropTable T;
    const float owh = (float)a->out_wh;
    for (int b = 0; b < a->B; ++b) {
        const hps_eval_crop_image& s = a->image[b];
        if (!s.rgb) return bad_arg("hps_eval_crop_u8: null pointer (image)");
        if (s.H < 1 || s.W < 1 || s.H > 32767 || s.W > 32767) return bad_arg("hps_eval_crop_u8: image size out of range (1 to 32767)");
        if (!(s.side > 0.0) || !std::isfinite(s.side) || !std::isfinite(s.centre_v) || !std::isfinite(s.centre_h))
            return bad_arg("hps_eval_crop_u8: a box needs a finite centre and a positive, finite side");
        // image_utils.py:155-159 (aspect 1 and a square box: neither branch), :168-169, :176, :191-194 -- float64 operations on float64
        // labels and the float32 output size, each rounded on its own, the results rounded to float32 on assignment
        const double bbox_h = s.side * a->scale_factor, bbox_w = s.side * a->scale_factor;
        const double centre = (double)(owh * 0.5f);
        const double qx = (double)owh / bbox_w, qy = (double)owh / bbox_h;
        const double px = qx * s.centre_h, py = qy * s.centre_v;
        T.im[b].rgb = s.rgb;
        T.im[b].seg = s.seg;
        T.im[b].H = s.H;
        T.im[b].W = s.W;
        T.im[b].a00 = (float)qx;
        T.im[b].a11 = (float)qy;
        T.im[b].a02 = (float)(centre - px);
        T.im[b].a12 = (float)(centre - py);
    }
    for (int b = a->B; b < DL_MAX; ++b) T.im[b] = T.im[0];
    T.keypoints = a->keypoints;
    T.rgb = a->rgb;
    T.seg = a->seg;
    T.joints = a->joints;
    T.positions = a->positions;
    T.wh = a->out_wh;
    T.K = a->K;
    const dim3 grid((unsigned)ceil_div(a->out_wh, 64), (unsigned)ceil_div(a->out_wh, 4), (unsigned)a->B);
    hipLaunchKernelGGL(eval_crop_u8_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, T);
    return check_launch("hps_eval_crop_u8");
}

extern "C" int hps_keypoints_scale_round(const double* keypoints, const double* scale, double* joints, int32_t* positions, int B, int K,
                                         hps_stream_t stream) {
    if (B == 0) return HPS_OK;
    if (B < 0 || B > 65536 || K < 1 || K > 256) return bad_arg("hps_keypoints_scale_round: B in [0, 65536], K in [1, 256]");
    if (!keypoints || !scale || !joints || !positions) return bad_arg("hps_keypoints_scale_round: null pointer");
    if ((((uintptr_t)keypoints | (uintptr_t)scale | (uintptr_t)joints) & 7) || ((uintptr_t)positions & 3))
        return bad_arg("hps_keypoints_scale_round: doubles must be 8-byte, positions 4-byte aligned");
    hipLaunchKernelGGL(keypoints_scale_round_kernel, dim3((unsigned)ceil_div(B * K, 256)), dim3(256), 0, (hipStream_t)stream, keypoints, scale,
                       joints, positions, B * K, K);
    return check_launch("hps_keypoints_scale_round");
}

extern "C" int hps_eval_heatmaps(const hps_eval_heatmaps_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_eval_heatmaps: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_eval_heatmaps_args)) return bad_arg("hps_eval_heatmaps: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->K < 1 || a->K > 32 || (long long)a->B * a->K > 65535) return bad_arg("hps_eval_heatmaps: K in [1, 32], B K <= 65535");
    if (a->wh < 1 || a->wh > 32767) return bad_arg("hps_eval_heatmaps: wh out of range (1 to 32767)");
    if (!a->positions || !a->out || (a->use_threshold && !a->keypoints)) return bad_arg("hps_eval_heatmaps: null pointer");
    if (((uintptr_t)a->positions & 3) || ((uintptr_t)a->keypoints & 7) || ((uintptr_t)a->out & 15))
        return bad_arg("hps_eval_heatmaps: positions 4-byte, keypoints 8-byte, out 16-byte aligned");
    if (!(a->std > 0.0f) || !std::isfinite(a->std) || (a->use_threshold && std::isnan(a->threshold)))
        return bad_arg("hps_eval_heatmaps: std must be positive and finite, threshold not NaN");
    HeatmapArgs A;
    A.positions = a->positions;
    A.keypoints = a->keypoints;
    A.out = a->out;
    A.threshold = a->threshold;
    A.maps = a->B * a->K;
    A.K = a->K;
    A.wh = a->wh;
    A.use_threshold = a->use_threshold ? 1 : 0;
    A.std = a->std;
    A.always_visible = a->always_visible;
    const dim3 grid((unsigned)ceil_div(ceil_div(a->wh, 4), 64), (unsigned)ceil_div(a->wh, 4), (unsigned)A.maps);
    hipLaunchKernelGGL(eval_heatmaps_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, A);
    return check_launch("hps_eval_heatmaps");
}
