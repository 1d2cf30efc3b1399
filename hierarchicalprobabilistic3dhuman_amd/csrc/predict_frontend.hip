// The predict front end for a batch of photographs of different sizes (predict/predict_hrnet.py:34-117,
// predict/predict_poseMF_shapeGaussian_net.py:61-99, utils/image_utils.py:310-370): person box -> crop to the HRNet input ->
// heat-map arg-max -> crop to the proxy-representation size.  fp32 throughout; compiled with -ffp-contract=off (build.py): the box
// record repeats the reference's float32 operations one by one and is held to them bit for bit, and a sample's value must not depend
// on how the compiler pairs its products.  Per-image descriptors travel by value in the kernel arguments (as hps_conv2d_bn_act_c16's
// problem table): no device allocation, no pointer-table upload, no host synchronisation.
#include <cmath>

#include "hps_common.h"

namespace hps {

constexpr int REC = HPS_FRONTEND_RECORD_FLOATS;

struct BoxImage {
    const float* boxes;
    const long long* labels;
    const float* scores;
    int n, H, W;
};

struct BoxTable {
    BoxImage im[HPS_FRONTEND_MAX_IMAGES];
    float* records;
    int B, hrnet_fix;
    float out_w, out_h, aspect_first, aspect_second, threshold, scale_factor;
};

// One thread per image; a launch of one workgroup.  Every operation below is one IEEE single operation of the reference, in its order.
__global__ __launch_bounds__(HPS_FRONTEND_MAX_IMAGES) void predict_boxes_kernel(const BoxTable T) {
    const int b = threadIdx.x;
    if (b >= T.B) return;
    const BoxImage I = T.im[b];
    // predict_hrnet.py:74-80: the whole image
    float cv = (float)I.H * 0.5f, ch = (float)I.W * 0.5f, h = (float)I.H, w = (float)I.W;
    int picked = -1;
    if (I.boxes) {
        // :55-66: persons above the threshold; the centre-most one, the first of equals (one candidate: itself)
        const float half_h = (float)I.H / 2.0f, half_w = (float)I.W / 2.0f;
        float best = 0.0f;
        for (int k = 0; k < I.n; ++k) {
            if (I.labels[k] != 1 || !(I.scores[k] > T.threshold)) continue;
            const float x1 = I.boxes[4 * k + 0], y1 = I.boxes[4 * k + 1], x2 = I.boxes[4 * k + 2], y2 = I.boxes[4 * k + 3];
            const float kv = (y1 + y2) / 2.0f, kh = (x1 + x2) / 2.0f;                  // utils/image_utils.py:31-34 on [1, 0, 3, 2]
            const float dv = kv - half_h, dh = kh - half_w;
            const float dist = dv * dv + dh * dh;
            if (picked < 0 || dist < best) {
                best = dist; picked = k;
                cv = kv; ch = kh; h = y2 - y1; w = x2 - x1;
            }
        }
    }
    if (T.hrnet_fix) {                                                              // predict_hrnet.py:83-87 (if / elif)
        if (h > w * T.aspect_first) w = h / T.aspect_first;
        else if (h < w * T.aspect_first) h = w * T.aspect_first;
    }
    // utils/image_utils.py:310-312: two masked assignments in sequence (the second sees the first's width); they write through the
    // views predict_hrnet passed, so the box it RETURNS carries them too
    if (h > w * T.aspect_second) w = h / T.aspect_second;
    if (h < w * T.aspect_second) h = w * T.aspect_second;
    const float bh = h * T.scale_factor, bw = w * T.scale_factor;                     // :321-322
    const float sx = T.out_w / bw, sy = T.out_h / bh;                                 // :331-333
    const float tx = T.out_w * 0.5f - sx * ch, ty = T.out_h * 0.5f - sy * cv;         // :329, :334
    float* r = T.records + (size_t)b * REC;
    r[0] = cv; r[1] = ch; r[2] = h; r[3] = w;
    r[4] = bh; r[5] = bw;
    r[6] = sx; r[7] = sy; r[8] = tx; r[9] = ty;
    r[10] = (float)picked;
    r[11] = fmaxf(h, w) * T.scale_factor;
}

struct CropImage {
    const void* src;
    int H, W, kind, reserved;
};

struct CropTable {
    CropImage im[HPS_FRONTEND_MAX_IMAGES];
    const float* records;
    float* raw;
    float* normalised;
    int B, oh, ow;
    float mean[3], std[3];
};

// One tap of the bilinear footprint: the three channels of source pixel (y, x), zero when it lies outside the image.
template <int KIND>
__device__ __forceinline__ void crop_tap(const void* src, int H, int W, int y, int x, float (&v)[3]) {
    if (y < 0 || y >= H || x < 0 || x >= W) {
        v[0] = v[1] = v[2] = 0.0f;
        return;
    }
    if (KIND == HPS_FRONTEND_SRC_HWC_U8) {
        const unsigned char* p = static_cast<const unsigned char*>(src) + ((size_t)y * W + x) * 3;
        v[0] = (float)p[0] / 255.0f; v[1] = (float)p[1] / 255.0f; v[2] = (float)p[2] / 255.0f;
    } else {
        const float* p = static_cast<const float*>(src) + (size_t)y * W + x;
        const size_t plane = (size_t)H * W;
        v[0] = p[0]; v[1] = p[plane]; v[2] = p[2 * plane];
    }
}

// Lanes run along an output row (neighbouring lanes read neighbouring source pixels, stores are row-contiguous), four rows per
// workgroup, blockIdx.z = image.  A sample's arithmetic involves nothing but its own image's descriptor and record.
__global__ __launch_bounds__(256) void crop_bilinear_kernel(const CropTable T) {
    const int b = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= T.ow || i >= T.oh) return;
    const CropImage I = T.im[b];
    const float* r = T.records + (size_t)b * REC;
    const float cv = r[0], ch = r[1], bh = r[4], bw = r[5];
    const float x = ((float)j + 0.5f) * (bw / (float)T.ow) + ((ch - bw * 0.5f) - 0.5f);
    const float y = ((float)i + 0.5f) * (bh / (float)T.oh) + ((cv - bh * 0.5f) - 0.5f);
    // clamped well inside int before the conversion: a position that far out has no tap in the image either way
    const float xf = floorf(fminf(fmaxf(x, -4.0f), (float)I.W + 4.0f)), yf = floorf(fminf(fmaxf(y, -4.0f), (float)I.H + 4.0f));
    const float fx = x - floorf(x), fy = y - floorf(y);
    const int x0 = (int)xf, y0 = (int)yf;
    float t00[3], t01[3], t10[3], t11[3];
    if (I.kind == HPS_FRONTEND_SRC_HWC_U8) {
        crop_tap<HPS_FRONTEND_SRC_HWC_U8>(I.src, I.H, I.W, y0, x0, t00);
        crop_tap<HPS_FRONTEND_SRC_HWC_U8>(I.src, I.H, I.W, y0, x0 + 1, t01);
        crop_tap<HPS_FRONTEND_SRC_HWC_U8>(I.src, I.H, I.W, y0 + 1, x0, t10);
        crop_tap<HPS_FRONTEND_SRC_HWC_U8>(I.src, I.H, I.W, y0 + 1, x0 + 1, t11);
    } else {
        crop_tap<HPS_FRONTEND_SRC_CHW_F32>(I.src, I.H, I.W, y0, x0, t00);
        crop_tap<HPS_FRONTEND_SRC_CHW_F32>(I.src, I.H, I.W, y0, x0 + 1, t01);
        crop_tap<HPS_FRONTEND_SRC_CHW_F32>(I.src, I.H, I.W, y0 + 1, x0, t10);
        crop_tap<HPS_FRONTEND_SRC_CHW_F32>(I.src, I.H, I.W, y0 + 1, x0 + 1, t11);
    }
    const float w00 = (1.0f - fy) * (1.0f - fx), w01 = (1.0f - fy) * fx, w10 = fy * (1.0f - fx), w11 = fy * fx;
    const size_t plane = (size_t)T.oh * T.ow;
    const size_t o = (size_t)b * 3 * plane + (size_t)i * T.ow + j;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = ((t00[c] * w00 + t01[c] * w01) + t10[c] * w10) + t11[c] * w11;
        T.raw[o + c * plane] = v;
        if (T.normalised) T.normalised[o + c * plane] = (v - T.mean[c]) / T.std[c];
    }
}

struct KeypointArgs {
    const float* heatmaps;
    const float* records;
    float *joints_hrnet, *confs, *joints_crop, *visib;
    int maps, K, n, w;
    float factor, vis_threshold;
    unsigned always_visible;
};

// One wave per heat map, four maps per workgroup.  Every lane starts from element 0 and walks its own ascending indices with a strict
// comparison, so it holds the FIRST index of its maximum; the butterfly keeps the larger value and, between equals, the lower index.
__global__ __launch_bounds__(256) void hrnet_keypoints_kernel(const KeypointArgs A) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= A.maps) return;                                                        // wave-uniform
    const float* hm = A.heatmaps + (size_t)m * A.n;
    float best = hm[0];
    int idx = 0;
    for (int e = lane; e < A.n; e += 64) {
        const float v = hm[e];
        if (v > best) { best = v; idx = e; }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float ob = __shfl_xor(best, s, 64);
        const int oi = __shfl_xor(idx, s, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane != 0) return;
    const int b = m / A.K, k = m - b * A.K;
    // predict_hrnet.py:24-28: column = idx % width, row = floor(idx / float(width)), both zeroed unless the maximum is positive; :107
    const float on = best > 0.0f ? 1.0f : 0.0f;
    const float jx = ((float)(idx % A.w) * on) * A.factor;
    const float jy = (floorf((float)idx / (float)A.w) * on) * A.factor;
    A.joints_hrnet[2 * m + 0] = jx;
    A.joints_hrnet[2 * m + 1] = jy;
    A.confs[m] = best;
    if (A.joints_crop) {                                                            // utils/image_utils.py:359-363 with the proxy crop's affine
        const float* r = A.records + (size_t)b * REC;
        A.joints_crop[2 * m + 0] = jx * r[6] + r[8];
        A.joints_crop[2 * m + 1] = jy * r[7] + r[9];
    }
    A.visib[m] = (best > A.vis_threshold || ((A.always_visible >> k) & 1u)) ? 1.0f : 0.0f;
}

}  // namespace hps

using namespace hps;

extern "C" int hps_sizeof_predict_boxes_args(void) { return (int)sizeof(hps_predict_boxes_args); }
extern "C" int hps_sizeof_crop_bilinear_args(void) { return (int)sizeof(hps_crop_bilinear_args); }
extern "C" int hps_sizeof_hrnet_keypoints_args(void) { return (int)sizeof(hps_hrnet_keypoints_args); }

extern "C" int hps_predict_boxes(const hps_predict_boxes_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_predict_boxes: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_predict_boxes_args)) return bad_arg("hps_predict_boxes: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_FRONTEND_MAX_IMAGES) return bad_arg("hps_predict_boxes: 1 to HPS_FRONTEND_MAX_IMAGES images per launch");
    if (!a->records) return bad_arg("hps_predict_boxes: null pointer (records)");
    if ((uintptr_t)a->records & 3) return bad_arg("hps_predict_boxes: records must be 4-byte aligned");
    if (a->out_w < 1 || a->out_h < 1 || a->out_w > 32767 || a->out_h > 32767) return bad_arg("hps_predict_boxes: output size out of range");
    if (!(a->scale_factor > 0.0f) || !std::isfinite(a->scale_factor)) return bad_arg("hps_predict_boxes: scale_factor must be positive and finite");
    if (std::isnan(a->threshold)) return bad_arg("hps_predict_boxes: threshold is NaN");
    BoxTable T;
    for (int b = 0; b < a->B; ++b) {
        const hps_box_image& s = a->image[b];
        if (s.H < 1 || s.W < 1 || s.H > 32767 || s.W > 32767) return bad_arg("hps_predict_boxes: image size out of range (1 to 32767)");
        if (s.n < 0) return bad_arg("hps_predict_boxes: negative number of detections");
        if (s.boxes && s.n > 0 && (!s.labels || !s.scores)) return bad_arg("hps_predict_boxes: null pointer (labels / scores of a detector output)");
        if (((uintptr_t)s.boxes & 3) || ((uintptr_t)s.scores & 3) || ((uintptr_t)s.labels & 7))
            return bad_arg("hps_predict_boxes: boxes / scores must be 4-byte, labels 8-byte aligned");
        T.im[b].boxes = s.boxes;
        T.im[b].labels = (const long long*)s.labels;
        T.im[b].scores = s.scores;
        T.im[b].n = s.boxes ? s.n : 0;
        T.im[b].H = s.H;
        T.im[b].W = s.W;
    }
    for (int b = a->B; b < HPS_FRONTEND_MAX_IMAGES; ++b) T.im[b] = T.im[0];
    T.records = a->records;
    T.B = a->B;
    T.hrnet_fix = a->hrnet_aspect_fix ? 1 : 0;
    T.out_w = (float)a->out_w;
    T.out_h = (float)a->out_h;
    T.aspect_first = (float)((double)a->out_h / (double)a->out_w);                  // predict_hrnet.py:83: a Python float, then a float32 operand
    T.aspect_second = (float)a->out_h / (float)a->out_w;                            // image_utils.py:310: a float32 quotient
    T.threshold = a->threshold;
    T.scale_factor = a->scale_factor;
    hipLaunchKernelGGL(predict_boxes_kernel, dim3(1), dim3(HPS_FRONTEND_MAX_IMAGES), 0, (hipStream_t)stream, T);
    return check_launch("hps_predict_boxes");
}

extern "C" int hps_crop_bilinear(const hps_crop_bilinear_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_crop_bilinear: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_crop_bilinear_args)) return bad_arg("hps_crop_bilinear: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_FRONTEND_MAX_IMAGES) return bad_arg("hps_crop_bilinear: 1 to HPS_FRONTEND_MAX_IMAGES images per launch");
    if (!a->records || !a->raw) return bad_arg("hps_crop_bilinear: null pointer (records / raw)");
    if (((uintptr_t)a->records | (uintptr_t)a->raw | (uintptr_t)a->normalised) & 3)
        return bad_arg("hps_crop_bilinear: records / raw / normalised must be 4-byte aligned");
    if (a->out_w < 1 || a->out_h < 1 || a->out_w > 32767 || a->out_h > 32767) return bad_arg("hps_crop_bilinear: output size out of range");
    if (a->normalised)
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(a->mean[c]) || !std::isfinite(a->std[c]) || a->std[c] == 0.0f)
                return bad_arg("hps_crop_bilinear: mean / std must be finite and std non-zero");
    CropTable T;
    for (int b = 0; b < a->B; ++b) {
        const hps_crop_image& s = a->image[b];
        if (!s.src) return bad_arg("hps_crop_bilinear: null pointer (image source)");
        if (s.H < 1 || s.W < 1 || s.H > 32767 || s.W > 32767) return bad_arg("hps_crop_bilinear: image size out of range (1 to 32767)");
        if (s.kind != HPS_FRONTEND_SRC_HWC_U8 && s.kind != HPS_FRONTEND_SRC_CHW_F32) return bad_arg("hps_crop_bilinear: unknown source kind");
        if (s.kind == HPS_FRONTEND_SRC_CHW_F32 && ((uintptr_t)s.src & 3)) return bad_arg("hps_crop_bilinear: a float source must be 4-byte aligned");
        T.im[b].src = s.src;
        T.im[b].H = s.H;
        T.im[b].W = s.W;
        T.im[b].kind = s.kind;
        T.im[b].reserved = 0;
    }
    for (int b = a->B; b < HPS_FRONTEND_MAX_IMAGES; ++b) T.im[b] = T.im[0];
    T.records = a->records;
    T.raw = a->raw;
    T.normalised = a->normalised;
    T.B = a->B;
    T.oh = a->out_h;
    T.ow = a->out_w;
    for (int c = 0; c < 3; ++c) {
        T.mean[c] = a->mean[c];
        T.std[c] = a->std[c];
    }
    const dim3 grid((unsigned)ceil_div(a->out_w, 64), (unsigned)ceil_div(a->out_h, 4), (unsigned)a->B);
    hipLaunchKernelGGL(crop_bilinear_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, T);
    return check_launch("hps_crop_bilinear");
}

extern "C" int hps_hrnet_keypoints(const hps_hrnet_keypoints_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_hrnet_keypoints: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_hrnet_keypoints_args)) return bad_arg("hps_hrnet_keypoints: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > 65536) return bad_arg("hps_hrnet_keypoints: B out of range");
    if (a->K < 1 || a->K > 32) return bad_arg("hps_hrnet_keypoints: 1 to 32 joints");
    if (a->h < 1 || a->w < 1 || (long)a->h * a->w >= (1L << 24)) return bad_arg("hps_hrnet_keypoints: heat maps of 1 to 2^24 - 1 pixels");
    if (!a->heatmaps || !a->joints_hrnet || !a->confs || !a->visib) return bad_arg("hps_hrnet_keypoints: null pointer");
    if ((a->joints_crop != nullptr) != (a->records != nullptr)) return bad_arg("hps_hrnet_keypoints: joints_crop and records go together");
    if (((uintptr_t)a->heatmaps | (uintptr_t)a->joints_hrnet | (uintptr_t)a->confs | (uintptr_t)a->visib | (uintptr_t)a->joints_crop |
         (uintptr_t)a->records) & 3)
        return bad_arg("hps_hrnet_keypoints: pointers must be 4-byte aligned");
    if (!std::isfinite(a->factor) || std::isnan(a->vis_threshold)) return bad_arg("hps_hrnet_keypoints: factor / vis_threshold not finite");
    KeypointArgs A;
    A.heatmaps = a->heatmaps;
    A.records = a->records;
    A.joints_hrnet = a->joints_hrnet;
    A.confs = a->confs;
    A.joints_crop = a->joints_crop;
    A.visib = a->visib;
    A.maps = a->B * a->K;
    A.K = a->K;
    A.n = a->h * a->w;
    A.w = a->w;
    A.factor = a->factor;
    A.vis_threshold = a->vis_threshold;
    A.always_visible = a->always_visible;
    hipLaunchKernelGGL(hrnet_keypoints_kernel, dim3((unsigned)ceil_div(A.maps, 4)), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch("hps_hrnet_keypoints");
}
