// The detection-specific launches of the person detector (detection.MaskRCNNBoxDetector: the box path of Mask R-CNN with a
// ResNet-50-FPN backbone; run_predict.py:43, predict/predict_hrnet.py:52-57): input transform, RPN decode, per-category NMS,
// level-mapped RoIAlign, the box head's soft-max / decode / filter, the final gather.  The semantics restate torchvision 0.7.0 as we
// understand it (include/hps.h); they have not been run against torchvision.  fp32 throughout, no atomics, nothing allocated, no host
// synchronisation; an absent row is a score of -infinity.  Per-image sizes travel by value in the kernel arguments.
#include <cmath>

#include "hps_common.h"

namespace hps {

constexpr float DET_CLAMP = 4.135166556742356f;                 // log(1000 / 16)

struct DetImage {
    const float* src;
    int H, W, oh, ow;
};

struct TransformTable {
    DetImage im[HPS_DET_MAX_IMAGES];
    float* y;
    int FH, FW, P;
    float mean[3], std[3];
};

// Lanes run along a frame row, four rows per workgroup, blockIdx.z = image; every interior pixel of the frame gets one 16-byte store.
__global__ __launch_bounds__(256) void det_transform_kernel(const TransformTable T) {
    const int b = blockIdx.z;
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= T.FW || i >= T.FH) return;
    const DetImage I = T.im[b];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i < I.oh && j < I.ow) {
        const float sh = (float)I.H / (float)I.oh, sw = (float)I.W / (float)I.ow;
        const float fy = fmaxf(((float)i + 0.5f) * sh - 0.5f, 0.0f), fx = fmaxf(((float)j + 0.5f) * sw - 0.5f, 0.0f);
        const int y0 = min((int)fy, I.H - 1), x0 = min((int)fx, I.W - 1);
        const int y1 = min(y0 + 1, I.H - 1), x1 = min(x0 + 1, I.W - 1);
        const float ly = fy - (float)y0, lx = fx - (float)x0;
        const float hy = 1.0f - ly, hx = 1.0f - lx;
        const size_t plane = (size_t)I.H * I.W;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = I.src + c * plane;
            const float m = T.mean[c], s = T.std[c];
            const float a = (p[(size_t)y0 * I.W + x0] - m) / s, bb = (p[(size_t)y0 * I.W + x1] - m) / s;
            const float cc = (p[(size_t)y1 * I.W + x0] - m) / s, d = (p[(size_t)y1 * I.W + x1] - m) / s;
            v[c] = hy * (hx * a + lx * bb) + ly * (hx * cc + lx * d);
        }
        o = make_float4(v[0], v[1], v[2], 0.0f);
    }
    const size_t row = (size_t)(T.FW + 2 * T.P);
    float4* y = reinterpret_cast<float4*>(T.y) + ((size_t)b * (T.FH + 2 * T.P) + i + T.P) * row + j + T.P;
    *y = o;
}

__global__ __launch_bounds__(256) void det_subsample2_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C4,
                                                            int ipad, int opad, int Ho, int Wo) {
    const long long total = (long long)B * Ho * Wo * C4;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C4);
    long long r = e / C4;
    const int j = (int)(r % Wo);
    r /= Wo;
    const int i = (int)(r % Ho), b = (int)(r / Ho);
    const float4* xs = reinterpret_cast<const float4*>(x) + (((size_t)b * (H + 2 * ipad) + 2 * i + ipad) * (W + 2 * ipad) + 2 * j + ipad) * C4 + c;
    float4* yd = reinterpret_cast<float4*>(y) + (((size_t)b * (Ho + 2 * opad) + i + opad) * (Wo + 2 * opad) + j + opad) * C4 + c;
    *yd = *xs;
}

struct RpnDecode {
    const float* deltas;
    const long long* index;
    const float* logits;
    float* boxes;
    float* scores;
    int h, w, A, k, n_out, out_offset;
    float stride_h, stride_w, min_size;
    float base[HPS_DET_MAX_ANCHORS][4];
    short size[HPS_DET_MAX_IMAGES][2];
};

// BoxCoder.decode_single for one box: anchor / proposal (ax1, ay1, ax2, ay2), deltas already divided by the coder's weights
__device__ __forceinline__ float4 det_decode(float ax1, float ay1, float ax2, float ay2, float dx, float dy, float dw, float dh) {
    const float w = ax2 - ax1, h = ay2 - ay1;
    const float cx = ax1 + 0.5f * w, cy = ay1 + 0.5f * h;
    dw = fminf(dw, DET_CLAMP);
    dh = fminf(dh, DET_CLAMP);
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    return make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw, pcy + 0.5f * ph);
}

__device__ __forceinline__ float4 det_clip(float4 v, float rw, float rh) {
    return make_float4(fminf(fmaxf(v.x, 0.0f), rw), fminf(fmaxf(v.y, 0.0f), rh), fminf(fmaxf(v.z, 0.0f), rw), fminf(fmaxf(v.w, 0.0f), rh));
}

__global__ __launch_bounds__(256) void det_rpn_decode_kernel(const RpnDecode T) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= T.k) return;
    const long long idx = T.index[(size_t)b * T.k + j];
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = -INFINITY;
    if (idx >= 0 && idx < (long long)T.h * T.w * T.A) {
        const int a = (int)(idx % T.A);
        const int p = (int)(idx / T.A);
        const int x = p % T.w, y = p / T.w;
        const float sx = (float)x * T.stride_w, sy = (float)y * T.stride_h;
        const float* d = T.deltas + (((size_t)b * T.h + y) * T.w + x) * (4 * T.A) + 4 * a;
        float4 v = det_decode(T.base[a][0] + sx, T.base[a][1] + sy, T.base[a][2] + sx, T.base[a][3] + sy, d[0], d[1], d[2], d[3]);
        v = det_clip(v, (float)T.size[b][1], (float)T.size[b][0]);
        if (v.z - v.x >= T.min_size && v.w - v.y >= T.min_size) {
            box = v;
            score = T.logits[(size_t)b * T.k + j];
        }
    }
    const size_t o = (size_t)b * T.n_out + T.out_offset + j;
    reinterpret_cast<float4*>(T.boxes)[o] = box;
    T.scores[o] = score;
}

// One workgroup per group; the group's boxes, in score order, and their alive flags in LDS.  Step i is uniform: every thread reads
// alive[i] behind the previous step's barrier; a dead or absent i writes nothing and needs no barrier.
__global__ __launch_bounds__(256) void det_nms_kernel(const float* __restrict__ boxes, const long long* __restrict__ order,
                                                     const float* __restrict__ scores, float* __restrict__ keep, int N, float thresh) {
    __shared__ float4 sb[HPS_DET_NMS_MAX_BOXES];
    __shared__ unsigned char alive[HPS_DET_NMS_MAX_BOXES];
    const size_t g = (size_t)blockIdx.x * N;
    const int tid = threadIdx.x;
    for (int i = tid; i < N; i += 256) {
        const float s = scores[g + i];
        long long o = order ? order[g + i] : (long long)i;
        const bool ok = s > -INFINITY && o >= 0 && o < N;
        sb[i] = ok ? reinterpret_cast<const float4*>(boxes)[g + o] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        alive[i] = ok ? 1 : 0;
    }
    __syncthreads();
    for (int i = 0; i < N - 1; ++i) {
        if (!alive[i]) continue;
        const float4 a = sb[i];
        const float area_a = (a.z - a.x) * (a.w - a.y);
        for (int t = i + 1 + tid; t < N; t += 256) {
            if (!alive[t]) continue;
            const float4 c = sb[t];
            const float iw = fmaxf(fminf(a.z, c.z) - fmaxf(a.x, c.x), 0.0f), ih = fmaxf(fminf(a.w, c.w) - fmaxf(a.y, c.y), 0.0f);
            const float inter = iw * ih;
            const float iou = inter / (area_a + (c.z - c.x) * (c.w - c.y) - inter);
            if (iou > thresh) alive[t] = 0;
        }
        __syncthreads();
    }
    for (int i = tid; i < N; i += 256) keep[g + i] = alive[i] ? scores[g + i] : -INFINITY;
}

struct DetLevel {
    const float* x;
    int h, w, pad;
    float scale;
};

struct RoiAlign {
    DetLevel level[HPS_DET_MAX_LEVELS];
    const float* boxes;
    const float* scores;
    float* y;
    int R, C, bins, n_levels, halo;
};

// One workgroup per box; a thread owns channels tid, tid + 256, ... (neighbouring lanes read neighbouring NHWC floats); the sample
// geometry is uniform over the workgroup.  The box's output is a (bins + 2 halo)^2 frame whose border is written as zeros; blockIdx.z
// takes an equal share of the frame's positions (one workgroup per box leaves most of the chip idle at 100 boxes of 256 positions).
__global__ __launch_bounds__(256) void det_roi_align_kernel(const RoiAlign T) {
    const int r = blockIdx.x, b = blockIdx.y;
    const size_t row = (size_t)b * T.R + r;
    const int fb = T.bins + 2 * T.halo, n = fb * fb;
    float* y = T.y + row * (size_t)n * T.C;
    const int share = ceil_div(n, (int)gridDim.z);
    const int p0 = (int)blockIdx.z * share, p1 = min(n, p0 + share);
    if (!(T.scores[row] > -INFINITY)) {
        for (int p = p0; p < p1; ++p)
            for (int c = threadIdx.x; c < T.C; c += 256) y[(size_t)p * T.C + c] = 0.0f;
        return;
    }
    const float4 bx = reinterpret_cast<const float4*>(T.boxes)[row];
    const float area = (bx.z - bx.x) * (bx.w - bx.y);
    int lv = (int)floorf(4.0f + log2f(sqrtf(area) / 224.0f + 1e-6f));
    lv = min(max(lv, 2), 1 + T.n_levels) - 2;
    const DetLevel L = T.level[lv];
    const float x1 = bx.x * L.scale, y1 = bx.y * L.scale;
    const float rw = fmaxf(bx.z * L.scale - x1, 1.0f), rh = fmaxf(bx.w * L.scale - y1, 1.0f);
    const float bw = rw / (float)T.bins, bh = rh / (float)T.bins;
    const size_t fw = (size_t)(L.w + 2 * L.pad);
    const float* base = L.x + ((size_t)b * (L.h + 2 * L.pad) + L.pad) * fw * T.C + (size_t)L.pad * T.C;
    for (int p = p0; p < p1; ++p) {
        const int fy = p / fb;
        const int ph = fy - T.halo, pw = p - fy * fb - T.halo;
        if (ph < 0 || ph >= T.bins || pw < 0 || pw >= T.bins) {
            for (int c = threadIdx.x; c < T.C; c += 256) y[(size_t)p * T.C + c] = 0.0f;
            continue;
        }
        // the four samples' taps and weights (uniform)
        size_t off[4][4];
        float wt[4][4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int iy = s >> 1, ix = s & 1;
            float yy = y1 + (float)ph * bh + ((float)iy + 0.5f) * bh / 2.0f;
            float xx = x1 + (float)pw * bw + ((float)ix + 0.5f) * bw / 2.0f;
            const bool out = !(yy >= -1.0f && yy <= (float)L.h && xx >= -1.0f && xx <= (float)L.w);      // also a NaN
            if (yy <= 0.0f) yy = 0.0f;
            if (xx <= 0.0f) xx = 0.0f;
            if (out) { yy = 0.0f; xx = 0.0f; }
            int yl = (int)yy, xl = (int)xx, yh, xh;
            if (yl >= L.h - 1) { yl = yh = L.h - 1; yy = (float)yl; } else yh = yl + 1;
            if (xl >= L.w - 1) { xl = xh = L.w - 1; xx = (float)xl; } else xh = xl + 1;
            const float ly = yy - (float)yl, lx = xx - (float)xl, hy = 1.0f - ly, hx = 1.0f - lx;
            const float z = out ? 0.0f : 1.0f;
            off[s][0] = ((size_t)yl * fw + xl) * T.C; wt[s][0] = z * (hy * hx);
            off[s][1] = ((size_t)yl * fw + xh) * T.C; wt[s][1] = z * (hy * lx);
            off[s][2] = ((size_t)yh * fw + xl) * T.C; wt[s][2] = z * (ly * hx);
            off[s][3] = ((size_t)yh * fw + xh) * T.C; wt[s][3] = z * (ly * lx);
        }
        for (int c = threadIdx.x; c < T.C; c += 256) {
            float acc = 0.0f;
#pragma unroll
            for (int s = 0; s < 4; ++s)
                acc += wt[s][0] * base[off[s][0] + c] + wt[s][1] * base[off[s][1] + c] + wt[s][2] * base[off[s][2] + c] + wt[s][3] * base[off[s][3] + c];
            y[(size_t)p * T.C + c] = acc / 4.0f;
        }
    }
}

struct BoxDecode {
    const float* logits;
    const float* deltas;
    const float* proposals;
    const float* prop_scores;
    float* boxes;
    float* scores;
    float* probs;
    int R, NC;
    float score_thresh, min_size;
    short size[HPS_DET_MAX_IMAGES][2];
};

// One thread per (proposal, class); the soft-max sums run in class order in every thread.
__global__ __launch_bounds__(256) void det_box_decode_kernel(const BoxDecode T) {
    const int b = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= T.R * T.NC) return;
    const int r = e / T.NC, c = e - r * T.NC;
    const size_t row = (size_t)b * T.R + r;
    const float* l = T.logits + row * T.NC;
    float m = l[0];
    for (int k = 1; k < T.NC; ++k) m = fmaxf(m, l[k]);
    float sum = 0.0f;
    for (int k = 0; k < T.NC; ++k) sum += expf(l[k] - m);
    const float prob = expf(l[c] - m) / sum;
    if (T.probs) T.probs[row * T.NC + c] = prob;
    if (c == 0) return;
    float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float score = -INFINITY;
    if (T.prop_scores[row] > -INFINITY && prob > T.score_thresh) {
        const float4 p = reinterpret_cast<const float4*>(T.proposals)[row];
        const float* d = T.deltas + row * (4 * (size_t)T.NC) + 4 * c;
        float4 v = det_decode(p.x, p.y, p.z, p.w, d[0] / 10.0f, d[1] / 10.0f, d[2] / 5.0f, d[3] / 5.0f);
        v = det_clip(v, (float)T.size[b][1], (float)T.size[b][0]);
        if (v.z - v.x >= T.min_size && v.w - v.y >= T.min_size) {
            box = v;
            score = prob;
        }
    }
    const size_t o = ((size_t)b * (T.NC - 1) + (c - 1)) * T.R + r;
    reinterpret_cast<float4*>(T.boxes)[o] = box;
    T.scores[o] = score;
}

struct Gather {
    const float* top_scores;
    const long long* top_index;
    const long long* order;
    const float* boxes;
    float* out_boxes;
    long long* out_labels;
    float* out_scores;
    int* counts;
    int D, R, NC;
    short size[HPS_DET_MAX_IMAGES][4];
};

// One workgroup per image.
__global__ __launch_bounds__(256) void det_gather_kernel(const Gather T) {
    const int b = blockIdx.x;
    const float ratio_h = (float)T.size[b][2] / (float)T.size[b][0], ratio_w = (float)T.size[b][3] / (float)T.size[b][1];
    int total = 0;
    for (int d0 = 0; d0 < T.D; d0 += 256) {
        const int d = d0 + threadIdx.x;
        bool present = false;
        if (d < T.D) {
            const size_t o = (size_t)b * T.D + d;
            const float s = T.top_scores[o];
            const long long idx = T.top_index[o];
            float4 box = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            long long label = 0;
            float score = 0.0f;
            if (s > -INFINITY && idx >= 0 && idx < (long long)(T.NC - 1) * T.R) {
                const size_t grp = (size_t)b * (T.NC - 1) + (size_t)(idx / T.R);
                const long long r = T.order[grp * T.R + (size_t)(idx % T.R)];
                if (r >= 0 && r < T.R) {
                    const float4 v = reinterpret_cast<const float4*>(T.boxes)[grp * T.R + r];
                    box = make_float4(v.x * ratio_w, v.y * ratio_h, v.z * ratio_w, v.w * ratio_h);
                    label = idx / T.R + 1;
                    score = s;
                    present = true;
                }
            }
            reinterpret_cast<float4*>(T.out_boxes)[o] = box;
            T.out_labels[o] = label;
            T.out_scores[o] = score;
        }
        total += __syncthreads_count(present ? 1 : 0);
    }
    if (threadIdx.x == 0) T.counts[b] = total;
}

static bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace hps

using namespace hps;

extern "C" int hps_sizeof_det_transform_args(void) { return (int)sizeof(hps_det_transform_args); }
extern "C" int hps_sizeof_det_rpn_decode_args(void) { return (int)sizeof(hps_det_rpn_decode_args); }
extern "C" int hps_sizeof_det_nms_args(void) { return (int)sizeof(hps_det_nms_args); }
extern "C" int hps_sizeof_det_roi_align_args(void) { return (int)sizeof(hps_det_roi_align_args); }
extern "C" int hps_sizeof_det_box_decode_args(void) { return (int)sizeof(hps_det_box_decode_args); }
extern "C" int hps_sizeof_det_gather_args(void) { return (int)sizeof(hps_det_gather_args); }

extern "C" int hps_det_transform(const hps_det_transform_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_transform: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_transform_args)) return bad_arg("hps_det_transform: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_DET_MAX_IMAGES) return bad_arg("hps_det_transform: 1 to HPS_DET_MAX_IMAGES images per launch");
    if (!a->y || !aligned(a->y, 16)) return bad_arg("hps_det_transform: y must be a 16-byte aligned pointer");
    if (a->FH < 1 || a->FW < 1 || a->FH > 32767 || a->FW > 32767 || a->P < 0 || a->P > 64) return bad_arg("hps_det_transform: frame size out of range");
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(a->mean[c]) || !std::isfinite(a->std[c]) || a->std[c] == 0.0f)
            return bad_arg("hps_det_transform: mean / std must be finite and std non-zero");
    TransformTable T;
    for (int b = 0; b < a->B; ++b) {
        const hps_det_image& s = a->image[b];
        if (!s.src || !aligned(s.src, 4)) return bad_arg("hps_det_transform: null or unaligned image source");
        if (s.H < 1 || s.W < 1 || s.H > 32767 || s.W > 32767) return bad_arg("hps_det_transform: image size out of range (1 to 32767)");
        if (s.oh < 1 || s.ow < 1 || s.oh > a->FH || s.ow > a->FW) return bad_arg("hps_det_transform: the resized image does not fit the frame");
        T.im[b].src = s.src; T.im[b].H = s.H; T.im[b].W = s.W; T.im[b].oh = s.oh; T.im[b].ow = s.ow;
    }
    for (int b = a->B; b < HPS_DET_MAX_IMAGES; ++b) T.im[b] = T.im[0];
    T.y = a->y; T.FH = a->FH; T.FW = a->FW; T.P = a->P;
    for (int c = 0; c < 3; ++c) { T.mean[c] = a->mean[c]; T.std[c] = a->std[c]; }
    const dim3 grid((unsigned)ceil_div(a->FW, 64), (unsigned)ceil_div(a->FH, 4), (unsigned)a->B);
    hipLaunchKernelGGL(det_transform_kernel, grid, dim3(64, 4), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_transform");
}

extern "C" int hps_det_subsample2(const float* x, float* y, int B, int H, int W, int C, int ipad, int opad, hps_stream_t stream) {
    if (B == 0) return HPS_OK;
    if (!x || !y) return bad_arg("hps_det_subsample2: null pointer");
    if (!aligned(x, 16) || !aligned(y, 16)) return bad_arg("hps_det_subsample2: frames must be 16-byte aligned");
    if (B < 0 || H < 1 || W < 1 || C < 4 || C % 4 != 0 || ipad < 0 || opad < 0) return bad_arg("hps_det_subsample2: sizes out of range (C % 4 == 0)");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long total = (long long)B * Ho * Wo * (C / 4);
    if (total > (1LL << 31) - 256) return bad_arg("hps_det_subsample2: map too large");
    hipLaunchKernelGGL(det_subsample2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, B, H, W, C / 4, ipad, opad, Ho, Wo);
    return check_launch("hps_det_subsample2");
}

static int copy_sizes(const int (*src)[2], short (*dst)[2], int B, const char* what) {
    for (int b = 0; b < HPS_DET_MAX_IMAGES; ++b) {
        const int k = b < B ? b : 0;
        if (src[k][0] < 1 || src[k][1] < 1 || src[k][0] > 32767 || src[k][1] > 32767) return bad_arg(what);
        dst[b][0] = (short)src[k][0];
        dst[b][1] = (short)src[k][1];
    }
    return HPS_OK;
}

extern "C" int hps_det_rpn_decode(const hps_det_rpn_decode_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_rpn_decode: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_rpn_decode_args)) return bad_arg("hps_det_rpn_decode: struct_bytes does not match this library");
    if (a->B == 0 || a->k == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_DET_MAX_IMAGES) return bad_arg("hps_det_rpn_decode: 1 to HPS_DET_MAX_IMAGES images per launch");
    if (a->A < 1 || a->A > HPS_DET_MAX_ANCHORS || a->h < 1 || a->w < 1 || (long long)a->h * a->w * a->A >= (1LL << 31))
        return bad_arg("hps_det_rpn_decode: map / anchor count out of range");
    if (a->k < 0 || a->out_offset < 0 || (long long)a->out_offset + a->k > a->n_out) return bad_arg("hps_det_rpn_decode: the k rows do not fit n_out");
    if (!a->deltas || !a->index || !a->logits || !a->boxes || !a->scores) return bad_arg("hps_det_rpn_decode: null pointer");
    if (!aligned(a->deltas, 4) || !aligned(a->index, 8) || !aligned(a->logits, 4) || !aligned(a->boxes, 16) || !aligned(a->scores, 4))
        return bad_arg("hps_det_rpn_decode: unaligned pointer (boxes 16 bytes, index 8, the rest 4)");
    if (!std::isfinite(a->stride_h) || !std::isfinite(a->stride_w) || std::isnan(a->min_size)) return bad_arg("hps_det_rpn_decode: strides / min_size not finite");
    RpnDecode T;
    if (int rc = copy_sizes(a->size, T.size, a->B, "hps_det_rpn_decode: image size out of range (1 to 32767)")) return rc;
    T.deltas = a->deltas; T.index = (const long long*)a->index; T.logits = a->logits; T.boxes = a->boxes; T.scores = a->scores;
    T.h = a->h; T.w = a->w; T.A = a->A; T.k = a->k; T.n_out = a->n_out; T.out_offset = a->out_offset;
    T.stride_h = a->stride_h; T.stride_w = a->stride_w; T.min_size = a->min_size;
    for (int i = 0; i < HPS_DET_MAX_ANCHORS; ++i)
        for (int e = 0; e < 4; ++e) T.base[i][e] = i < a->A ? a->base[i][e] : 0.0f;
    hipLaunchKernelGGL(det_rpn_decode_kernel, dim3((unsigned)ceil_div(a->k, 256), (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_rpn_decode");
}

extern "C" int hps_det_nms(const hps_det_nms_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_nms: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_nms_args)) return bad_arg("hps_det_nms: struct_bytes does not match this library");
    if (a->G == 0 || a->N == 0) return HPS_OK;
    if (a->G < 0 || a->N < 0 || a->N > HPS_DET_NMS_MAX_BOXES) return bad_arg("hps_det_nms: G >= 0 groups of 0 to HPS_DET_NMS_MAX_BOXES boxes");
    if (!a->boxes || !a->scores || !a->keep_scores) return bad_arg("hps_det_nms: null pointer");
    if (!aligned(a->boxes, 16) || !aligned(a->scores, 4) || !aligned(a->keep_scores, 4) || !aligned(a->order, 8))
        return bad_arg("hps_det_nms: unaligned pointer (boxes 16 bytes, order 8, scores 4)");
    if (std::isnan(a->thresh)) return bad_arg("hps_det_nms: thresh is NaN");
    hipLaunchKernelGGL(det_nms_kernel, dim3((unsigned)a->G), dim3(256), 0, (hipStream_t)stream, a->boxes, (const long long*)a->order, a->scores,
                       a->keep_scores, a->N, a->thresh);
    return check_launch("hps_det_nms");
}

extern "C" int hps_det_roi_align(const hps_det_roi_align_args* a, hps_stream_t stream) { return hps_det_roi_align_halo(a, 0, stream); }

extern "C" int hps_det_roi_align_halo(const hps_det_roi_align_args* a, int halo, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_roi_align: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_roi_align_args)) return bad_arg("hps_det_roi_align: struct_bytes does not match this library");
    if (a->B == 0 || a->R == 0) return HPS_OK;
    if (a->B < 0 || a->B > 65535 || a->R < 0 || a->C < 1 || a->bins < 1 || a->bins > 64) return bad_arg("hps_det_roi_align: sizes out of range");
    if (halo < 0 || halo > 8) return bad_arg("hps_det_roi_align: halo out of range (0 to 8)");
    if (a->n_levels < 1 || a->n_levels > HPS_DET_MAX_LEVELS) return bad_arg("hps_det_roi_align: 1 to HPS_DET_MAX_LEVELS levels");
    if (!a->boxes || !a->scores || !a->y) return bad_arg("hps_det_roi_align: null pointer");
    if (!aligned(a->boxes, 16) || !aligned(a->scores, 4) || !aligned(a->y, 4)) return bad_arg("hps_det_roi_align: unaligned pointer (boxes 16 bytes)");
    RoiAlign T;
    for (int l = 0; l < HPS_DET_MAX_LEVELS; ++l) {
        const hps_det_level& s = a->level[l < a->n_levels ? l : 0];
        if (!s.x || !aligned(s.x, 4)) return bad_arg("hps_det_roi_align: null or unaligned level frame");
        if (s.h < 1 || s.w < 1 || s.pad < 0 || !(s.scale > 0.0f) || !std::isfinite(s.scale)) return bad_arg("hps_det_roi_align: level geometry out of range");
        T.level[l].x = s.x; T.level[l].h = s.h; T.level[l].w = s.w; T.level[l].pad = s.pad; T.level[l].scale = s.scale;
    }
    T.boxes = a->boxes; T.scores = a->scores; T.y = a->y; T.R = a->R; T.C = a->C; T.bins = a->bins; T.n_levels = a->n_levels; T.halo = halo;
    hipLaunchKernelGGL(det_roi_align_kernel, dim3((unsigned)a->R, (unsigned)a->B, halo ? 8u : 1u), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_roi_align");
}

extern "C" int hps_det_box_decode(const hps_det_box_decode_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_box_decode: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_box_decode_args)) return bad_arg("hps_det_box_decode: struct_bytes does not match this library");
    if (a->B == 0 || a->R == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_DET_MAX_IMAGES) return bad_arg("hps_det_box_decode: 1 to HPS_DET_MAX_IMAGES images per launch");
    if (a->R < 0 || a->NC < 2 || (long long)a->R * a->NC >= (1LL << 30)) return bad_arg("hps_det_box_decode: R >= 0, NC >= 2");
    if (!a->logits || !a->deltas || !a->proposals || !a->prop_scores || !a->boxes || !a->scores) return bad_arg("hps_det_box_decode: null pointer");
    if (!aligned(a->logits, 4) || !aligned(a->deltas, 4) || !aligned(a->proposals, 16) || !aligned(a->prop_scores, 4) || !aligned(a->boxes, 16) ||
        !aligned(a->scores, 4) || !aligned(a->probs, 4))
        return bad_arg("hps_det_box_decode: unaligned pointer (proposals / boxes 16 bytes)");
    if (std::isnan(a->score_thresh) || std::isnan(a->min_size)) return bad_arg("hps_det_box_decode: score_thresh / min_size is NaN");
    BoxDecode T;
    if (int rc = copy_sizes(a->size, T.size, a->B, "hps_det_box_decode: image size out of range (1 to 32767)")) return rc;
    T.logits = a->logits; T.deltas = a->deltas; T.proposals = a->proposals; T.prop_scores = a->prop_scores;
    T.boxes = a->boxes; T.scores = a->scores; T.probs = a->probs; T.R = a->R; T.NC = a->NC;
    T.score_thresh = a->score_thresh; T.min_size = a->min_size;
    hipLaunchKernelGGL(det_box_decode_kernel, dim3((unsigned)ceil_div(a->R * a->NC, 256), (unsigned)a->B), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_box_decode");
}

extern "C" int hps_det_gather(const hps_det_gather_args* a, hps_stream_t stream) {
    if (!a) return bad_arg("hps_det_gather: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_det_gather_args)) return bad_arg("hps_det_gather: struct_bytes does not match this library");
    if (a->B == 0) return HPS_OK;
    if (a->B < 0 || a->B > HPS_DET_MAX_IMAGES) return bad_arg("hps_det_gather: 1 to HPS_DET_MAX_IMAGES images per launch");
    if (a->D < 0 || a->R < 1 || a->NC < 2) return bad_arg("hps_det_gather: D >= 0, R >= 1, NC >= 2");
    if (!a->counts || !aligned(a->counts, 4)) return bad_arg("hps_det_gather: null or unaligned pointer (counts)");
    if (a->D > 0 && (!a->top_scores || !a->top_index || !a->order || !a->boxes || !a->out_boxes || !a->out_labels || !a->out_scores))
        return bad_arg("hps_det_gather: null pointer");
    if (!aligned(a->top_scores, 4) || !aligned(a->top_index, 8) || !aligned(a->order, 8) || !aligned(a->boxes, 16) || !aligned(a->out_boxes, 16) ||
        !aligned(a->out_labels, 8) || !aligned(a->out_scores, 4))
        return bad_arg("hps_det_gather: unaligned pointer (boxes 16 bytes, int64 8)");
    Gather T;
    for (int b = 0; b < HPS_DET_MAX_IMAGES; ++b) {
        const int k = b < a->B ? b : 0;
        for (int e = 0; e < 4; ++e) {
            if (a->size[k][e] < 1 || a->size[k][e] > 32767) return bad_arg("hps_det_gather: image size out of range (1 to 32767)");
            T.size[b][e] = (short)a->size[k][e];
        }
    }
    T.top_scores = a->top_scores; T.top_index = (const long long*)a->top_index; T.order = (const long long*)a->order; T.boxes = a->boxes;
    T.out_boxes = a->out_boxes; T.out_labels = (long long*)a->out_labels; T.out_scores = a->out_scores; T.counts = a->counts;
    T.D = a->D; T.R = a->R; T.NC = a->NC;
    hipLaunchKernelGGL(det_gather_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, T);
    return check_launch("hps_det_gather");
}
