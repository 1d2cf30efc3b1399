// The synthetic-data training front end between the renderer's output and the Canny / heat-map kernels
// (train/train_poseMF_shapeGaussian_net.py:199-244): bounding box of the part segmentation and the augmented crop's affine maps,
// the fused crop + segmentation augmentation + background composite + RGB augmentation, and the 2D joints with their visibility.
//
// Every random DECISION of a step is made on the host (train_augmentation.draw_augment_plan) and arrives as one block of
// HPS_TRAIN_PLAN_WORDS 32-bit words per image; the kernels only see class masks, half-open [lo, hi) ranges, thresholds and factors.
//
// This file is compiled with -ffp-contract=off (build.py): the box and affine arithmetic follows the reference's fp32 operations one
// by one (utils/image_utils.py:307-345), and a fused multiply-add would round differently.
#include "hps_common.h"

namespace hps {

constexpr int TF_K = HPS_TRAIN_NUM_JOINTS;          // COCO joints
constexpr int TF_PW = HPS_TRAIN_PLAN_WORDS;
constexpr int TF_CHUNKS = 32;                       // row chunks of the box reduction (HPS_WS_SEG_BBOX)
constexpr int TF_PARTS = HPS_TRAIN_NUM_PART_COUNTS; // counted 14-part labels 3, 5, 7, 9, 11, 12, 13, 14

// word offsets inside one image's plan record (include/hps.h: hps_seg_bbox_affine)
enum {
    PW_CROP_MASK = 0, PW_SEG_MASK = 1, PW_DSCALE = 2, PW_DCENTRE = 3, PW_BOX = 5, PW_SEG_OCC = 9, PW_RGB_OCC = 15, PW_SEG_JT = 21,
    PW_RGB_JT = 25, PW_INVIS = 29, PW_CHAN = 30, PW_SWAP = 33, PW_DEV = 50
};
static_assert(PW_DEV + 2 * TF_K == TF_PW, "plan record layout");

// utils/label_conversions.py:47-70 restricted to the labels utils/joints2d_utils.py:37 asks for: 24-part class -> slot of
// (3, 5, 7, 9, 11, 12, 13, 14), -1 for every other class
__device__ __forceinline__ int part24_slot(int c) {
    switch (c) {
        case 19: case 21: return 0;   // 14-part 3
        case 20: case 22: return 1;   // 5
        case 12: case 14: return 2;   // 7
        case 11: case 13: return 3;   // 9
        case 3: return 4;             // 11
        case 4: return 5;             // 12
        case 6: return 6;             // 13
        case 5: return 7;             // 14
        default: return -1;
    }
}

__device__ __forceinline__ int part14_slot(int c) {
    switch (c) {
        case 3: return 0; case 5: return 1; case 7: return 2; case 9: return 3;
        case 11: return 4; case 12: return 5; case 13: return 6; case 14: return 7;
        default: return -1;
    }
}

// true when class value v (a float holding an integer) is one of the classes of mask
__device__ __forceinline__ bool class_in_mask(float v, uint32_t mask) {
    if (!(v >= 0.0f && v < 32.0f)) return false;
    const int c = (int)v;
    return (float)c == v && ((mask >> c) & 1u);
}

// ---- hps_seg_bbox_affine, stage 1: per (row chunk, image) the integer min / max of the rows and columns of kept pixels ----------------
__global__ __launch_bounds__(256) void seg_bbox_partial_kernel(const float* __restrict__ part, int64_t part_batch_stride,
                                                               const int32_t* __restrict__ plan, int H, int W,
                                                               int32_t* __restrict__ ws) {
    const int b = blockIdx.y, chunk = blockIdx.x;
    const uint32_t mask = plan ? (uint32_t)plan[(size_t)b * TF_PW + PW_CROP_MASK] : 0u;
    const int rows_per = ceil_div(H, TF_CHUNKS);
    const int r_begin = min(H, chunk * rows_per), r_end = min(H, r_begin + rows_per);
    const float* p = part + (size_t)b * part_batch_stride;
    int rmin = INT_MAX, cmin = INT_MAX, rmax = -1, cmax = -1;
    for (int r = r_begin; r < r_end; ++r) {
        const float* row = p + (size_t)r * W;
        for (int c = threadIdx.x; c < W; c += 256) {
            const float v = row[c];
            if (v != 0.0f && !class_in_mask(v, mask)) {
                rmin = min(rmin, r); rmax = max(rmax, r);
                cmin = min(cmin, c); cmax = max(cmax, c);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rmin = min(rmin, __shfl_xor(rmin, off)); cmin = min(cmin, __shfl_xor(cmin, off));
        rmax = max(rmax, __shfl_xor(rmax, off)); cmax = max(cmax, __shfl_xor(cmax, off));
    }
    __shared__ int s[4][4];
    if ((threadIdx.x & 63) == 0) {
        int* d = s[threadIdx.x >> 6];
        d[0] = rmin; d[1] = cmin; d[2] = rmax; d[3] = cmax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            rmin = min(rmin, s[w][0]); cmin = min(cmin, s[w][1]);
            rmax = max(rmax, s[w][2]); cmax = max(cmax, s[w][3]);
        }
        int32_t* o = ws + ((size_t)b * TF_CHUNKS + chunk) * 4;
        o[0] = rmin; o[1] = cmin; o[2] = rmax; o[3] = cmax;
    }
}

// ---- stage 2: one lane per image -- the box, then utils/image_utils.py:307-345 in fp32, operation by operation -----------------------
__global__ __launch_bounds__(64) void seg_bbox_finish_kernel(const int32_t* __restrict__ ws, const int32_t* __restrict__ plan, int B,
                                                             int H, int W, int D, float orig_scale, float* __restrict__ affine,
                                                             float* __restrict__ theta, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ part_counts) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int rmin = INT_MAX, cmin = INT_MAX, rmax = -1, cmax = -1;
    for (int c = 0; c < TF_CHUNKS; ++c) {
        const int32_t* o = ws + ((size_t)b * TF_CHUNKS + c) * 4;
        rmin = min(rmin, o[0]); cmin = min(cmin, o[1]); rmax = max(rmax, o[2]); cmax = max(cmax, o[3]);
    }
    const bool empty = rmax < 0;
    if (empty) { rmin = 0; cmin = 0; rmax = H - 1; cmax = W - 1; }       // where the reference raises: whole frame + status word
    if (status) status[b] = empty ? 1 : 0;
    if (part_counts)
        for (int i = 0; i < TF_PARTS; ++i) part_counts[(size_t)b * TF_PARTS + i] = 0;
    float dscale = 0.0f, dcv = 0.0f, dch = 0.0f;
    if (plan) {
        const float* pf = reinterpret_cast<const float*>(plan + (size_t)b * TF_PW);
        dscale = pf[PW_DSCALE]; dcv = pf[PW_DCENTRE]; dch = pf[PW_DCENTRE + 1];
    }
    const float out_w = (float)D, out_h = (float)D, in_w = (float)W, in_h = (float)H;
    float cv = ((float)rmin + (float)rmax) / 2.0f, ch = ((float)cmin + (float)cmax) / 2.0f;      // :31-34
    float bh = (float)rmax - (float)rmin, bw = (float)cmax - (float)cmin;
    const float aspect = out_h / out_w;                                                          // :310-312, one after the other
    if (bh > bw * aspect) bw = bh / aspect;
    if (bh < bw * aspect) bh = bw * aspect;
    const float scale = orig_scale + dscale;                                                     // :315-326
    bh = bh * scale; bw = bw * scale;
    cv = cv + dcv; ch = ch + dch;
    const float sx = out_w / bw, sy = out_h / bh;                                                // :329-334
    const float a02 = out_w * 0.5f - sx * ch, a12 = out_h * 0.5f - sy * cv;
    float* a = affine + (size_t)b * 6;
    a[0] = sx; a[1] = 0.0f; a[2] = a02; a[3] = 0.0f; a[4] = sy; a[5] = a12;
    float t02 = (-a02) / sx, t12 = (-a12) / sy;                                                  // :341-345
    t02 = t02 / (in_w * 0.5f) + bw / in_w - 1.0f;
    t12 = t12 / (in_h * 0.5f) + bh / in_h - 1.0f;
    float* t = theta + (size_t)b * 4;
    t[0] = bw / in_w; t[1] = t02; t[2] = bh / in_h; t[3] = t12;
}

// ---- hps_train_crop_augment ---------------------------------------------------------------------------------------------------------
struct CropArgs {
    const float* part; int64_t part_batch_stride;
    const float* rgb; const float* background; const float* theta; const int32_t* plan;
    float* rgb_out; int32_t* part_counts; float* part_crop; float* part_aug;
    int H, W, OH, OW, quads_per_row, stages;      // output OH x OW: D x D when resampling, else H x W
};

__device__ __forceinline__ bool in_range(int v, int lo, int hi) { return v >= lo && v < hi; }

// One lane: four consecutive output pixels of one row, the part plane and the three colour planes.  256 lanes per workgroup, grid
// (quads / 256, B).  No lane leaves before the barrier of the part counts.
__global__ __launch_bounds__(256) void train_crop_augment_kernel(const CropArgs A) {
    __shared__ int s_cnt[TF_PARTS];
    const int b = blockIdx.y, OH = A.OH, OW = A.OW, H = A.H, W = A.W, st = A.stages;
    if (threadIdx.x < TF_PARTS) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int row = q / A.quads_per_row, col0 = (q - row * A.quads_per_row) * 4;
    const bool active = row < OH;
    const int npx = active ? min(4, OW - col0) : 0;
    const bool resample = st & HPS_TRAIN_RESAMPLE;

    const int32_t* pw = A.plan ? A.plan + (size_t)b * TF_PW : nullptr;
    const float* pf = reinterpret_cast<const float*>(pw);
    uint32_t class_mask = 0;
    if (st & HPS_TRAIN_CLASS_MASK) class_mask |= (uint32_t)pw[PW_SEG_MASK];
    if (st & HPS_TRAIN_CROP_CLASS_MASK) class_mask |= (uint32_t)pw[PW_CROP_MASK];

    const float* part = A.part ? A.part + (size_t)b * A.part_batch_stride : nullptr;
    const float* rgb = A.rgb ? A.rgb + (size_t)b * 3 * H * W : nullptr;
    const size_t plane_in = (size_t)H * W, plane_out = (size_t)OH * OW;

    // the row's source coordinate (F.affine_grid + grid_sample's unnormalise, align_corners = False)
    float t00 = 1.0f, t02 = 0.0f, iy = (float)row;
    if (resample) {
        const float* t = A.theta + (size_t)b * 4;
        t00 = t[0]; t02 = t[1];
        const float yn = ((float)(2 * row + 1) / (float)OH - 1.0f) * t[2] + t[3];
        iy = ((yn + 1.0f) * (float)H - 1.0f) / 2.0f;
    }
    const bool y_ok = iy > -1.0f && iy < (float)H;                 // some bilinear corner row inside the frame
    const float y0f = floorf(iy);
    const int y0 = y_ok ? (int)y0f : 0;
    const float wy1 = iy - y0f, wy0 = (y0f + 1.0f) - iy;
    const float yr = rintf(iy);                                    // nearest: round half to even (std::nearbyint)
    const bool yn_ok = yr >= 0.0f && yr <= (float)(H - 1);
    const int yn_i = yn_ok ? (int)yr : 0;

    // this row's occlusion state
    bool seg_row_zero = false, rgb_row_zero = false, box_row = false;
    if (active && (st & HPS_TRAIN_SEG_OCCLUDE)) {
        box_row = in_range(row, pw[PW_BOX], pw[PW_BOX + 1]);
        seg_row_zero = in_range(row, pw[PW_SEG_OCC], pw[PW_SEG_OCC + 1]) || in_range(row, pw[PW_SEG_OCC + 2], pw[PW_SEG_OCC + 3]);
    }
    if (active && (st & HPS_TRAIN_RGB_OCCLUDE))
        rgb_row_zero = in_range(row, pw[PW_RGB_OCC], pw[PW_RGB_OCC + 1]) || in_range(row, pw[PW_RGB_OCC + 2], pw[PW_RGB_OCC + 3]);

    // the background quad, one 16-byte load per plane where the addresses allow (most of a frame is background: the loads are
    // issued before the gathers they would otherwise wait behind); else pixel by pixel below
    float bgv[3][4];
    bool bg_quad = false;
    const float* bg_px = nullptr;
    if (active && (st & HPS_TRAIN_BACKGROUND)) {
        bg_px = A.background + (size_t)b * 3 * plane_out + (size_t)row * OW + col0;
        bg_quad = npx == 4 && ((reinterpret_cast<uintptr_t>(bg_px) | (plane_out * sizeof(float))) & 15) == 0;
        if (bg_quad) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float4 v = *reinterpret_cast<const float4*>(bg_px + c * plane_out);
                bgv[c][0] = v.x; bgv[c][1] = v.y; bgv[c][2] = v.z; bgv[c][3] = v.w;
            }
        }
    }
    float o_crop[4], o_aug[4], o_rgb[3][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o_crop[i] = 0.0f; o_aug[i] = 0.0f;
        o_rgb[0][i] = o_rgb[1][i] = o_rgb[2][i] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= npx) continue;
        const int col = col0 + i;
        float p = 0.0f, c3[3] = {0.0f, 0.0f, 0.0f};
        if (resample) {
            const float xn = ((float)(2 * col + 1) / (float)OW - 1.0f) * t00 + t02;
            const float ix = ((xn + 1.0f) * (float)W - 1.0f) / 2.0f;
            if (part) {
                const float xr = rintf(ix);
                const bool ok = yn_ok && xr >= 0.0f && xr <= (float)(W - 1);
                p = ok ? part[(size_t)yn_i * W + (int)xr] : -1.0f;
            }
            if (rgb && y_ok && ix > -1.0f && ix < (float)W) {
                const float x0f = floorf(ix);
                const int x0 = (int)x0f;
                const float wx1 = ix - x0f, wx0 = (x0f + 1.0f) - ix;
                const bool xa = x0 >= 0, xb = x0 + 1 < W, ya = y0 >= 0, yb = y0 + 1 < H;
                const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
                const size_t o00 = (size_t)y0 * W + x0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float* pl = rgb + c * plane_in;
                    float acc = 0.0f;
                    if (xa && ya) acc = acc + pl[o00] * nw;
                    if (xb && ya) acc = acc + pl[o00 + 1] * ne;
                    if (xa && yb) acc = acc + pl[o00 + W] * sw;
                    if (xb && yb) acc = acc + pl[o00 + W + 1] * se;
                    c3[c] = acc;
                }
            }
        } else {
            const size_t o = (size_t)row * W + col;             // identity: OH == H, OW == W
            if (part) p = part[o];
            if (rgb) {
#pragma unroll
                for (int c = 0; c < 3; ++c) c3[c] = rgb[c * plane_in + o];
            }
        }
        if (st & (HPS_TRAIN_COUNT | HPS_TRAIN_COUNT14)) {
            const int slot = (p >= 0.0f && p < 32.0f && (float)(int)p == p) ? ((st & HPS_TRAIN_COUNT14) ? part14_slot((int)p) : part24_slot((int)p)) : -1;
            if (slot >= 0) atomicAdd(&s_cnt[slot], 1);
        }
        float a = p;
        if (class_in_mask(a, class_mask)) a = 0.0f;
        if (st & HPS_TRAIN_SEG_OCCLUDE) {
            if (box_row && in_range(col, pw[PW_BOX + 2], pw[PW_BOX + 3])) a = 0.0f;
            if (seg_row_zero || in_range(col, pw[PW_SEG_OCC + 4], pw[PW_SEG_OCC + 5])) a = 0.0f;
        }
        if ((st & HPS_TRAIN_BACKGROUND) && a == 0.0f) {
#pragma unroll
            for (int c = 0; c < 3; ++c) c3[c] = bg_quad ? bgv[c][i] : bg_px[c * plane_out + i];
        }
        if (st & HPS_TRAIN_RGB_OCCLUDE) {
            if (rgb_row_zero || in_range(col, pw[PW_RGB_OCC + 4], pw[PW_RGB_OCC + 5])) c3[0] = c3[1] = c3[2] = 0.0f;
        }
        if (st & HPS_TRAIN_RGB_NOISE) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = c3[c] * pf[PW_CHAN + c];
                c3[c] = v > 1.0f ? 1.0f : v;                     // torch.clamp(max=1.0): NaN stays NaN
            }
        }
        o_crop[i] = p; o_aug[i] = a;
        o_rgb[0][i] = c3[0]; o_rgb[1][i] = c3[1]; o_rgb[2][i] = c3[2];
    }

    if (active) {
        const size_t o = (size_t)row * OW + col0;
        auto put = [&](float* base, const float (&v)[4]) {
            float* dst = base + o;
            if (npx == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < npx) dst[i] = v[i];
            }
        };
        if (A.rgb_out) {
#pragma unroll
            for (int c = 0; c < 3; ++c) put(A.rgb_out + ((size_t)b * 3 + c) * plane_out, o_rgb[c]);
        }
        if (A.part_crop) put(A.part_crop + (size_t)b * plane_out, o_crop);
        if (A.part_aug) put(A.part_aug + (size_t)b * plane_out, o_aug);
    }
    __syncthreads();
    if (A.part_counts && threadIdx.x < TF_PARTS && s_cnt[threadIdx.x] != 0)
        atomicAdd(&A.part_counts[(size_t)b * TF_PARTS + threadIdx.x], s_cnt[threadIdx.x]);
}

// ---- hps_train_joints2d: one lane per (image, joint) -----------------------------------------------------------------------------------
__device__ __forceinline__ bool joint_in_frame(float x, float y, float wh) {     // utils/joints2d_utils.py:21-24
    return !(x > wh) && !(y > wh) && !(x < 0.0f) && !(y < 0.0f);
}

__global__ __launch_bounds__(64) void train_joints2d_kernel(const float* __restrict__ joints2d, const uint8_t* __restrict__ vis_in,
                                                            const float* __restrict__ affine, const int32_t* __restrict__ part_counts,
                                                            const int32_t* __restrict__ plan, int B, float img_wh, int count_threshold,
                                                            int stages, float* __restrict__ joints_target,
                                                            float* __restrict__ joints_input, float* __restrict__ vis_f,
                                                            uint8_t* __restrict__ vis_u8) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= B * TF_K) return;
    const int b = e / TF_K, k = e - b * TF_K;
    const float* j = joints2d + (size_t)b * TF_K * 2;
    float a00 = 1.0f, a02 = 0.0f, a11 = 1.0f, a12 = 0.0f;
    if (stages & HPS_TRAIN_J_AFFINE) {
        const float* a = affine + (size_t)b * 6;
        a00 = a[0]; a02 = a[2]; a11 = a[4]; a12 = a[5];
    }
    const bool tf = stages & HPS_TRAIN_J_AFFINE;
    const float x = j[2 * k], y = j[2 * k + 1];
    const float tx = tf ? x * a00 + a02 : x, ty = tf ? y * a11 + a12 : y;
    bool vis = vis_in ? vis_in[e] != 0 : true;
    if (stages & HPS_TRAIN_J_PRE_VIS) vis = vis && joint_in_frame(x, y, img_wh);
    if (stages & HPS_TRAIN_J_POST_VIS) vis = vis && joint_in_frame(tx, ty, img_wh);
    if (stages & HPS_TRAIN_J_OCCLUDED) {                           // utils/joints2d_utils.py:37-43
        int slot = -1;
        switch (k) {
            case 7: slot = 0; break;  case 8: slot = 1; break;  case 9: slot = 5; break;   case 10: slot = 4; break;
            case 13: slot = 2; break; case 14: slot = 3; break; case 15: slot = 7; break;  case 16: slot = 6; break;
            default: break;
        }
        if (slot >= 0) vis = vis && part_counts[(size_t)b * TF_PARTS + slot] > count_threshold;
    }
    float ix = tx, iy = ty;
    const int32_t* pw = plan ? plan + (size_t)b * TF_PW : nullptr;
    const float* pf = reinterpret_cast<const float*>(pw);
    if (stages & HPS_TRAIN_J_SEG_AUG) {
        int src = pw[PW_SWAP + k];
        src = src < 0 ? 0 : (src >= TF_K ? TF_K - 1 : src);
        const float sx = j[2 * src], sy = j[2 * src + 1];
        ix = (tf ? sx * a00 + a02 : sx) + pf[PW_DEV + 2 * k];
        iy = (tf ? sy * a11 + a12 : sy) + pf[PW_DEV + 2 * k + 1];
        if ((pw[PW_INVIS] >> k) & 1) vis = false;
        if (iy > pf[PW_SEG_JT] || iy < pf[PW_SEG_JT + 1] || ix < pf[PW_SEG_JT + 2] || ix > pf[PW_SEG_JT + 3]) vis = false;
    }
    if (stages & HPS_TRAIN_J_RGB_AUG) {
        if (iy > pf[PW_RGB_JT] || iy < pf[PW_RGB_JT + 1] || ix < pf[PW_RGB_JT + 2] || ix > pf[PW_RGB_JT + 3]) vis = false;
    }
    if (joints_target) { joints_target[2 * e] = tx; joints_target[2 * e + 1] = ty; }
    if (joints_input) { joints_input[2 * e] = ix; joints_input[2 * e + 1] = iy; }
    if (vis_f) vis_f[e] = vis ? 1.0f : 0.0f;
    if (vis_u8) vis_u8[e] = vis ? 1 : 0;
}

}  // namespace hps

using namespace hps;

extern "C" int hps_seg_bbox_affine(const float* part, int64_t part_batch_stride, const int32_t* plan, int B, int H, int W, int out_wh,
                                   float orig_scale_factor, int32_t* ws, float* affine, float* theta, int32_t* status,
                                   int32_t* part_counts, hps_stream_t stream) {
    if (!part || !ws || !affine || !theta) return bad_arg("hps_seg_bbox_affine: null pointer");
    if (H <= 0 || W <= 0 || out_wh <= 0 || H > 32768 || W > 32768) return bad_arg("hps_seg_bbox_affine: image size out of range");
    if (part_batch_stride < (int64_t)H * W) return bad_arg("hps_seg_bbox_affine: part_batch_stride smaller than one plane");
    if (B <= 0) return HPS_OK;
    if (B > 65535) return bad_arg("hps_seg_bbox_affine: at most 65535 images");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_bbox_partial_kernel, dim3(TF_CHUNKS, B), dim3(256), 0, st, part, part_batch_stride, plan, H, W, ws);
    int rc = check_launch("hps_seg_bbox_affine");
    if (rc) return rc;
    hipLaunchKernelGGL(seg_bbox_finish_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, st, ws, plan, B, H, W, out_wh, orig_scale_factor,
                       affine, theta, status, part_counts);
    return check_launch("hps_seg_bbox_affine");
}

extern "C" int hps_train_crop_augment(const float* part, int64_t part_batch_stride, const float* rgb, const float* background,
                                      const float* theta, const int32_t* plan, int B, int H, int W, int D, int stages, float* rgb_out,
                                      int32_t* part_counts, float* part_crop, float* part_aug, hps_stream_t stream) {
    const char* who = "hps_train_crop_augment";
    if (!part && !rgb) return bad_arg("hps_train_crop_augment: neither a part plane nor rgb");
    if (H <= 0 || W <= 0 || H > 32768 || W > 32768 || ((stages & HPS_TRAIN_RESAMPLE) && (D <= 0 || D > 32768)))
        return bad_arg("hps_train_crop_augment: image size out of range");
    if (part && part_batch_stride < (int64_t)H * W) return bad_arg("hps_train_crop_augment: part_batch_stride smaller than one plane");
    if (stages & ~HPS_TRAIN_ALL_STAGES) return bad_arg("hps_train_crop_augment: unknown stage bit");
    if ((stages & HPS_TRAIN_RESAMPLE) && !theta) return bad_arg("hps_train_crop_augment: theta needed to resample");
    const int OH = (stages & HPS_TRAIN_RESAMPLE) ? D : H, OW = (stages & HPS_TRAIN_RESAMPLE) ? D : W;
    const int plan_stages = HPS_TRAIN_CLASS_MASK | HPS_TRAIN_CROP_CLASS_MASK | HPS_TRAIN_SEG_OCCLUDE | HPS_TRAIN_RGB_OCCLUDE | HPS_TRAIN_RGB_NOISE;
    if ((stages & plan_stages) && !plan) return bad_arg("hps_train_crop_augment: these stages need the plan");
    if ((stages & HPS_TRAIN_BACKGROUND) && (!background || !part)) return bad_arg("hps_train_crop_augment: the composite needs background and a part plane");
    if ((stages & (HPS_TRAIN_COUNT | HPS_TRAIN_COUNT14)) && (!part_counts || !part)) return bad_arg("hps_train_crop_augment: counting needs part_counts and a part plane");
    if ((rgb_out && !rgb && !(stages & HPS_TRAIN_BACKGROUND)) || ((part_crop || part_aug) && !part)) return bad_arg("hps_train_crop_augment: output without its input");
    if (B <= 0) return HPS_OK;
    if (B > 65535) return bad_arg("hps_train_crop_augment: at most 65535 images");
    CropArgs A{part, part_batch_stride, rgb, background, theta, plan, rgb_out,
               (stages & (HPS_TRAIN_COUNT | HPS_TRAIN_COUNT14)) ? part_counts : nullptr, part_crop, part_aug, H, W, OH, OW, ceil_div(OW, 4), stages};
    const long quads = (long)OH * A.quads_per_row;
    hipLaunchKernelGGL(train_crop_augment_kernel, dim3((unsigned)((quads + 255) / 256), B), dim3(256), 0, (hipStream_t)stream, A);
    return check_launch(who);
}

extern "C" int hps_train_joints2d(const float* joints2d, const uint8_t* vis_in, const float* affine, const int32_t* part_counts,
                                  const int32_t* plan, int B, int K, float img_wh, int pixel_count_threshold, int stages,
                                  float* joints_target, float* joints_input, float* vis, uint8_t* vis_u8, hps_stream_t stream) {
    if (!joints2d) return bad_arg("hps_train_joints2d: null pointer");
    if (K != TF_K) return bad_arg("hps_train_joints2d: K must be 17 (COCO joints)");
    if (stages & ~HPS_TRAIN_J_ALL_STAGES) return bad_arg("hps_train_joints2d: unknown stage bit");
    if ((stages & HPS_TRAIN_J_AFFINE) && !affine) return bad_arg("hps_train_joints2d: affine missing");
    if ((stages & HPS_TRAIN_J_OCCLUDED) && !part_counts) return bad_arg("hps_train_joints2d: part_counts missing");
    if ((stages & (HPS_TRAIN_J_SEG_AUG | HPS_TRAIN_J_RGB_AUG)) && !plan) return bad_arg("hps_train_joints2d: these stages need the plan");
    if (B <= 0) return HPS_OK;
    if (B > (1 << 24)) return bad_arg("hps_train_joints2d: too many images");
    hipLaunchKernelGGL(train_joints2d_kernel, dim3(ceil_div(B * TF_K, 64)), dim3(64), 0, (hipStream_t)stream, joints2d, vis_in, affine,
                       part_counts, plan, B, img_wh, pixel_count_threshold, stages, joints_target, joints_input, vis, vis_u8);
    return check_launch("hps_train_joints2d");
}
