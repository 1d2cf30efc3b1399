// The predict visualisations on the device (predict/predict_poseMF_shapeGaussian_net.py:116-147, 174-190, 198-205, 236-333;
// utils/image_utils.py:195-229 with uncrop=True): what lies between hps_render's planes and a PNG.  Three launches, one per entry:
//   hps_vis_views    the vertex and colour buffers of every view of a figure, laid out as ONE hps_render batch;
//   hps_vis_compose  the finished figure, (rows wh, cols wh, 3) uint8, from a list of panels;
//   hps_vis_uncrop   the posed render warped back onto the original photograph, (H, W, 3) uint8.
// The reference does this with fourteen renderer calls, a dozen .cpu().numpy() copies of float images, matplotlib, cv2.warpAffine and
// numpy tiling per image; here only the finished bytes cross to the host.
//
// The reference renders the two T-pose views and the sample sheet through a constant 0.7 UV texture (TexturesUV); here they take a
// constant per-vertex colour (TexturesVertex), so that all views of a figure share one render call.  A constant interpolates to itself
// on either route up to rounding: the texel route forms a + t (b - a) on equal a and b, the vertex route w0 c + w1 c + w2 c with
// w0 + w1 + w2 = 1 up to rounding -- the two differ by the rounding of that sum only.
//
// The warp restates cv2.warpAffine's fixed-point arithmetic as we understand it from OpenCV's sources; like hps_render's rules
// against pytorch3d, these have NOT been run against OpenCV itself (it is not available where this was written).
//
// Bandwidth-bound sweeps: no LDS, no atomics, nothing allocated, bitwise repeatable.  A lane of the two image kernels produces 16
// consecutive BYTES of the interleaved output and stores them as one dwordx4: the output is addressed as a flat run of bytes, so a
// figure row of 3 cols wh bytes that is no multiple of 4 (the 3 x 6 sheet at odd wh) and a panel edge that is not dword-aligned need no
// special case -- a lane's run simply crosses pixels, rows and panels.  Only the last lane of an image whose byte count is no multiple
// of 16 stores dwords and at most three single bytes.  Compiled with -ffp-contract=off: the float32 twin of tests/vis_scenario.py
// rounds every product.
#include "cv_warp.h"
#include "hps_common.h"

namespace hps {

// ---------------------------------------------------------------------------------------------------------------------------------
// views
// ---------------------------------------------------------------------------------------------------------------------------------
struct ViewTable {
    const float* vertices[HPS_VIS_MAX_VIEWS];
    const float* var[HPS_VIS_MAX_VIEWS];
    int yaw[HPS_VIS_MAX_VIEWS];
    int camera[HPS_VIS_MAX_VIEWS];
    float fixed_cam_t[3], fixed_scale, cam_z;
};

__global__ __launch_bounds__(256) void vis_views_kernel(const ViewTable t, const float* __restrict__ lut, float constant, int V,
                                                        const float* __restrict__ cam, float* __restrict__ out_vertices,
                                                        float* __restrict__ out_colours, float* __restrict__ out_cam_t,
                                                        float* __restrict__ out_scale) {
    const int v = blockIdx.x * 256 + threadIdx.x, view = blockIdx.y;
    if (v == 0 && out_cam_t) {
        // :151-154: orthographic_scale = cam[[0, 0]], cam_t = [cam[1], cam[2], 2.5]; or the figure's fixed camera
        const bool own = t.camera[view] != 0;
        out_cam_t[3 * view] = own ? cam[1] : t.fixed_cam_t[0];
        out_cam_t[3 * view + 1] = own ? cam[2] : t.fixed_cam_t[1];
        out_cam_t[3 * view + 2] = own ? t.cam_z : t.fixed_cam_t[2];
        out_scale[2 * view] = out_scale[2 * view + 1] = own ? cam[0] : t.fixed_scale;
    }
    if (v >= V) return;
    const f3 p = reinterpret_cast<const f3*>(t.vertices[view])[v];
    // rotation by pi about x, then yaw times by -pi / 2 about y, the trigonometry exact: signed permutations
    float x = p.x, y = -p.y, z = -p.z;
    for (int k = 0; k < t.yaw[view]; ++k) {
        const float nx = -z;
        z = x;
        x = nx;
    }
    f3 o;
    o.x = x; o.y = y; o.z = z;
    const size_t at = (size_t)view * V + v;
    reinterpret_cast<f3*>(out_vertices)[at] = o;
    f3 c;
    c.x = c.y = c.z = constant;
    if (t.var[view]) {
        // plt.cm.jet(plt.Normalize(0, 0.2, clip=True)(var))[:, :3]: float64 on the float32 variance -- clip, / 0.2, * 256, truncate,
        // 256 -> 255, table look-up, rounded to float32 (the table already is).  NaN is matplotlib's "bad" colour, (0, 0, 0).
        const double d = (double)t.var[view][v];
        if (d != d) {
            c.x = c.y = c.z = 0.0f;
        } else {
            const double n = fmin(fmax(d, 0.0), 0.2) / 0.2;
            int i = (int)(n * 256.0);
            i = i > 255 ? 255 : (i < 0 ? 0 : i);
            c = reinterpret_cast<const f3*>(lut)[i];
        }
    }
    reinterpret_cast<f3*>(out_colours)[at] = c;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// byte runs
// ---------------------------------------------------------------------------------------------------------------------------------
// cv2.imwrite of a float image: saturate_cast<uchar>(255 v), round half to even
__device__ __forceinline__ unsigned to_byte(float v) {
    return (unsigned)fminf(fmaxf(rintf(255.0f * v), 0.0f), 255.0f);
}

__device__ __forceinline__ unsigned pack3(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }

// Bytes [16 lane, 16 lane + 16) of an interleaved (rows, width, 3) uint8 image of nbytes bytes; pixel(y, x) -> r | g << 8 | b << 16.
// `out` is 16-byte aligned (checked on the host).
template <class Pixel>
__device__ __forceinline__ void store_run16(uint8_t* __restrict__ out, int nbytes, int width, int lane, Pixel pixel) {
    const int b0 = lane * 16;
    if (b0 >= nbytes) return;
    int p = b0 / 3, c = b0 - 3 * p;
    int y = p / width, x = p - y * width;
    unsigned cur = pixel(y, x) >> (8 * c);
    unsigned w[4] = {0u, 0u, 0u, 0u};
    const int n = min(16, nbytes - b0);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i < n) {
            w[i >> 2] |= (cur & 255u) << (8 * (i & 3));
            cur >>= 8;
            if (++c == 3 && i + 1 < n) {
                c = 0;
                if (++x == width) { x = 0; ++y; }
                cur = pixel(y, x);
            }
        }
    }
    if (n == 16) {
        *reinterpret_cast<uint4*>(out + b0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int i = 0; i < n / 4; ++i) reinterpret_cast<unsigned*>(out + b0)[i] = w[i];
        for (int i = n & ~3; i < n; ++i) out[b0 + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// compose
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int VIS_EMPTY = -1;

struct ComposeParams {
    int kind[HPS_VIS_MAX_CELLS];       // per grid cell: VIS_EMPTY or HPS_VIS_PANEL_*
    int render[HPS_VIS_MAX_CELLS];
    int rows, cols, wh, D, C, K;
    const float *rgb, *iuv, *crop, *proxy, *joints;
};

// F.interpolate(mode='bilinear', align_corners=False) / cv2.resize(INTER_LINEAR) from side D to side wh: output index i samples
// (i + 0.5) D / wh - 0.5, clamped below at 0; the upper neighbour is clamped to D - 1
struct Tap {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Tap tap(int i, float scale, int D) {
    const float s = fmaxf((i + 0.5f) * scale - 0.5f, 0.0f);
    Tap t;
    t.i0 = min((int)s, D - 1);
    t.i1 = min(t.i0 + 1, D - 1);
    t.l1 = s - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, const Tap& ty, const Tap& tx) {
    return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

__device__ __forceinline__ unsigned crop_pixel(const ComposeParams& P, int r, int c) {
    if (!P.crop) return 0u;
    const float scale = (float)P.D / (float)P.wh;
    const Tap ty = tap(r, scale, P.D), tx = tap(c, scale, P.D);
    unsigned b[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float* s = P.crop + (size_t)ch * P.D * P.D;
        b[ch] = to_byte(bilerp(s[ty.i0 * P.D + tx.i0], s[ty.i0 * P.D + tx.i1], s[ty.i1 * P.D + tx.i0], s[ty.i1 * P.D + tx.i1], ty, tx));
    }
    return pack3(b[0], b[1], b[2]);
}

__device__ __forceinline__ unsigned proxy_pixel(const ComposeParams& P, int r, int c) {
    // cv2.circle(radius 3, filled, (255, 0, 0)) at (int(x wh / D), int(y wh / D)), the products in float64 as Python forms them; the
    // figure is multiplied by 255 afterwards, so a disc pixel saturates to the bytes (255, 0, 0)
    if (P.joints) {
        for (int k = 0; k < P.K; ++k) {
            const double jx = (double)P.joints[2 * k] * (double)P.wh / (double)P.D;
            const double jy = (double)P.joints[2 * k + 1] * (double)P.wh / (double)P.D;
            if (!(fabs(jx) < 1.0e6) || !(fabs(jy) < 1.0e6)) continue;          // NaN, or nowhere near the panel
            const long long dx = c - (int)jx, dy = r - (int)jy;
            if (dx * dx + dy * dy <= 9) return pack3(255u, 0u, 0u);
        }
    }
    const float scale = (float)P.D / (float)P.wh;
    const Tap ty = tap(r, scale, P.D), tx = tap(c, scale, P.D);
    float s00 = 0.0f, s01 = 0.0f, s10 = 0.0f, s11 = 0.0f;
    for (int ch = 0; ch < P.C; ++ch) {
        const float* s = P.proxy + (size_t)ch * P.D * P.D;
        s00 += s[ty.i0 * P.D + tx.i0];
        s01 += s[ty.i0 * P.D + tx.i1];
        s10 += s[ty.i1 * P.D + tx.i0];
        s11 += s[ty.i1 * P.D + tx.i1];
    }
    const unsigned g = to_byte(bilerp(s00, s01, s10, s11, ty, tx));
    return pack3(g, g, g);
}

__global__ __launch_bounds__(256) void vis_compose_kernel(const ComposeParams P, int nbytes, uint8_t* __restrict__ out) {
    const int lane = blockIdx.x * 256 + threadIdx.x;
    store_run16(out, nbytes, P.cols * P.wh, lane, [&](int y, int x) -> unsigned {
        const int cr = y / P.wh, r = y - cr * P.wh, cc = x / P.wh, c = x - cc * P.wh;
        const int cell = cr * P.cols + cc, kind = P.kind[cell];
        if (kind == VIS_EMPTY) return 0u;
        if (kind == HPS_VIS_PANEL_CROP) return crop_pixel(P, r, c);
        if (kind == HPS_VIS_PANEL_PROXY) return proxy_pixel(P, r, c);
        const size_t plane = (size_t)P.wh * P.wh, at = (size_t)P.render[cell] * 3 * plane + (size_t)r * P.wh + c;
        // batch_add_rgb_background on iuv_images[..., 0].round(): the crop where the rounded part label is 0
        if (kind == HPS_VIS_PANEL_RENDER_OVER_CROP && rintf(P.iuv[at]) == 0.0f) return crop_pixel(P, r, c);
        return pack3(to_byte(P.rgb[at]), to_byte(P.rgb[at + plane]), to_byte(P.rgb[at + 2 * plane]));
    });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// uncrop
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float tap_or_zero(const float* __restrict__ s, int wh, int y, int x) {
    return (y >= 0 && y < wh && x >= 0 && x < wh) ? s[y * wh + x] : 0.0f;
}

__global__ __launch_bounds__(256) void vis_uncrop_kernel(const float* __restrict__ rgb, const float* __restrict__ iplane,
                                                         const float* __restrict__ image, const float* __restrict__ bbox_centre,
                                                         const float* __restrict__ bbox_wh, int H, int W, int wh, int nbytes,
                                                         uint8_t* __restrict__ out) {
    const int lane = blockIdx.x * 256 + threadIdx.x;
    if (lane * 16 >= nbytes) return;
    // utils/image_utils.py:197-201 in float32: the matrix that takes the render to the photograph ...
    const float side = bbox_wh[0], owh = (float)wh, ocentre = owh * 0.5f;
    const float f00 = side / owh, f11 = side / owh;
    const float f02 = bbox_centre[1] - (side / owh) * ocentre, f12 = bbox_centre[0] - (side / owh) * ocentre;
    // ... and cv2.warpAffine's inversion of it in float64 (no WARP_INVERSE_MAP); the fixed-point positions are cv_warp.h's
    const WarpInverse A = warp_invert(f00, 0.0, f02, 0.0, f11, f12);
    const size_t src_plane = (size_t)wh * wh, img_plane = (size_t)H * W;
    store_run16(out, nbytes, W, lane, [&](int y, int x) -> unsigned {
        const WarpFixed p = warp_fixed(A, x, y);
        // INTER_NEAREST on the part plane; outside reads 0
        int nx, ny;
        warp_nearest(p, nx, ny);
        const size_t at = (size_t)y * W + x;
        if (tap_or_zero(iplane, wh, ny, nx) == 0.0f)
            return pack3(to_byte(image[at]), to_byte(image[at + img_plane]), to_byte(image[at + 2 * img_plane]));
        // INTER_LINEAR on the colour: the fraction in thirty-seconds
        int sx, sy, ix, iy;
        warp_linear(p, sx, sy, ix, iy);
        const float fx = (float)ix * 0.03125f, fy = (float)iy * 0.03125f;
        const float w00 = (1.0f - fy) * (1.0f - fx), w01 = (1.0f - fy) * fx, w10 = fy * (1.0f - fx), w11 = fy * fx;
        unsigned b[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float* s = rgb + ch * src_plane;
            const float v = tap_or_zero(s, wh, sy, sx) * w00 + tap_or_zero(s, wh, sy, sx + 1) * w01 +
                            tap_or_zero(s, wh, sy + 1, sx) * w10 + tap_or_zero(s, wh, sy + 1, sx + 1) * w11;
            b[ch] = to_byte(v);
        }
        return pack3(b[0], b[1], b[2]);
    });
}

}  // namespace hps

// ---------------------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" int hps_sizeof_vis_views_args(void) { return (int)sizeof(hps_vis_views_args); }
extern "C" int hps_sizeof_vis_compose_args(void) { return (int)sizeof(hps_vis_compose_args); }
extern "C" int hps_sizeof_vis_uncrop_args(void) { return (int)sizeof(hps_vis_uncrop_args); }

extern "C" int hps_vis_views(const hps_vis_views_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_vis_views: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_vis_views_args)) return bad_arg("hps_vis_views: struct_bytes is not sizeof(hps_vis_views_args)");
    if (!a->views || !a->lut || !a->out_vertices || !a->out_colours) return bad_arg("hps_vis_views: null pointer (views, lut, out_vertices, out_colours)");
    if (a->num_views < 1 || a->num_views > HPS_VIS_MAX_VIEWS) return bad_arg("hps_vis_views: num_views in [1, HPS_VIS_MAX_VIEWS]");
    if (a->num_verts < 1 || a->num_verts > (1 << 24)) return bad_arg("hps_vis_views: num_verts in [1, 2^24]");
    ViewTable t;
    for (int i = 0; i < HPS_VIS_MAX_VIEWS; ++i) {
        t.vertices[i] = nullptr; t.var[i] = nullptr; t.yaw[i] = 0; t.camera[i] = 0;
    }
    if ((a->out_cam_t != nullptr) != (a->out_scale != nullptr)) return bad_arg("hps_vis_views: out_cam_t and out_scale come together");
    for (int i = 0; i < a->num_views; ++i) {
        const hps_vis_view& v = a->views[i];
        if (!v.vertices) return bad_arg("hps_vis_views: null pointer (a view's vertices)");
        if (v.yaw < 0 || v.yaw > 3) return bad_arg("hps_vis_views: a view's yaw step is 0, 1, 2 or 3");
        if (v.camera != 0 && v.camera != 1) return bad_arg("hps_vis_views: a view's camera is 0 (fixed) or 1 (predicted)");
        if (v.camera == 1 && a->out_cam_t && !a->cam) return bad_arg("hps_vis_views: null pointer (cam) with a view on the predicted camera");
        t.vertices[i] = v.vertices; t.var[i] = v.var; t.yaw[i] = v.yaw; t.camera[i] = v.camera;
    }
    for (int k = 0; k < 3; ++k) t.fixed_cam_t[k] = a->fixed_cam_t[k];
    t.fixed_scale = a->fixed_scale; t.cam_z = a->cam_z;
    vis_views_kernel<<<dim3(ceil_div(a->num_verts, 256), a->num_views), 256, 0, (hipStream_t)stream>>>(
        t, a->lut, a->constant, a->num_verts, a->cam, a->out_vertices, a->out_colours, a->out_cam_t, a->out_scale);
    return check_launch("hps_vis_views");
}

extern "C" int hps_vis_compose(const hps_vis_compose_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_vis_compose: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_vis_compose_args)) return bad_arg("hps_vis_compose: struct_bytes is not sizeof(hps_vis_compose_args)");
    if (!a->out || (a->num_panels > 0 && !a->panels)) return bad_arg("hps_vis_compose: null pointer (out, panels)");
    if (reinterpret_cast<uintptr_t>(a->out) & 15) return bad_arg("hps_vis_compose: out must be 16-byte aligned");
    if (a->rows < 1 || a->cols < 1 || a->rows * (int64_t)a->cols > HPS_VIS_MAX_CELLS) return bad_arg("hps_vis_compose: rows, cols >= 1, rows cols <= HPS_VIS_MAX_CELLS");
    if (a->wh < 1 || a->wh > 4096) return bad_arg("hps_vis_compose: wh in [1, 4096]");
    const int64_t nbytes = (int64_t)a->rows * a->wh * a->cols * a->wh * 3;
    if (nbytes >= (int64_t)1 << 31) return bad_arg("hps_vis_compose: the figure must be smaller than 2^31 bytes");
    if (a->num_panels < 0 || a->num_panels > a->rows * a->cols) return bad_arg("hps_vis_compose: num_panels in [0, rows cols]");
    ComposeParams P;
    for (int i = 0; i < HPS_VIS_MAX_CELLS; ++i) {
        P.kind[i] = VIS_EMPTY; P.render[i] = 0;
    }
    bool need_render = false, need_iuv = false, need_proxy = false, need_d = false;
    for (int i = 0; i < a->num_panels; ++i) {
        const hps_vis_panel& p = a->panels[i];
        if (p.row < 0 || p.row >= a->rows || p.col < 0 || p.col >= a->cols) return bad_arg("hps_vis_compose: a panel's cell is outside the grid");
        const int cell = p.row * a->cols + p.col;
        if (P.kind[cell] != VIS_EMPTY) return bad_arg("hps_vis_compose: two panels name one cell");
        switch (p.kind) {
            case HPS_VIS_PANEL_RENDER_OVER_CROP: need_iuv = true; need_d = need_d || a->crop;   /* fall through */
            case HPS_VIS_PANEL_RENDER:
                need_render = true;
                if (p.render < 0 || p.render >= a->num_renders) return bad_arg("hps_vis_compose: a panel's render index is outside [0, num_renders)");
                break;
            case HPS_VIS_PANEL_CROP: need_d = need_d || a->crop; break;
            case HPS_VIS_PANEL_PROXY: need_proxy = need_d = true; break;
            default: return bad_arg("hps_vis_compose: unknown panel kind");
        }
        P.kind[cell] = p.kind; P.render[cell] = p.render;
    }
    if (need_render && (!a->rgb || a->num_renders < 1 || a->num_renders > 65535)) return bad_arg("hps_vis_compose: render panels need rgb and num_renders in [1, 65535]");
    if (need_iuv && !a->iuv) return bad_arg("hps_vis_compose: null pointer (iuv) with a RENDER_OVER_CROP panel");
    if (need_proxy && (!a->proxy || a->proxy_channels < 1 || a->proxy_channels > 4096)) return bad_arg("hps_vis_compose: a PROXY panel needs proxy and proxy_channels in [1, 4096]");
    if (need_d && (a->D < 1 || a->D > 8192)) return bad_arg("hps_vis_compose: D in [1, 8192]");
    if (a->joints && (a->num_joints < 0 || a->num_joints > 4096)) return bad_arg("hps_vis_compose: num_joints in [0, 4096]");
    P.rows = a->rows; P.cols = a->cols; P.wh = a->wh; P.D = a->D; P.C = a->proxy_channels; P.K = a->joints ? a->num_joints : 0;
    P.rgb = a->rgb; P.iuv = a->iuv; P.crop = a->crop; P.proxy = a->proxy; P.joints = a->joints;
    const int lanes = (int)((nbytes + 15) / 16);
    vis_compose_kernel<<<ceil_div(lanes, 256), 256, 0, (hipStream_t)stream>>>(P, (int)nbytes, a->out);
    return check_launch("hps_vis_compose");
}

extern "C" int hps_vis_uncrop(const hps_vis_uncrop_args* a, hps_stream_t stream) {
    using namespace hps;
    if (!a) return bad_arg("hps_vis_uncrop: null pointer (args)");
    if (a->struct_bytes != (int)sizeof(hps_vis_uncrop_args)) return bad_arg("hps_vis_uncrop: struct_bytes is not sizeof(hps_vis_uncrop_args)");
    if (!a->rgb || !a->iplane || !a->image || !a->bbox_centre || !a->bbox_wh || !a->out)
        return bad_arg("hps_vis_uncrop: null pointer (rgb, iplane, image, bbox_centre, bbox_wh, out)");
    if (reinterpret_cast<uintptr_t>(a->out) & 15) return bad_arg("hps_vis_uncrop: out must be 16-byte aligned");
    if (a->wh < 1 || a->wh > 4096 || a->H < 1 || a->W < 1 || a->H > 32767 || a->W > 32767) return bad_arg("hps_vis_uncrop: wh in [1, 4096], H and W in [1, 32767]");
    const int64_t nbytes = (int64_t)a->H * a->W * 3;
    if (nbytes >= (int64_t)1 << 31) return bad_arg("hps_vis_uncrop: the picture must be smaller than 2^31 bytes");
    const int lanes = (int)((nbytes + 15) / 16);
    vis_uncrop_kernel<<<ceil_div(lanes, 256), 256, 0, (hipStream_t)stream>>>(a->rgb, a->iplane, a->image, a->bbox_centre, a->bbox_wh, a->H,
                                                                          a->W, a->wh, (int)nbytes, a->out);
    return check_launch("hps_vis_uncrop");
}
