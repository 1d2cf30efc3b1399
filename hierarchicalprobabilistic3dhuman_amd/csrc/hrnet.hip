// HRNet (models/pose2D_hrnet.py) around the convolutions of csrc/conv_c16.hip: the input pack (NCHW RGB -> the stem's 16-channel
// frame), the fuse step of a HighResolutionModule (:255-264), the output unpack (NHWC frame -> NCHW heat maps) and the op-list entry
// point hps_hrnet_run (include/hps.h).  The three kernels are memory passes: one thread per 16 bytes (pack, fuse) or per float (unpack).
#include "hps_common.h"

namespace hps {

// x (B, 3, H, W) NCHW -> the interior of y (B, H + 2 P, W + 2 P, CP): channels 0..2 and a zero in channel 3 as one 16-byte store;
// channels 4.. of the frame (zero, like the halo) belong to the owner.
__global__ __launch_bounds__(256) void hrnet_pack_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int CP,
                                                         int P, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W);
    const long t = i / W;
    const int h = (int)(t % H);
    const long b = t / H;
    const long plane = (long)H * W;
    const float* s = x + b * 3 * plane + (long)h * W + w;
    const float4 v = make_float4(s[0], s[plane], s[2 * plane], 0.f);
    *reinterpret_cast<float4*>(y + ((b * (H + 2 * P) + h + P) * (long)(W + 2 * P) + w + P) * CP) = v;
}

// the interior of x (B, H + 2 P, W + 2 P, C) NHWC -> y (B, C, H, W) NCHW
__global__ __launch_bounds__(256) void hrnet_unpack_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int C,
                                                           int P, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int w = (int)(i % W);
    long t = i / W;
    const int h = (int)(t % H);
    t /= H;
    const int c = (int)(t % C);
    const long b = t / C;
    y[i] = x[((b * (H + 2 * P) + h + P) * (long)(W + 2 * P) + w + P) * C + c];
}

struct FuseDev {
    const float* term[HPS_HRNET_MAX_TERMS];
    int shift[HPS_HRNET_MAX_TERMS], pad[HPS_HRNET_MAX_TERMS];
    int n;
    float* y;
    int opad, H, W, C4, relu;
};

// y[b, h, w, :] = act(((t0 + t1) + t2) + t3), term k read at (h >> shift_k, w >> shift_k) of its own frame: the additions in term
// order, as models/pose2D_hrnet.py:258-263 adds them.
__global__ __launch_bounds__(256) void hrnet_fuse_kernel(const FuseDev f, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % f.C4);
    long t = i / f.C4;
    const int w = (int)(t % f.W);
    t /= f.W;
    const int h = (int)(t % f.H);
    const long b = t / f.H;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int k = 0; k < HPS_HRNET_MAX_TERMS; ++k) {
        if (k >= f.n) break;
        const int s = f.shift[k], p = f.pad[k];
        const int Hk = (f.H >> s) + 2 * p, Wk = (f.W >> s) + 2 * p;
        const float4 v = *reinterpret_cast<const float4*>(f.term[k] + (((b * Hk + (h >> s) + p) * (long)Wk + (w >> s) + p) * f.C4 + c4) * 4);
        if (k == 0) acc = v;
        else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
    }
    if (f.relu) { acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f); acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f); }
    *reinterpret_cast<float4*>(f.y + (((b * (f.H + 2 * f.opad) + h + f.opad) * (long)(f.W + 2 * f.opad) + w + f.opad) * f.C4 + c4) * 4) = acc;
}

}  // namespace hps

using namespace hps;

extern "C" int hps_hrnet_pack_input(const float* x, float* y, int B, int H, int W, int CP, int P, hps_stream_t stream) {
    if (!x || !y) return bad_arg("hps_hrnet_pack_input: null pointer");
    if (CP < 4 || CP % 4 != 0 || P < 0 || ((uintptr_t)y & 15)) return bad_arg("hps_hrnet_pack_input: CP % 4 == 0, CP >= 4, P >= 0 and a 16-byte aligned frame required");
    if (B <= 0 || H <= 0 || W <= 0) return HPS_OK;
    const long total = (long)B * H * W;
    if ((total + 255) / 256 > 0x7fffffffL) return bad_arg("hps_hrnet_pack_input: tensor too large");
    hipLaunchKernelGGL(hrnet_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, CP, P, total);
    return check_launch("hps_hrnet_pack_input");
}

extern "C" int hps_hrnet_unpack_output(const float* x, float* y, int B, int H, int W, int C, int P, hps_stream_t stream) {
    if (!x || !y) return bad_arg("hps_hrnet_unpack_output: null pointer");
    if (C < 1 || P < 0) return bad_arg("hps_hrnet_unpack_output: C >= 1 and P >= 0 required");
    if (B <= 0 || H <= 0 || W <= 0) return HPS_OK;
    const long total = (long)B * C * H * W;
    if ((total + 255) / 256 > 0x7fffffffL) return bad_arg("hps_hrnet_unpack_output: tensor too large");
    hipLaunchKernelGGL(hrnet_unpack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, P, total);
    return check_launch("hps_hrnet_unpack_output");
}

extern "C" int hps_sizeof_hrnet_fuse_args(void) { return (int)sizeof(hps_hrnet_fuse_args); }

extern "C" int hps_hrnet_fuse(const hps_hrnet_fuse_args* a, hps_stream_t stream) {
    if (!a || !a->y) return bad_arg("hps_hrnet_fuse: null pointer");
    if (a->n_terms < 1 || a->n_terms > HPS_HRNET_MAX_TERMS) return bad_arg("hps_hrnet_fuse: 1 to 4 terms");
    if (a->C < 4 || a->C % 4 != 0 || a->H < 1 || a->W < 1 || a->opad < 0) return bad_arg("hps_hrnet_fuse: C % 4 == 0 and H, W >= 1 required");
    FuseDev f;
    uintptr_t align = (uintptr_t)a->y;
    for (int k = 0; k < HPS_HRNET_MAX_TERMS; ++k) {
        const int kk = k < a->n_terms ? k : 0;
        if (!a->term[kk]) return bad_arg("hps_hrnet_fuse: null pointer (term)");
        if (a->shift[kk] < 0 || a->shift[kk] > 8 || a->pad[kk] < 0 || a->H % (1 << a->shift[kk]) != 0 || a->W % (1 << a->shift[kk]) != 0)
            return bad_arg("hps_hrnet_fuse: a term's shift must divide H and W (0 <= shift <= 8), its halo must be >= 0");
        f.term[k] = a->term[kk]; f.shift[k] = a->shift[kk]; f.pad[k] = a->pad[kk];
        align |= (uintptr_t)a->term[kk];
    }
    if (align & 15) return bad_arg("hps_hrnet_fuse: frames must be 16-byte aligned");
    if (a->B <= 0) return HPS_OK;
    f.n = a->n_terms; f.y = a->y; f.opad = a->opad; f.H = a->H; f.W = a->W; f.C4 = a->C / 4; f.relu = a->relu ? 1 : 0;
    const long total = (long)a->B * a->H * a->W * f.C4;
    if ((total + 255) / 256 > 0x7fffffffL) return bad_arg("hps_hrnet_fuse: tensor too large");
    hipLaunchKernelGGL(hrnet_fuse_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, f, total);
    return check_launch("hps_hrnet_fuse");
}

extern "C" int hps_sizeof_hrnet_op(void) { return (int)sizeof(hps_hrnet_op); }

extern "C" int hps_hrnet_run(const hps_hrnet_op* ops, int n_ops, hps_stream_t stream) {
    if (!ops && n_ops > 0) return bad_arg("hps_hrnet_run: null op list");
    for (int i = 0; i < n_ops; ++i) {
        const hps_hrnet_op& o = ops[i];
        int rc;
        switch (o.kind) {
            case HPS_HRNET_PACK: rc = hps_hrnet_pack_input(o.x, o.y, o.B, o.H, o.W, o.C, o.P, stream); break;
            case HPS_HRNET_CONV: rc = hps_conv2d_bn_act_c16(o.conv, o.n_problems, stream); break;
            case HPS_HRNET_FUSE: rc = hps_hrnet_fuse(&o.fuse, stream); break;
            case HPS_HRNET_UNPACK: rc = hps_hrnet_unpack_output(o.x, o.y, o.B, o.H, o.W, o.C, o.P, stream); break;
            default: return bad_arg("hps_hrnet_run: unknown op kind");
        }
        if (rc != HPS_OK) return rc;
    }
    return HPS_OK;
}
