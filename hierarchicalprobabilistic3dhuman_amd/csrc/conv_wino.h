// What the Winograd layer kernel (conv_wino.hip) and the earlier forms kept beside it in the dev library (conv_wino_dev.hip) share:
// the sizes of an item, the geometry record both kernels take, and the host code that checks a call and fills that record.
#pragma once

#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WC = 64;            // output channels per item
constexpr int WK = 8;             // input channels per chunk
constexpr int W_OPER = 16 * 2 * 64 * 4;                   // floats of one operand chunk: [16 positions][2 k-quads][64 rows][4]
constexpr int W_WIN = 18 * 18;                            // pixels of the raw input window of an item
constexpr int W_RAW = W_WIN * WK;                         // floats of one raw window chunk (10 368 bytes)
constexpr int W_RAW_PIECES = (W_WIN * 2 + 63) / 64;       // 1 KiB DMA pieces of a raw window chunk (11, the last one partial)

struct WinoGeom {
    int in_row, in_img;           // input frame pitches in floats: (W + 2 ipad) * Cin, (H + 2 ipad) * that
    int out_row, out_img;         // output frame pitches
    int ipad, opad;
    int blocks_x, blocks_img;     // 8 x 8-tile blocks per row / per image
    int Cin, Cout, n_ct, relu;
    int items;                    // B * blocks_img * n_ct  (quad geometry: ceil(B / 4) * n_ct * ksplit)
    unsigned magic_ct, magic_img, magic_x;
    // quad geometry (8 x 8 maps, four images per item, K split into slices that write raw partial sums)
    int B, ksplit, cps, raw;      // images, K slices, chunks per slice, raw = 1: store Y without BatchNorm / residual / ReLU
    unsigned magic_ks;
};

__device__ __forceinline__ unsigned wino_div(unsigned n, unsigned d, unsigned magic) {
    unsigned q = __umulhi(n, magic);
    if (n - q * d >= d) ++q;
    return q;
}

inline unsigned wino_magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ull / d); }

// conv_wino.hip: K slices of the quad geometry for a layer with Cin input channels
int wino_quad_ksplit(int Cin);

// Checks the arguments of a Winograd layer call and fills g.  B <= 0 is no error and leaves g.items = 0: nothing to launch.
// The quad geometry (H = W = 8) gets the pitches of the raw partial sums (slice, image, 8, 8, Cout) that its kernel writes.
inline int wino_geom(WinoGeom& g, const float* x, const float* u, const float* scale, const float* shift, const float* y, int B, int H,
                     int W, int ipad, int Cin, int Cout, int opad, int relu, const float* splitk_ws) {
    g.items = 0;
    if (!x || !u || !scale || !shift || !y) return bad_arg("hps_conv3x3_winograd: null pointer");
    if (B <= 0) return HPS_OK;
    const bool quad = H == 8 && W == 8;
    if (!quad && (H <= 0 || W <= 0 || (H % 16) || (W % 16)))
        return bad_arg("hps_conv3x3_winograd: H and W must be multiples of 16 (8 x 8 blocks of 2 x 2 tiles), or H = W = 8");
    if (Cin <= 0 || Cin % WK != 0 || Cout <= 0 || Cout % WC != 0) return bad_arg("hps_conv3x3_winograd: Cin % 8 == 0 and Cout % 64 == 0 required");
    if (ipad < 1 || opad < 0) return bad_arg("hps_conv3x3_winograd: the input frame needs a halo of at least one pixel");
    if ((size_t)B * (H + 2 * ipad) * (W + 2 * ipad) * Cin * 4 >= 0xffffffffull || (size_t)B * (H + 2 * opad) * (W + 2 * opad) * Cout * 4 >= 0xffffffffull)
        return bad_arg("hps_conv3x3_winograd: tensor exceeds the 32-bit lane offsets");
    if (quad && !splitk_ws) return bad_arg("hps_conv3x3_winograd: 8 x 8 maps need splitk_ws (hps_conv3x3_winograd_workspace bytes)");
    g.in_row = (W + 2 * ipad) * Cin;
    g.in_img = (H + 2 * ipad) * g.in_row;
    g.out_row = (W + 2 * opad) * Cout;
    g.out_img = (H + 2 * opad) * g.out_row;
    g.ipad = ipad; g.opad = opad;
    g.blocks_x = W / 16;
    g.blocks_img = (H / 16) * (W / 16);
    g.Cin = Cin; g.Cout = Cout; g.n_ct = Cout / WC; g.relu = relu;
    g.items = B * g.blocks_img * g.n_ct;
    g.B = B; g.ksplit = 1; g.cps = Cin / WK; g.raw = 0;
    if (quad) {                     // the kernel writes raw partial sums (slice, image, 8, 8, Cout); the second pass finishes
        g.ksplit = wino_quad_ksplit(Cin);
        g.cps = Cin / WK / g.ksplit;
        g.raw = 1;
        g.out_row = 8 * Cout; g.out_img = 64 * Cout; g.opad = 0;
        g.items = ((B + 3) / 4) * g.n_ct * g.ksplit;
    }
    g.magic_ct = wino_magic((unsigned)g.n_ct);
    g.magic_img = wino_magic((unsigned)g.blocks_img);
    g.magic_x = wino_magic((unsigned)g.blocks_x);
    g.magic_ks = wino_magic((unsigned)g.ksplit);
    return HPS_OK;
}

constexpr size_t W_LDS_BYTES = (size_t)(4 * W_OPER + 3 * W_RAW) * sizeof(float);       // sA[2] | sB[2] | raw[3]: 162 176 bytes

// conv_wino.hip: the product form.  grid_cap: workgroups of the persistent grid (dev entry only), 0 = one per CU.
int wino_launch(const float* x, const float* u, const float* scale, const float* shift, const float* residual, float* y, int B, int H, int W,
                int ipad, int Cin, int Cout, int opad, int relu, float* splitk_ws, hps_stream_t stream, int grid_cap);
// conv_wino.hip: the second pass of the quad geometry (wino_splitk_epilogue_kernel) on ksplit slices of (B, 8, 8, Cout) partial sums
int wino_sum_slices(const float* splitk_ws, const float* scale, const float* shift, const float* residual, float* y, int B, int ksplit,
                    int Cout, int opad, int relu, hps_stream_t stream);

}  // namespace hps
