// What the Winograd stem kernel (stem_wino.hip) and its profiling ablations kept in the dev library (stem_wino_dev.hip) share: the sizes
// of an item, the table of position rows, the geometry record both kernels take with the host code that checks a call and fills it,
// and the small device helpers of the input transform.
#pragma once

#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float v2f __attribute__((ext_vector_type(2)));

constexpr int SW_C = 18;                         // input channels
constexpr int SW_CO = 64;                        // output channels
constexpr int SW_PAIR = 38;                      // floats per pixel PAIR: 2 x 18 channels + 2 floats of padding (see stem_phase_split_kernel)
constexpr int SW_SLOTS = 90;                     // 16-byte slots per window row: 19 pixels = 9.5 pairs x 152 bytes = 1440
constexpr int SW_ROWF = SW_SLOTS * 4;            // floats per window row in LDS
constexpr int SW_RAW_PIECES = 27;                // 1 KiB DMA pieces per window: 19 rows x 90 slots = 1710 slots (the tail over-reads row 19)
constexpr int SW_RAW_F = SW_RAW_PIECES * 256;    // floats per window buffer
constexpr int SW_POS_F = 1152;                   // floats of one position's filters: [co half][k 0-7 | k 8-15 | k 16-17] x 32 co
constexpr int SW_U_PIECES = 23;                  // a row of five positions = 22.5 KiB
constexpr int SW_U_F = SW_U_PIECES * 256;
constexpr int SW_ROWS = 18;
constexpr int SW_LDS_F = 4 * SW_RAW_F + 2 * SW_U_F;      // 157 696 bytes

// one row of positions: phase, number of x points, the vertical combination, the output fold
struct StemRow {
    int phase, first, nxp, ne;
    int upos;                   // index of the row's first position in the filter array
    int aoff[4];                // window rows of the vertical combination, as float offsets (a * SW_ROWF)
    float coef[4];
    float e0, e1;               // A_y^T[0][i], A_y^T[1][i]
};
// F(2, 4), points 0, 1, -1, 2, inf:  B^T = [2 -1 -2 1 0; 0 -2 -1 1 0; 0 2 -3 1 0; 0 -1 0 1 0; 0 2 -1 -2 1],  A^T = [1 1 1 1 0; 0 1 -1 2 1]
// F(2, 3), points 0, 1, -1, inf:     B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 -1 0 1],                          A^T = [1 1 1 0; 0 1 -1 1]
// Phases in the order (even rows, even columns), (even, odd), (odd, even), (odd, odd); ne = taps of the row's vertical combination
// (unused entries repeat tap 0 with coefficient 0).
// inline: the libraries are built without relocatable device code, so each translation unit that reads the table carries its own copy
// in its code object, and the host side gets no shadow object to collide.  (Not static: hipcc makes a static __constant__ object that
// a kernel's lambdas name visible to the host and then addresses it through the GOT -- one more scalar load per use.)
inline __constant__ StemRow c_stem_rows[SW_ROWS] = {
    {0, 1, 5, 4,  0, {0 * SW_ROWF, 1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF}, {2.0f, -1.0f, -2.0f, 1.0f}, 1.0f, 0.0f},
    {0, 0, 5, 3,  5, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF}, {-2.0f, -1.0f, 1.0f, 0.0f}, 1.0f, 1.0f},
    {0, 0, 5, 3, 10, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF}, {2.0f, -3.0f, 1.0f, 0.0f}, 1.0f, -1.0f},
    {0, 0, 5, 2, 15, {1 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, 2.0f},
    {0, 0, 5, 4, 20, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 4 * SW_ROWF}, {2.0f, -1.0f, -2.0f, 1.0f}, 0.0f, 1.0f},
    {1, 1, 4, 4, 25, {0 * SW_ROWF, 1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF}, {2.0f, -1.0f, -2.0f, 1.0f}, 1.0f, 0.0f},
    {1, 0, 4, 3, 29, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF}, {-2.0f, -1.0f, 1.0f, 0.0f}, 1.0f, 1.0f},
    {1, 0, 4, 3, 33, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF}, {2.0f, -3.0f, 1.0f, 0.0f}, 1.0f, -1.0f},
    {1, 0, 4, 2, 37, {1 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, 2.0f},
    {1, 0, 4, 4, 41, {1 * SW_ROWF, 2 * SW_ROWF, 3 * SW_ROWF, 4 * SW_ROWF}, {2.0f, -1.0f, -2.0f, 1.0f}, 0.0f, 1.0f},
    {2, 1, 5, 2, 45, {0 * SW_ROWF, 2 * SW_ROWF, 0 * SW_ROWF, 0 * SW_ROWF}, {1.0f, -1.0f, 0.0f, 0.0f}, 1.0f, 0.0f},
    {2, 0, 5, 2, 50, {1 * SW_ROWF, 2 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, 1.0f},
    {2, 0, 5, 2, 55, {1 * SW_ROWF, 2 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, -1.0f},
    {2, 0, 5, 2, 60, {1 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 0.0f, 1.0f},
    {3, 1, 4, 2, 65, {0 * SW_ROWF, 2 * SW_ROWF, 0 * SW_ROWF, 0 * SW_ROWF}, {1.0f, -1.0f, 0.0f, 0.0f}, 1.0f, 0.0f},
    {3, 0, 4, 2, 69, {1 * SW_ROWF, 2 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, 1.0f},
    {3, 0, 4, 2, 73, {1 * SW_ROWF, 2 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 1.0f, -1.0f},
    {3, 0, 4, 2, 77, {1 * SW_ROWF, 3 * SW_ROWF, 1 * SW_ROWF, 1 * SW_ROWF}, {-1.0f, 1.0f, 0.0f, 0.0f}, 0.0f, 1.0f}};

struct StemGeom {
    int fr_rowf, fr_phasef, fr_imgf;      // phase frame pitches in floats: row, phase frame, image (4 phase frames)
    int blocks_x, blocks_img, n_items;
    int out_row, out_img, opad, relu;     // output frame (B, Ho + 2 opad, Wo + 2 opad, 64)
    unsigned magic_img, magic_x;
    int in_h, in_w;                       // NCHW-fed form: the input image (B, 18, in_h, in_w)
};

__device__ __forceinline__ unsigned sw_div(unsigned n, unsigned d, unsigned magic) {
    unsigned q = __umulhi(n, magic);
    if (n - q * d >= d) ++q;
    return q;
}
inline unsigned sw_magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)(0x100000000ull / d); }

// Where an item lies: image b, block row by and block column bx of its 16 x 16 output pixels
struct StemItem {
    unsigned b, by, bx;
};
__device__ __forceinline__ StemItem sw_item(int item, const StemGeom& g) {
    const unsigned b = sw_div((unsigned)item, (unsigned)g.blocks_img, g.magic_img), rem = item - b * g.blocks_img;
    const unsigned by = sw_div(rem, (unsigned)g.blocks_x, g.magic_x), bx = rem - by * g.blocks_x;
    return {b, by, bx};
}

// B_x^T applied to the vertical combinations c[0..NXP): position j of the row
template <int NXP, typename T>
__device__ __forceinline__ T sw_horiz(int j, const T (&c)[5]) {
    if (NXP == 5) {
        switch (j) {
            case 0: return 2.0f * (c[0] - c[2]) + (c[3] - c[1]);
            case 1: return (c[3] - c[2]) - 2.0f * c[1];
            case 2: return (2.0f * c[1] + c[3]) - 3.0f * c[2];
            case 3: return c[3] - c[1];
            default: return 2.0f * (c[1] - c[3]) + (c[4] - c[2]);
        }
    }
    switch (j) {
        case 0: return c[0] - c[2];
        case 1: return c[1] + c[2];
        case 2: return c[2] - c[1];
        default: return c[3] - c[1];
    }
}

// One 8-byte LDS read per patch pixel and channel pair, as ds_read_b64 (volatile: hipcc would pair two of them into a
// ds_read2_b64, which the LDS serves at half the rate -- 16-lane groups, banks mod 32 -- and with the tiles' 144-byte pitch at
// half of that again)
__device__ __forceinline__ v2f sw_ld2(const float* p) {
    typedef const volatile __attribute__((address_space(3))) v2f* lds_v2f_t;
    return *(lds_v2f_t)(const __attribute__((address_space(3))) float*)p;
}

// ---- host side ----

// Checks the arguments of a stem call and fills g; pool: out_* describe the frame of the pooled map.  B <= 0 is no error and leaves
// g.n_items = 0: nothing to launch.
inline int stem_geom(StemGeom& g, const float* frames, const float* u, const float* scale, const float* shift, const float* y, int B, int H,
                     int W, int opad, int relu, bool pool) {
    g.n_items = 0;
    if (!frames || !u || !scale || !shift || !y) return bad_arg("hps_stem_winograd: null pointer");
    if (H <= 0 || W <= 0 || (H % 32) || (W % 32)) return bad_arg("hps_stem_winograd: H and W must be multiples of 32 (8 x 8 blocks of 2 x 2-pixel tiles at stride 2)");
    if (opad < 0) return bad_arg("hps_stem_winograd: opad");
    if (B <= 0) return HPS_OK;
    const int Ho = H / 2, Wo = W / 2;
    g.fr_rowf = (Wo + 4) / 2 * SW_PAIR;
    g.fr_phasef = (Ho + 4) * g.fr_rowf;
    g.fr_imgf = 4 * g.fr_phasef;
    g.blocks_x = Wo / 16;
    g.blocks_img = (Ho / 16) * g.blocks_x;
    g.out_row = ((pool ? Wo / 2 : Wo) + 2 * opad) * SW_CO;
    g.out_img = ((pool ? Ho / 2 : Ho) + 2 * opad) * g.out_row;
    g.opad = opad;
    g.relu = relu;
    g.magic_img = sw_magic((unsigned)g.blocks_img);
    g.magic_x = sw_magic((unsigned)g.blocks_x);
    g.in_h = H; g.in_w = W;
    if ((size_t)B * g.fr_imgf * 4 >= 0xffffffffull || (size_t)B * g.out_img * 4 >= 0xffffffffull)
        return bad_arg("hps_stem_winograd: tensor exceeds the 32-bit lane offsets");
    g.n_items = B * g.blocks_img;
    return HPS_OK;
}

// grant_lds + the launch of one stem kernel instantiation on the persistent grid (a workgroup per pair of items, one per CU at most).
// what: the entry point named in an error.  The launch itself is checked by the caller (check_launch).
template <auto Kernel>
inline int stem_launch_kernel(const StemGeom& g, const float* xf, const float* u, const float* scale, const float* shift, float* y, float* side,
                              hps_stream_t stream, const char* what) {
    const size_t lds = (size_t)SW_LDS_F * sizeof(float);
    const int pairs = (g.n_items + 1) / 2;
    const int rc = grant_lds<Kernel>((int)lds, what);
    if (rc != HPS_OK) return rc;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)(pairs < 256 ? pairs : 256)), dim3(512), lds, (hipStream_t)stream, xf, u, scale, shift, y, side, g);
    return HPS_OK;
}

// stem_wino.hip: the product forms.  pool: the max pool in the epilogue (side: hps_stem_pool_side_bytes) and the border pass behind it;
// nchw (pooled form only): xf is the (B, 18, H, W) input itself instead of its phase frames.
int stem_wino_launch(const float* xf, const float* u, const float* scale, const float* shift, float* y, float* side, int B, int H, int W,
                     int opad, int relu, bool pool, bool nchw, hps_stream_t stream);
// stem_wino.hip: the second pass of a pooled form (stem_pool_borders_kernel) on what the first pass left in y and side
int stem_pool_borders_launch(float* y, const float* side, const StemGeom& g, hps_stream_t stream);

}  // namespace hps
