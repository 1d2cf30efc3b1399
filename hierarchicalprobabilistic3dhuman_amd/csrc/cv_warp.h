// cv2.warpAffine's fixed-point source positions, restated as we understand them from OpenCV's sources (NOT run against OpenCV itself:
// it is not available where this was written).  One reading, shared by csrc/visualise.hip (hps_vis_uncrop) and csrc/data_layer.hip
// (hps_eval_crop_u8); tests/vis_scenario.py (warp_positions) is its NumPy twin.  Include from a file compiled with -ffp-contract=off:
// every product below rounds on its own.
#pragma once
#include "hps_common.h"

namespace hps {

__device__ __forceinline__ int cv_round(double v) {      // saturate_cast<int>(double)
    return (int)rint(fmin(fmax(v, -2147483648.0), 2147483647.0));
}

// The (2,3) matrix M = [m0 m1 m2; m3 m4 m5] inverted in float64, as warpAffine does without WARP_INVERSE_MAP
struct WarpInverse {
    double m0, m1, b1, m3, m4, b2;
};

__device__ __forceinline__ WarpInverse warp_invert(double M0, double M1, double M2, double M3, double M4, double M5) {
    double Dt = M0 * M4 - M1 * M3;
    Dt = Dt != 0.0 ? 1.0 / Dt : 0.0;
    const double A11 = M4 * Dt, A22 = M0 * Dt;
    M0 = A11; M1 *= -Dt; M3 *= -Dt; M4 = A22;
    WarpInverse A;
    A.m0 = M0; A.m1 = M1; A.m3 = M3; A.m4 = M4;
    A.b1 = -M0 * M2 - M1 * M5;
    A.b2 = -M3 * M2 - M4 * M5;
    return A;
}

// AB_BITS = 10: per column rint(M x 1024), per row rint((M y + t) 1024), added in 32-bit (wrapping) integers; the rounding offset of
// the interpolation comes on top
struct WarpFixed {
    unsigned x, y;
};

__device__ __forceinline__ WarpFixed warp_fixed(const WarpInverse& A, int x, int y) {
    const unsigned ax = (unsigned)cv_round(A.m0 * x * 1024.0), ay = (unsigned)cv_round(A.m3 * x * 1024.0);
    const unsigned rx = (unsigned)cv_round((A.m1 * y + A.b1) * 1024.0), ry = (unsigned)cv_round((A.m4 * y + A.b2) * 1024.0);
    WarpFixed p;
    p.x = rx + ax; p.y = ry + ay;
    return p;
}

// INTER_NEAREST: + 512, >> 10
__device__ __forceinline__ void warp_nearest(const WarpFixed p, int& nx, int& ny) {
    nx = (int)(p.x + 512u) >> 10;
    ny = (int)(p.y + 512u) >> 10;
}

// INTER_LINEAR: + 16, >> 5; the index is >> 5 (a short), the fraction & 31 thirty-seconds
__device__ __forceinline__ void warp_linear(const WarpFixed p, int& sx, int& sy, int& fx, int& fy) {
    const int lx = (int)(p.x + 16u) >> 5, ly = (int)(p.y + 16u) >> 5;
    sx = max(-32768, min(32767, lx >> 5));
    sy = max(-32768, min(32767, ly >> 5));
    fx = lx & 31;
    fy = ly & 31;
}

}  // namespace hps
