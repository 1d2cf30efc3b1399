// What the backward GEMMs of csrc/conv_backward.hip and csrc/conv1x1_backward.hip share: the MFMA accumulator type, the length of a
// summation chain and the register -> row map of a 32x32 result.  One definition: hps_conv1x1_dgrad owes hps_conv_dgrad its bits.
#pragma once
#include "hps_common.h"

namespace hps {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// An MFMA accumulator is a serial fp32 chain; both GEMMs cut theirs into pieces of 64 products (WGRAD_CHAIN pixels, DGRAD_CHAIN output
// channels) and add the pieces in order: the rounding error of a sum of n terms grows like sqrt(n) of the piece, not of the whole.
constexpr int WGRAD_CHAIN = 64;
constexpr int DGRAD_CHAIN = 64;

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
    return z;
}

// row of a 32x32 MFMA result held in register i of lane half h (the column is lane & 31)
__device__ __forceinline__ int mfma_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

}  // namespace hps
