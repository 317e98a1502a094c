// hz_iir_math.h -- the arithmetic of the IIR bank (include/hzsdr_iir.h), HIP-free: one step of one second-order section
// in transposed direct form II, every operation one float32 operation rounded by itself.  It compiles as
// __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and both the kernel of hz_iir.hip
// and the restatement of tests/host/iir_ref.cpp evaluate every output through iir_step, so that the host build and the
// device build compute the same bits.  Nothing here calls libm or the device's math library: fmaf and one product.
//
// The loop-carried path of a section is y -> z1 -> y, two dependent fused steps per sample; t and u depend on the
// sample alone (and on z2, a sample old) and sit beside it.  Denormals are kept: neither build flushes them.
#pragma once

#include <math.h>

#include "hz_plan.h"

#if defined(__clang__)
#define HZ_IM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_IM_NO_CONTRACT
#endif

namespace hz {
namespace im {

constexpr int kCoefs = 5;  // b0 b1 b2 a1 a2 of a section, a0 = 1 divided out by the caller

// one sample x through the section c = {b0, b1, b2, a1, a2} with the state (z1, z2) -> y
HZ_HD float iir_step(const float *c, float x, float &z1, float &z2) {
    HZ_IM_NO_CONTRACT
    const float y = fmaf(c[0], x, z1);
    const float t = fmaf(c[1], x, z2);
    z1 = fmaf(-c[3], y, t);
    const float u = c[2] * x;
    z2 = fmaf(-c[4], y, u);
    return y;
}

}  // namespace im
}  // namespace hz
