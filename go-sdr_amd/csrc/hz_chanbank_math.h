// hz_chanbank_math.h -- the arithmetic of the channel bank (include/hzsdr_chanbank.h), HIP-free: the term of the fold
// (step 1) and the four-fma term of the product (step 3) as the host restatement evaluates it.  It compiles as
// __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off); the fold of hz_chanbank.hip and
// tests/host/chanbank_ref.cpp evaluate every term from this header, so that the host build and the device build
// compute the same bits.
//
// Nothing here calls libm or the device's math library: fmaf where a fused step is written out.  The DFT table is
// host-made (hz_chanbank_plan.h, float64) and comes in as data.
#pragma once
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace cb {

struct c32 {
    float re, im;
};

// one term of the fold: u += g * x, one fused multiply-add per component
HZ_HD c32 chanbank_fold(c32 acc, float g, c32 x) {
    acc.re = __builtin_fmaf(g, x.re, acc.re);
    acc.im = __builtin_fmaf(g, x.im, acc.im);
    return acc;
}

// one r of the product as a chain of four fused steps: THE expression the matrix product must reproduce
HZ_HD c32 chanbank_term(c32 acc, c32 w, c32 a) {
    acc.re = __builtin_fmaf(w.re, a.re, acc.re);
    acc.re = __builtin_fmaf(-w.im, a.im, acc.re);
    acc.im = __builtin_fmaf(w.im, a.re, acc.im);
    acc.im = __builtin_fmaf(w.re, a.im, acc.im);
    return acc;
}

}  // namespace cb
}  // namespace hz
