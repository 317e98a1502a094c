// hz_equalizer_math.h -- the arithmetic of the equalizer bank (include/hzsdr_equalizer.h), HIP-free: one tap's product,
// the error of an output under the three modes, the clip, the track value and one tap's update.  It compiles as
// __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and both the kernel of
// hz_equalizer.hip and the restatement of tests/host/equalizer_ref.cpp evaluate every output, every track value and
// every state word through these functions, so that the host build and the device build compute the same bits.  Nothing
// here calls libm or the device's math library: IEEE float32 *, +, - and fmaf, each correctly rounded by itself,
// copysign, comparisons and selections.
//
// A value is PL floats: PL = 1 a real one, PL = 2 (re, im).  The step of the header, cut where the lanes meet:
//   eq_product  p = w X                       every tap by itself
//   (the sum)   p[i] += p[i ^ s], s = 1, 2, 4 ... < Np: the kernel's lane exchange, the host program's loop -- float
//               addition commutes, so every entry ends with the same bits and y = p[0]
//   eq_error    e from y under the mode, clipped to [-1, 1] component by component
//   eq_gain     g = mu e
//   eq_track    |e|^2 of the clipped error
//   eq_update   w += g conj(X)                every tap by itself
// Every step is written without a branch on a value: the mode is the same for all rows of a bank.
//
// Properties (restated in include/hzsdr_equalizer.h):
//   - denormals are kept: neither build flushes them;
//   - a NaN passes the clip (no comparison with it holds) and stays in its row: y, e, g and every tap of the row become
//     NaNs and stay so until a reset or a set_state;
//   - no value of a row reaches another row, an address or a trip count.
#pragma once

#include <stdint.h>

#include "hz_plan.h"

#if defined(__clang__)
#define HZ_EM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_EM_NO_CONTRACT
#endif

namespace hz {
namespace em {

constexpr int kCma = 0, kDdBpsk = 1, kDdQpsk = 2;  // HZSDR_EQUALIZER_CMA, _DD_BPSK, _DD_QPSK

// the parameters of one row, as the kernel sees them
struct Loop {
    float mu;     // the step
    float level;  // CMA: the modulus squared; DD: the decision's amplitude per component
};

HZ_HD float eq_clip(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// p = w X
template <int PL> HZ_HD void eq_product(const float (&w)[PL], const float (&x)[PL], float (&p)[PL]) {
    HZ_EM_NO_CONTRACT
    if constexpr (PL == 2) {
        p[0] = __builtin_fmaf(-w[1], x[1], w[0] * x[0]);
        p[1] = __builtin_fmaf(w[1], x[0], w[0] * x[1]);
    } else {
        p[0] = w[0] * x[0];
    }
}

// the clipped error of the output y
template <int PL> HZ_HD void eq_error(int mode, const float (&y)[PL], float level, float (&e)[PL]) {
    HZ_EM_NO_CONTRACT
    if constexpr (PL == 2) {
        if (mode == kCma) {
            const float c = level - __builtin_fmaf(y[1], y[1], y[0] * y[0]);
            e[0] = c * y[0];
            e[1] = c * y[1];
        } else {
            e[0] = __builtin_copysignf(level, y[0]) - y[0];
            e[1] = mode == kDdQpsk ? __builtin_copysignf(level, y[1]) - y[1] : -y[1];
        }
        e[0] = eq_clip(e[0]);
        e[1] = eq_clip(e[1]);
    } else {
        if (mode == kCma) {
            const float c = level - y[0] * y[0];
            e[0] = c * y[0];
        } else {
            e[0] = __builtin_copysignf(level, y[0]) - y[0];
        }
        e[0] = eq_clip(e[0]);
    }
}

// g = mu e
template <int PL> HZ_HD void eq_gain(float mu, const float (&e)[PL], float (&g)[PL]) {
    HZ_EM_NO_CONTRACT
    for (int p = 0; p < PL; p++) g[p] = mu * e[p];
}

// the track value: the clipped error's square
template <int PL> HZ_HD float eq_track(const float (&e)[PL]) {
    HZ_EM_NO_CONTRACT
    if constexpr (PL == 2) {
        return __builtin_fmaf(e[1], e[1], e[0] * e[0]);
    } else {
        return e[0] * e[0];
    }
}

// w += g conj(X)
template <int PL> HZ_HD void eq_update(float (&w)[PL], const float (&g)[PL], const float (&x)[PL]) {
    HZ_EM_NO_CONTRACT
    if constexpr (PL == 2) {
        const float re = __builtin_fmaf(g[1], x[1], __builtin_fmaf(g[0], x[0], w[0]));
        const float im = __builtin_fmaf(-g[0], x[1], __builtin_fmaf(g[1], x[0], w[1]));
        w[0] = re;
        w[1] = im;
    } else {
        w[0] = __builtin_fmaf(g[0], x[0], w[0]);
    }
}

}  // namespace em
}  // namespace hz
