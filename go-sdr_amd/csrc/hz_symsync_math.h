// hz_symsync_math.h -- the arithmetic of the symbol-timing recovery bank (include/hzsdr_symsync.h), HIP-free: the
// 4-point cubic Lagrange interpolator and one step of the Gardner loop, every operation one float32 operation rounded by
// itself.  It compiles as __host__ __device__ under hipcc and as plain C++17 under g++ (-ffp-contract=off), and both the
// kernel of hz_symsync.hip and the restatement of tests/host/symsync_ref.cpp evaluate every symbol, every count and
// every state value through sync_step, so that the host build and the device build compute the same bits.  Nothing
// here calls libm or the device's math library: fmaf, sums, products and comparisons.
//
// The step is written without a branch: the interpolant and the loop update are computed for every sample and selected
// by the strobe and the flag, so that the lanes of a wave (lane = row) stay together whatever their clocks do.  What is
// computed and not selected is discarded: it touches neither the state nor the output.
//
// Properties (restated in include/hzsdr_symsync.h):
//   - denormals are kept: neither build flushes them;
//   - bit parity is defined for finite inputs; a NaN or an infinity may silence or garble its own row (a NaN counter
//     compares false with 1 and never strobes again) until reset or set_state, and its bits are not part of the contract;
//   - no value of a row reaches another row, an address or a trip count: the walk is a fixed loop over the samples, at
//     most one strobe per sample, and the flag alternates whatever the data, so a tile of T samples emits at most
//     T / 2 + 1 symbols (hz_symsync_plan.h, tile_symbols).
#pragma once

#include <math.h>
#include <stdint.h>

#include "hz_plan.h"

#if defined(__clang__)
#define HZ_SM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define HZ_SM_NO_CONTRACT
#endif

namespace hz {
namespace sm {

// the loop's constants of one row, as the kernel sees them (derived by hz_symsync_plan.h, derive)
struct Loop {
    float g_mu, g_omega, hmin, hmax;
};

// the kept state of one row with PL planes (1: real, 2: re and im)
template <int PL> struct State {
    float c;        // the counter: samples until the next strobe
    float h;        // the half-period estimate
    uint32_t flag;  // 0: the next strobe is the mid-symbol one, 1: the symbol one
    float yp[PL], ym[PL];         // the last symbol, the last mid-symbol interpolant
    float x1[PL], x2[PL], x3[PL];  // the three latest samples, newest first
};

// the cubic through x3, x2, x1, x0 (oldest first) at x2 + mu (x1 - x2): x2 at mu = 0, x1 at mu = 1
HZ_HD float interp(float x3, float x2, float x1, float x0, float mu) {
    HZ_SM_NO_CONTRACT
    const float c3 = fmaf(0.5f, x2 - x1, (1.0f / 6.0f) * (x0 - x3));
    const float c2 = fmaf(0.5f, x1 + x3, -x2);
    const float c1 = ((x1 - 0.5f * x2) - (1.0f / 3.0f) * x3) - (1.0f / 6.0f) * x0;
    return fmaf(fmaf(fmaf(c3, mu, c2), mu, c1), mu, x2);
}

// the new sample x0 into the row: true when a symbol is emitted, then in y
template <int PL> HZ_HD bool sync_step(State<PL> &s, const Loop &k, const float *x0, float *y) {
    HZ_SM_NO_CONTRACT
    const bool strobe = s.c < 1.0f;  // a strobe lies in [n - 2, n - 1), at the fraction mu = c
    const bool sym = strobe && s.flag != 0u, mid = strobe && s.flag == 0u;
    float v[PL];
    for (int p = 0; p < PL; p++) v[p] = interp(s.x3[p], s.x2[p], s.x1[p], x0[p], s.c);
    float e = (s.yp[0] - v[0]) * s.ym[0];
    if (PL == 2) e = fmaf(s.yp[PL - 1] - v[PL - 1], s.ym[PL - 1], e);
    e = e < -1.0f ? -1.0f : (e > 1.0f ? 1.0f : e);
    float h = fmaf(k.g_omega, e, s.h);
    h = h < k.hmin ? k.hmin : (h > k.hmax ? k.hmax : h);
    const float adv = sym ? fmaf(k.g_mu, e, h) : s.h;
    s.h = sym ? h : s.h;
    for (int p = 0; p < PL; p++) {
        y[p] = v[p];
        s.ym[p] = mid ? v[p] : s.ym[p];
        s.yp[p] = sym ? v[p] : s.yp[p];
    }
    s.flag = strobe ? s.flag ^ 1u : s.flag;
    const float c = strobe ? s.c + adv : s.c;
    s.c = c - 1.0f;
    for (int p = 0; p < PL; p++) {
        s.x3[p] = s.x2[p];
        s.x2[p] = s.x1[p];
        s.x1[p] = x0[p];
    }
    return sym;
}

// The new sample x0 into a row whose sample holds no strobe (c >= 1, or a NaN counter): exactly what sync_step does to
// the state then, and nothing else.  The kernel takes this way when NO lane of the wave has a strobe (a wave-uniform
// test), which is most samples of a wave that owns one row; tests/host/symsync_plan.cpp compares the two bit for bit.
template <int PL> HZ_HD void sync_idle(State<PL> &s, const float *x0) {
    HZ_SM_NO_CONTRACT
    s.c = s.c - 1.0f;
    for (int p = 0; p < PL; p++) {
        s.x3[p] = s.x2[p];
        s.x2[p] = s.x1[p];
        s.x1[p] = x0[p];
    }
}

}  // namespace sm
}  // namespace hz
