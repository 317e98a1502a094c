// hz_demap_math.h -- the arithmetic of the demapper bank (include/hzsdr_demap.h), HIP-free and shared by the kernel
// (hz_demap.hip) and the host restatement (tests/host/demap_ref.cpp), as hz_received.h is shared: a point's distance, a
// bit's value, what is stored, and the two ways a symbol's 2 m minima are taken.  Every function is a chain of single
// float32 operations; the units that include it are built without contraction.
//
// The minima.  No distance is a NaN or -0 once the symbol has no NaN, so fminf over any order and grouping gives the same
// bits.  symbol_naive takes them point by point and bit by bit: m M minima.  symbol_tree walks the points in blocks of
// C = min(M, 32) consecutive labels; inside a block, for the label's last bit, then the one before it, ...: the minima
// over the even and the odd entries are that bit's two values, then neighbours are merged and the block halves; what is
// left is the block's minimum, which goes to the side of every higher bit that the block's number names.  A block costs
// 3 C - 3 + (m - log2 C) minima: 3 M per symbol at m = 8 where the naive form takes 2048.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace dm {

constexpr uint32_t kNanBits = 0x7FC00000u;  // what every NaN is stored as: the soft frame bank's erasure
constexpr uint32_t kErased = 0xFFFFFFFFu;   // HZSDR_DEMAP_ERASED
constexpr int kTreeBlockBits = 5;

HZ_HD uint32_t bits_of(float v) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}
HZ_HD float float_of(uint32_t u) {
    float v;
    __builtin_memcpy(&v, &u, 4);
    return v;
}

// d_p of a complex and of a real point: two multiplies and one add, not fused
HZ_HD float dist(float xr, float xi, float pr, float pi) {
    const float dr = xr - pr, di = xi - pi;
    const float a = dr * dr, b = di * di;
    return a + b;
}
HZ_HD float dist_real(float x, float p) {
    const float d = x - p;
    return d * d;
}
// bit j (0: the first) of the label p of m bits
HZ_HD uint32_t bit_of(uint32_t p, uint32_t m, uint32_t j) { return (p >> (m - 1u - j)) & 1u; }
// L = (d0 - d1) g; positive says 1
HZ_HD float llr(float d0, float d1, float g) {
    const float t = d0 - d1;
    return t * g;
}
// the bit pattern stored for the value v under the flip bit `flip`: the sign bit flipped, any NaN canonical
HZ_HD uint32_t stored(float v, uint32_t flip) { return v != v ? kNanBits : bits_of(v) ^ (flip << 31); }

// point p of `pts` (P: a pointer to float in any address space): M pairs re, im, or M floats
template <bool CPLX, class P> HZ_HD float point_dist(float xr, float xi, P pts, uint32_t p) {
    if (CPLX) return dist(xr, xi, pts[2 * p], pts[2 * p + 1]);
    return dist_real(xr, pts[p]);
}

// d0[j], d1[j] for the m bits of one symbol, point by point
template <int m, bool CPLX, class P> HZ_HD void symbol_naive(float xr, float xi, P pts, float *d0, float *d1) {
#pragma unroll
    for (int j = 0; j < m; j++) d0[j] = d1[j] = INFINITY;
#pragma unroll
    for (uint32_t p = 0; p < (1u << m); p++) {
        const float d = point_dist<CPLX>(xr, xi, pts, p);
#pragma unroll
        for (int j = 0; j < m; j++) {
            if ((p >> (m - 1 - j)) & 1u)
                d1[j] = fminf(d1[j], d);
            else
                d0[j] = fminf(d0[j], d);
        }
    }
}

// the same values by the two-sided tree over blocks of C labels
template <int m, bool CPLX, class P> HZ_HD void symbol_tree(float xr, float xi, P pts, float *d0, float *d1) {
    constexpr int c = m < kTreeBlockBits ? m : kTreeBlockBits;
    constexpr uint32_t C = 1u << c, M = 1u << m;
#pragma unroll
    for (int j = 0; j < m; j++) d0[j] = d1[j] = INFINITY;
#pragma unroll
    for (uint32_t base = 0; base < M; base += C) {
        float L[C];
#pragma unroll
        for (uint32_t i = 0; i < C; i++) L[i] = point_dist<CPLX>(xr, xi, pts, base + i);
#pragma unroll
        for (int k = 0; k < c; k++) {  // bit m - 1 - k of the label: the parity of an entry's number
            const uint32_t n = C >> k;
            float e = L[0], o = L[1];
#pragma unroll
            for (uint32_t q = 2; q < n; q += 2) e = fminf(e, L[q]), o = fminf(o, L[q + 1]);
            d0[m - 1 - k] = fminf(d0[m - 1 - k], e), d1[m - 1 - k] = fminf(d1[m - 1 - k], o);
#pragma unroll
            for (uint32_t q = 0; q < n / 2; q++) L[q] = fminf(L[2 * q], L[2 * q + 1]);
        }
#pragma unroll
        for (int k = c; k < m; k++) {  // the bits above the block: the block's number
            if ((base >> k) & 1u)
                d1[m - 1 - k] = fminf(d1[m - 1 - k], L[0]);
            else
                d0[m - 1 - k] = fminf(d0[m - 1 - k], L[0]);
        }
    }
}

// the minima a symbol costs in either form (tools/demap_time.py)
constexpr uint32_t naive_minima(uint32_t m) { return m << m; }
constexpr uint32_t tree_minima(uint32_t m) {
    const uint32_t c = m < (uint32_t)kTreeBlockBits ? m : (uint32_t)kTreeBlockBits;
    return ((1u << m) >> c) * (3u * (1u << c) - 3u + (m - c));
}

}  // namespace dm
}  // namespace hz
