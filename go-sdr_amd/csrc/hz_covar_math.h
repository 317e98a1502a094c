// hz_covar_math.h -- the arithmetic of the covariance bank and the beam scan (include/hzsdr_covar.h), HIP-free: the
// step of a segment's chain, the node of the pairwise tree, the combine that turns the real Gram matrix G into the
// complex covariance R, and the terms of the scan.  It compiles as __host__ __device__ under hipcc and as plain C++17
// under g++ (-ffp-contract=off); hz_covar.hip and tests/host/covar_ref.cpp evaluate every term from this header, so that
// the host build and the device build compute the same bits.
//
// Nothing here calls libm or the device's math library: fmaf where a fused step is written out, one plain float32
// addition or subtraction elsewhere.
#pragma once
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace cv {

struct c32 {
    float re, im;
};

// one snapshot of a segment's chain: g[p][q] += v_p[n] v_q[n], fused.  THE expression one k-slot of the matrix
// instruction must reproduce
HZ_HD float covar_step(float acc, float vp, float vq) { return __builtin_fmaf(vp, vq, acc); }

// one node of the block's tree: the earlier group is the left operand
HZ_HD float covar_node(float left, float right) { return left + right; }

// R[i][j] out of the four entries of G that belong to channels i and j: g00 = G[2i][2j], g11 = G[2i+1][2j+1],
// g10 = G[2i+1][2j], g01 = G[2i][2j+1]; one rounding per component
HZ_HD c32 covar_combine(float g00, float g11, float g10, float g01) { return c32{g00 + g11, g10 - g01}; }

// ---- the scan ----------------------------------------------------------------------------------------------
// t += Q[i][j] conj(w_j): four fused steps, u = conj(w_j)
HZ_HD c32 scan_inner(c32 t, c32 q, c32 w) {
    const float ure = w.re, uim = -w.im;
    t.re = __builtin_fmaf(q.re, ure, t.re);
    t.re = __builtin_fmaf(-q.im, uim, t.re);
    t.im = __builtin_fmaf(q.im, ure, t.im);
    t.im = __builtin_fmaf(q.re, uim, t.im);
    return t;
}
// p += Re(w_i t): two fused steps
HZ_HD float scan_outer(float p, c32 w, c32 t) {
    p = __builtin_fmaf(w.re, t.re, p);
    p = __builtin_fmaf(-w.im, t.im, p);
    return p;
}
// p[g] of one matrix Q (row-major N x N) and one weight vector w: i ascending, inside it j ascending, from +0
HZ_HD float scan_power(const c32 *Q, const c32 *w, uint32_t N) {
    float p = 0.0f;
    for (uint32_t i = 0; i < N; i++) {
        c32 t{0.0f, 0.0f};
        for (uint32_t j = 0; j < N; j++) t = scan_inner(t, Q[i * N + j], w[j]);
        p = scan_outer(p, w[i], t);
    }
    return p;
}

}  // namespace cv
}  // namespace hz
