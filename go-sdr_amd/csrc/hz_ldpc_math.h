// hz_ldpc_math.h -- the arithmetic of the LDPC decoder bank (include/hzsdr_ldpc.h), shared by the kernel (hz_ldpc.hip)
// and the host restatement (tests/host/ldpc_ref.cpp): the quantisation of one received value, the value an edge sends
// to its check, the running summary of a check (parity, the two smallest magnitudes, the first edge of the smallest),
// the normalised and offset magnitude and the message an edge gets back.  Everything behind quantise() is integer
// arithmetic; HIP-free.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hz_plan.h"
#include "hz_received.h"

namespace hz {
namespace lm {

constexpr int kClamp = 127;

// ---- one received value -> q in -127 ... 127 (0: an erasure): hz_received.h; a hard bit is +-level ----
using rx::quantise, rx::hard, rx::packed_bit;

// ---- step 1: what an edge sends to its check ----
HZ_HD int to_check(int P, int r) {
    const int t = P - r;
    return t < -kClamp ? -kClamp : (t > kClamp ? kClamp : t);
}

// ---- step 2: a check over its edges in col order ----
struct Check {
    uint32_t par;     // the xor of (t > 0)
    uint32_t m1, m2;  // the two smallest |t|, m1 <= m2
    uint32_t first;   // the number (in col order, from 0) of the first edge that attains m1
};
HZ_HD Check check_start() { return Check{0u, 255u, 255u, 0u}; }
// edge number k of the check brings t
HZ_HD void check_take(Check &c, uint32_t k, int t) {
    const uint32_t a = (uint32_t)(t < 0 ? -t : t);
    c.par ^= t > 0 ? 1u : 0u;
    if (a < c.m1) {
        c.m2 = c.m1, c.m1 = a, c.first = k;
    } else if (a < c.m2) {
        c.m2 = a;
    }
}
// mag' = max(((mag * a) >> 4) - beta, 0)
HZ_HD int scaled(uint32_t mag, uint32_t a, uint32_t beta) {
    const int v = (int)((mag * a) >> 4) - (int)beta;
    return v > 0 ? v : 0;
}
// the message edge number k gets back, its own t in hand; s1 = scaled(m1), s2 = scaled(m2)
HZ_HD int to_variable(const Check &c, uint32_t k, int t, int s1, int s2) {
    const int mag = k == c.first ? s2 : s1;
    return (c.par ^ (t > 0 ? 1u : 0u)) ? mag : -mag;
}

// ---- info ----
HZ_HD uint32_t info_word(uint32_t u, uint32_t iters) { return u | (iters << 16) | (u == 0 ? 1u << 31 : 0u); }

}  // namespace lm
}  // namespace hz
