// hz_received.h -- what a received value means to every decoder bank that takes the soft frame bank's floats or the frame
// sync bank's packed bits (hz_viterbi_math.h, hz_ldpc_math.h), written once so that the banks cannot drift apart.
// HIP-free; shared by the kernels and the host restatements of tests/host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace rx {

// ---- one received value -> q in -127 ... 127 (0: an erasure) ----
// each step is ONE float32 operation; a NaN gives 0, +-infinity +-127, -0 gives 0
HZ_HD int quantise(float x, float scale) {
    const float y = x * scale;
    if (y != y) return 0;
    return (int)rintf(fminf(fmaxf(y, -127.0f), 127.0f));
}
// a hard bit at the confidence `level`
HZ_HD int hard(uint32_t bit, int level) { return bit ? level : -level; }
// bit k (0: the first) of a frame of packed bits, most significant bit first
HZ_HD uint32_t packed_bit(const uint8_t *bytes, uint32_t k) { return (uint32_t)(bytes[k >> 3] >> (7u - (k & 7u))) & 1u; }

}  // namespace rx
}  // namespace hz
