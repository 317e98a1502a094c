// hz_framesync_math.h -- the arithmetic of the frame sync bank (include/hzsdr_framesync.h), shared by the kernel
// (hz_framesync.hip) and the host restatement (tests/host/framesync_ref.cpp): the decision of one float, the
// differential decodings, the payload maps, and the word forms of them that the kernel evaluates 64 bits at a time.
// Everything is integer arithmetic on decided bits; HIP-free.
//
// A word of the bit stream holds 64 consecutive bits, the EARLIEST in bit 0 (the order __ballot gives with lane =
// float).  The caller's sync words and mask have the first-received bit as the most significant of their W bits:
// reverse_bits turns them into the stream's order once, at create.
#pragma once
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace fm {

// ---- bit by bit: the definition ----

// the raw decision of one float32, from its bit pattern: 1 when the sign bit is clear (-0 decides 0, a NaN by its sign)
HZ_HD uint32_t decide(uint32_t float_bits) { return (float_bits >> 31) ^ 1u; }
// the bit behind the differential decoding: diff 0 plain, 1 d ^ prev, 2 the complement of that (NRZI)
HZ_HD uint32_t diff_bit(uint32_t d, uint32_t prev, int diff) { return diff == 0 ? d : (diff == 1 ? d ^ prev : 1u ^ d ^ prev); }
// payload maps: B = 1: 0 identity, 1 inverted
HZ_HD uint32_t map_bit(uint32_t b, int map) { return b ^ (uint32_t)(map & 1); }
// B = 2, q = 0 ... 3: q times (b0, b1) -> (b1, !b0); returns b0' | b1' << 1 of b0 | b1 << 1
HZ_HD uint32_t map_dibit(uint32_t d, int q) {
    uint32_t b0 = d & 1u, b1 = (d >> 1) & 1u;
    for (int k = 0; k < (q & 3); k++) {
        const uint32_t t = b0;
        b0 = b1, b1 = t ^ 1u;
    }
    return b0 | (b1 << 1);
}

// ---- word by word: what the kernel evaluates ----

constexpr uint64_t kEven = 0x5555555555555555ull;

// the low `bits` bits (0 ... 64)
HZ_HD uint64_t low_mask(uint32_t bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }
// bit k of the result is bit bits - 1 - k of v (bits: 1 ... 64)
HZ_HD uint64_t reverse_bits(uint64_t v, uint32_t bits) {
    uint64_t r = 0;
    for (uint32_t k = 0; k < bits; k++) r |= ((v >> k) & 1ull) << (bits - 1 - k);
    return r;
}
// 64 stream bits from bit `sh` (0 ... 63) of lo on, continued in hi
HZ_HD uint64_t funnel(uint64_t lo, uint64_t hi, uint32_t sh) { return sh ? (lo >> sh) | (hi << (64 - sh)) : lo; }
// a tile's raw decisions -> its bits; carry: the raw decision in front of the tile's first
HZ_HD uint64_t diff_word(uint64_t raw, uint32_t carry, int diff) {
    if (diff == 0) return raw;
    const uint64_t x = raw ^ ((raw << 1) | (uint64_t)(carry & 1u));
    return diff == 1 ? x : ~x;
}
// Hamming distance under the mask; word and mask in the stream's order, bits from W up of the mask 0
HZ_HD uint32_t distance(uint64_t window, uint64_t word, uint64_t mask) { return (uint32_t)__builtin_popcountll((window ^ word) & mask); }
// 64 payload bits through the map; b2: B = 2, bit 0 of x a dibit's first bit
HZ_HD uint64_t map_word(uint64_t x, int map, bool b2) {
    if (!b2) return (map & 1) ? ~x : x;
    const uint64_t e = x & kEven, o = (x >> 1) & kEven;
    switch (map & 3) {
    case 1: return o | ((e ^ kEven) << 1);
    case 2: return (e ^ kEven) | ((o ^ kEven) << 1);
    case 3: return (o ^ kEven) | (e << 1);
    default: return x;
    }
}
// 64 payload bits, the earliest in bit 0, as the 8 output bytes read as a little-endian word: payload bit k in byte
// k / 8, bit 7 - k % 8 (the bits of every byte reversed)
HZ_HD uint64_t out_word(uint64_t x) {
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return x;
}

}  // namespace fm
}  // namespace hz
