// hz_hdlc_math.h -- the arithmetic of the HDLC deframer bank (include/hzsdr_hdlc.h), shared by the kernel (hz_hdlc.hip),
// the host restatement (tests/host/hdlc_ref.cpp) and the walk of tests/host/hdlc_plan.cpp: the two event tests, the
// stuffed-bit test, the FCS step, and the word forms of them that the kernel evaluates 64 bits at a time.  The decision
// of a float and the differential decodings are hz_framesync_math.h's, as they are.  Everything is integer arithmetic on
// decided bits; HIP-free.
//
// A word of the bit stream holds 64 consecutive bits, the EARLIEST in bit 0 (hz_framesync_math.h).  An 8-bit window
// b[i-7 ... i] has b[i-7] in bit 0, so the flag 0,1,1,1,1,1,1,0 is 0x7E and the abort 0,1,1,1,1,1,1,1 is 0xFE.
#pragma once
#include <stdint.h>

#include "hz_framesync_math.h"

namespace hz {
namespace hm {

constexpr uint32_t kFlag = 0x7Eu, kAbort = 0xFEu;
constexpr uint32_t kPoly16 = 0x8408u, kInit16 = 0xFFFFu, kGood16 = 0xF0B8u;
constexpr uint32_t kPoly32 = 0xEDB88320u, kInit32 = 0xFFFFFFFFu, kGood32 = 0xDEBB20E3u;

// ---- bit by bit: the definition ----

// the window b[i-7 ... i], b[i-7] in bit 0
HZ_HD bool is_flag(uint32_t window) { return (window & 0xFFu) == kFlag; }
HZ_HD bool is_abort(uint32_t window) { return (window & 0xFFu) == kAbort; }
// bit i of a span is stuffed when it is 0 behind five 1s; before5: b[i-5 ... i-1], b[i-5] in bit 0
HZ_HD bool is_stuffed(uint32_t bit, uint32_t before5) { return bit == 0 && (before5 & 31u) == 31u; }
// fcs: 16 or 32
HZ_HD uint32_t fcs_poly(uint32_t fcs) { return fcs == 16 ? kPoly16 : kPoly32; }
HZ_HD uint32_t fcs_init(uint32_t fcs) { return fcs == 16 ? kInit16 : kInit32; }
HZ_HD uint32_t fcs_good(uint32_t fcs) { return fcs == 16 ? kGood16 : kGood32; }
// one frame bit through the register
HZ_HD uint32_t fcs_step(uint32_t c, uint32_t bit, uint32_t poly) { return (c >> 1) ^ (((c ^ bit) & 1u) ? poly : 0u); }

// ---- word by word: what the kernel evaluates ----

// the stuffed bits of 64 span bits; before5: the five span bits in front of the word (0 in front of the span)
HZ_HD uint64_t stuffed_mask(uint64_t w, uint32_t before5) {
    const uint64_t p = before5 & 31u;
    uint64_t m = ~w;
    for (uint32_t k = 1; k <= 5; k++) m &= (w << k) | (p >> (5 - k));  // bit i: b[i - k]
    return m;
}
// w with the bits of `mask` deleted, the bits above them moved down; the top popcount(mask) bits are 0
HZ_HD uint64_t delete_bits(uint64_t w, uint64_t mask) {
    while (mask) {  // from the highest down: the positions below stay where they are
        const uint32_t p = 63u - (uint32_t)__builtin_clzll(mask);
        const uint64_t low = fm::low_mask(p);
        w = (w & low) | ((w >> 1) & ~low);
        mask &= low;
    }
    return w;
}
// `bits` (0 ... 64) frame bits of w, the earliest in bit 0, through the register
HZ_HD uint32_t fcs_word(uint32_t c, uint64_t w, uint32_t bits, uint32_t poly) {
    for (uint32_t k = 0; k < bits; k++) {
        c = (c >> 1) ^ (poly & (0u - ((c ^ (uint32_t)(w >> k)) & 1u)));
    }
    return c;
}
// the register behind 8 zero bits from c = e: the entry e of the byte table; and one frame byte through the table
HZ_HD uint32_t fcs_table_entry(uint32_t e, uint32_t poly) { return fcs_word(e, 0, 8, poly); }
HZ_HD uint32_t fcs_byte(uint32_t c, uint32_t byte, const uint32_t *table) { return (c >> 8) ^ table[(c ^ byte) & 0xFFu]; }
// The register is linear in the bits: behind k zero bits a register c is c * x^k modulo the polynomial, in the
// reflected form in which bit fcs - 1 is x^0.  mulmod is that product; next_power is a * x.
HZ_HD uint32_t fcs_next_power(uint32_t a, uint32_t poly) { return (a >> 1) ^ (poly & (0u - (a & 1u))); }
HZ_HD uint32_t fcs_mulmod(uint32_t a, uint32_t b, uint32_t fcs, uint32_t poly) {
    uint32_t p = 0;
    for (uint32_t m = 1u << (fcs - 1); m; m >>= 1) {
        p ^= b & (0u - ((a & m) ? 1u : 0u));
        b = fcs_next_power(b, poly);
    }
    return p;
}

}  // namespace hm
}  // namespace hz
