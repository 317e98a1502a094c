// hz_viterbi_math.h -- the arithmetic of the Viterbi decoder bank (include/hzsdr_viterbi.h), shared by the kernel
// (hz_viterbi.hip) and the host restatement (tests/host/viterbi_ref.cpp): the quantisation of one received value, the
// code bits a trellis branch expects, the branch cost, the puncture walk, the add-compare-select of one state, the
// traceback step, the CRC register and the byte packing.  Everything behind quantise() is integer arithmetic; HIP-free.
#pragma once
#include <math.h>
#include <stdint.h>

#include "hz_framesync_math.h"
#include "hz_plan.h"
#include "hz_received.h"

namespace hz {
namespace vm {

constexpr uint32_t kInf = 1u << 30;      // the start metric of every state but 0
constexpr uint16_t kPunctured = 0xffffu;  // the index table's entry of a position that was not sent

// ---- one received value -> q in -127 ... 127 (0: an erasure): hz_received.h; a hard bit is +-1 ----
using rx::quantise, rx::packed_bit;
HZ_HD int hard(uint32_t bit) { return rx::hard(bit, 1); }
// a step's n values (j >= n: 0) as one word, q_j in byte j
HZ_HD uint32_t pack_q(int q, uint32_t j) { return ((uint32_t)q & 0xffu) << (8u * j); }
HZ_HD int unpack_q(uint32_t qw, uint32_t j) { return (int)(int8_t)(qw >> (8u * j)); }

// ---- the code ----
HZ_HD uint32_t parity(uint32_t v) { return (uint32_t)__builtin_popcount(v) & 1u; }
// the n code bits of the shift register reg = u << (K-1) | state, c_j in bit j
HZ_HD uint32_t expected(uint32_t reg, const uint32_t *gens, uint32_t n, uint32_t inv) {
    uint32_t e = 0;
    for (uint32_t j = 0; j < n; j++) e |= (parity(reg & gens[j]) ^ ((inv >> j) & 1u)) << j;
    return e;
}
// the input bit of state s', its predecessor under decision b, the register of that branch
HZ_HD uint32_t input_of(uint32_t s, uint32_t K) { return s >> (K - 2); }
HZ_HD uint32_t predecessor(uint32_t s, uint32_t b, uint32_t S) { return ((s & (S / 2 - 1)) << 1) | b; }
HZ_HD uint32_t branch_reg(uint32_t s, uint32_t b, uint32_t K) { return (input_of(s, K) << (K - 1)) | predecessor(s, b, 1u << (K - 1)); }

// ---- the metric ----
// one position: |q| when q != 0 and (q > 0) != (c == 1)
HZ_HD uint32_t position_cost(int q, uint32_t c) { return c ? (q < 0 ? (uint32_t)-q : 0u) : (q > 0 ? (uint32_t)q : 0u); }
// a branch that expects the bits e under the step's packed values (punctured positions and j >= n hold 0)
HZ_HD uint32_t branch_cost(uint32_t qw, uint32_t e) {
    uint32_t c = 0;
    for (uint32_t j = 0; j < 4; j++) c += position_cost(unpack_q(qw, j), (e >> j) & 1u);
    return c;
}
// add, compare, select: the tie goes to b = 0; returns the decision
HZ_HD uint32_t acs(uint32_t m0, uint32_t c0, uint32_t m1, uint32_t c1, uint32_t *metric) {
    const uint32_t a = m0 + c0, b = m1 + c1;
    const uint32_t d = b < a ? 1u : 0u;
    *metric = d ? b : a;
    return d;
}

// ---- the puncture walk ----
// is mother-code bit m of a frame transmitted?  (pattern: Lp bits, the first the most significant)
HZ_HD uint32_t transmitted(uint64_t pattern, uint32_t Lp, uint32_t m) { return (uint32_t)(pattern >> (Lp - 1 - m % Lp)) & 1u; }

// ---- the CRC ----
HZ_HD uint32_t crc_mask(uint32_t C) { return C >= 32 ? 0xffffffffu : ((1u << C) - 1u); }
HZ_HD uint32_t crc_step(uint32_t reg, uint32_t bit, uint32_t C, uint32_t poly) {
    const uint32_t top = ((reg >> (C - 1)) & 1u) ^ (bit & 1u);
    reg = (reg << 1) & crc_mask(C);
    return top ? reg ^ poly : reg;
}
// eight steps at once: table[v] is the register that eight steps make of v << (C - 8) under zero bits
HZ_HD uint32_t crc_table_entry(uint32_t v, uint32_t C, uint32_t poly) {
    uint32_t reg = (v << (C - 8)) & crc_mask(C);
    for (int k = 0; k < 8; k++) reg = crc_step(reg, 0, C, poly);
    return reg;
}
// byte: eight bits of the stream, the first the most significant
HZ_HD uint32_t crc_byte(uint32_t reg, uint32_t byte, uint32_t C, const uint32_t *table) {
    return ((reg << 8) & crc_mask(C)) ^ table[((reg >> (C - 8)) ^ byte) & 0xffu];
}

// ---- the decoded bits ----
// Words of the decoded stream hold 64 bits, the EARLIEST in bit 0, as the frame sync bank's do: fm::out_word turns one
// into its 8 output bytes.  Byte b (0: the first) of such a word, most significant bit first:
HZ_HD uint32_t stream_byte(uint64_t out_word, uint32_t b) { return (uint32_t)(out_word >> (8u * b)) & 0xffu; }

}  // namespace vm
}  // namespace hz
