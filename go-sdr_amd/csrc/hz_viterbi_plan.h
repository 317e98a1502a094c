// hz_viterbi_plan.h -- the host arithmetic of the Viterbi decoder bank (include/hzsdr_viterbi.h), HIP-free so that
// tests/host/viterbi_plan.cpp can run it under the sanitizers: the validation of a bank's configuration, the puncture
// index table, how frames and states are dealt to the lanes of a wave, where the decisions live and the LDS request.
//
// Lanes.  The workgroup is one wave.  S = 2^(K-1) states: S = 64 is one state per lane and one frame per wave; S < 64
// puts G = 64 / S frames side by side, frame g on the lanes [g S, (g + 1) S); S = 128, 256 gives a lane SPL = S / 64
// states, state s on lane s & 63 in register s >> 6.  A wave takes the frame slots [w G, (w + 1) G) (slot = row * cap +
// frame), then those a grid further on: a row's frames may well lie in several waves, and a wave's in several rows.
//
// Decisions.  A step's decisions are SPL words of 64 bits, bit l of word k the decision of the state that lane l holds
// in register k (with G frames side by side a word holds all of them).  A frame's T steps are T SPL words: in the wave's
// LDS where the whole request stays inside the family's budget (FORM_LDS), else in a device scratch of the bank that has
// T SPL words per wave of the grid (FORM_SCRATCH); the traceback then brings them back kChunkSteps steps at a time.
//
// The index table.  idx[t n + j] is the received position that feeds mother-code bit j of step t, or kPunctured: made
// once at create from the pattern, so that the kernel divides nothing.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hz_decodebank_plan.h"
#include "hz_rowwave_plan.h"
#include "hz_viterbi_math.h"

namespace hz {
namespace vp {

using rw::kLanes, rw::kLdsBudget;
using dbp::kBits, dbp::kSoftF32, dbp::kMaxRows, dbp::kMaxFrames;  // HZSDR_VITERBI_BITS, HZSDR_VITERBI_SOFT_F32

constexpr int kTail = 0, kTruncated = 1;    // HZSDR_VITERBI_TAIL, HZSDR_VITERBI_TRUNCATED
constexpr int kFormLds = 1, kFormScratch = 2;
constexpr uint32_t kMinK = 3, kMaxK = 9, kMinRate = 2, kMaxRate = 4, kMaxPattern = 64, kMaxBits = 8192;
constexpr uint32_t kTileSteps = 64;    // the steps whose received values are quantised into LDS together
constexpr uint32_t kChunkSteps = 512;  // FORM_SCRATCH: the steps of decisions the traceback holds in LDS at a time
constexpr uint32_t kWavesLds = 4096, kWavesScratch = 1024;  // the grid at most; a wave walks on from slot to slot

struct Config {
    int kind;
    uint32_t K, n;
    uint32_t gens[kMaxRate];
    uint32_t inv;
    uint64_t pattern;
    uint32_t Lp;
    int term;
    uint64_t D;
    float scale;
    uint32_t C, poly, init, xorout;
};

inline uint64_t steps(const Config &q) { return q.D + (q.term == kTail ? q.K - 1 : 0); }

// nullptr when the configuration makes a bank, else what is wrong with it (the kind is the caller's to check first)
inline const char *check_config(const Config &q) {
    if (q.K < kMinK || q.K > kMaxK) return "3 <= K <= 9";
    if (q.n < kMinRate || q.n > kMaxRate) return "rate 1/n with n = 2, 3 or 4";
    for (uint32_t j = 0; j < q.n; j++)
        if (q.gens[j] == 0 || q.gens[j] >> q.K) return "generators are K-bit words, not zero";
    if (q.inv >> q.n) return "inv has n bits";
    if (q.Lp < q.n || q.Lp > kMaxPattern || q.Lp % q.n) return "n <= pattern bits <= 64, a multiple of n";
    if (q.Lp < 64 && (q.pattern >> q.Lp)) return "a pattern of pattern_bits bits";
    for (uint32_t m = 0; m < q.Lp; m += q.n) {
        uint32_t any = 0;
        for (uint32_t j = 0; j < q.n; j++) any |= vm::transmitted(q.pattern, q.Lp, m + j);
        if (!any) return "every group of n pattern bits has a 1";
    }
    if (q.term != kTail && q.term != kTruncated) return "termination is TAIL or TRUNCATED";
    if (q.D < 1 || q.D > kMaxBits || steps(q) > kMaxBits) return "1 <= D, T <= 8192";
    if (const char *why = q.kind == kSoftF32 ? dbp::check_scale(q.scale) : nullptr) return why;
    if (q.C != 0 && q.C != 8 && q.C != 16 && q.C != 24 && q.C != 32) return "a CRC of 0, 8, 16, 24 or 32 bits";
    if (q.C && q.C >= q.D) return "the CRC is shorter than the data";
    if (q.C && q.C < 32 && ((q.poly | q.init | q.xorout) >> q.C)) return "CRC parameters below 2^C";
    if (!q.C && (q.poly | q.init | q.xorout)) return "CRC parameters without a CRC";
    uint64_t N = 0;
    const uint64_t T = steps(q);
    for (uint64_t m = 0; m < T * q.n; m++) N += vm::transmitted(q.pattern, q.Lp, (uint32_t)(m % q.Lp));
    if (N > kMaxBits) return "N <= 8192 received positions";
    return nullptr;
}

struct Geom {
    uint32_t S, G, SPL, gsz;  // states; frames per wave; states per lane; lanes per frame
    uint32_t T, N, FB, DB, DW;  // steps, received positions, ceil(N / 8), ceil(D / 8), ceil(D / 64)
    uint32_t tiles;             // ceil(T / kTileSteps)
    int form;
    uint32_t chunk;      // steps of decisions in LDS: T (FORM_LDS) or kChunkSteps
    uint32_t max_waves;  // the grid at most
    uint32_t off_tb, off_crc, off_dec;  // LDS, bytes: [0, off_tb) the tile's packed values, one word per frame and step;
                                        // the decoded words, DW per frame; the CRC's byte table; the decisions
    size_t lds_bytes;
    size_t decision_bytes;  // of one frame: T S / 8
    size_t scratch_words;   // FORM_SCRATCH: max_waves * T * SPL, else 0
};

// a checked configuration (out of line, as build_index is: both stay in the library's symbol table, where the compiler
// had left them before the create shrank around them)
__attribute__((noinline)) inline Geom geom(const Config &q) {
    Geom g{};
    g.S = 1u << (q.K - 1);
    g.G = g.S < kLanes ? kLanes / g.S : 1;
    g.SPL = g.S > kLanes ? g.S / kLanes : 1;
    g.gsz = g.S < kLanes ? g.S : kLanes;
    g.T = (uint32_t)steps(q);
    for (uint32_t m = 0; m < g.T * q.n; m++) g.N += vm::transmitted(q.pattern, q.Lp, m);
    g.FB = dbp::packed_bytes(g.N), g.DB = dbp::packed_bytes((uint32_t)q.D), g.DW = ((uint32_t)q.D + 63) / 64;
    g.tiles = (g.T + kTileSteps - 1) / kTileSteps;
    g.off_tb = g.G * kTileSteps * 4;
    g.off_crc = g.off_tb + g.G * g.DW * 8;
    g.off_dec = g.off_crc + (q.C ? 256 * 4 : 0);
    const size_t whole = (size_t)g.off_dec + (size_t)g.T * g.SPL * 8;
    g.form = whole <= kLdsBudget ? kFormLds : kFormScratch;
    g.chunk = g.form == kFormLds ? g.T : kChunkSteps;
    g.lds_bytes = (size_t)g.off_dec + (size_t)g.chunk * g.SPL * 8;
    g.max_waves = g.form == kFormLds ? kWavesLds : kWavesScratch;
    g.decision_bytes = (size_t)g.T * g.S / 8;
    g.scratch_words = g.form == kFormScratch ? (size_t)g.max_waves * g.T * g.SPL : 0;
    return g;
}

// the waves of a call over `slots` frame slots
inline uint32_t waves_for(const Geom &g, size_t slots) {
    const size_t w = (slots + g.G - 1) / g.G;
    return (uint32_t)(w < g.max_waves ? w : g.max_waves);
}

// idx: T n entries
__attribute__((noinline)) inline void build_index(const Config &q, const Geom &g, std::vector<uint16_t> &idx) {
    idx.assign((size_t)g.T * q.n, vm::kPunctured);
    uint32_t at = 0, phase = 0;  // phase: m mod Lp, carried so that nothing is divided here either
    for (uint32_t t = 0; t < g.T; t++) {
        for (uint32_t j = 0; j < q.n; j++) {
            if ((q.pattern >> (q.Lp - 1 - phase)) & 1u) idx[(size_t)t * q.n + j] = (uint16_t)at++;
            if (++phase == q.Lp) phase = 0;
        }
    }
}

// ---- where a decision lies ----
// the word of state s at step t of the decisions held from step t0 on, and its bit (gbase: the frame's first lane)
HZ_HD uint32_t dec_word(uint32_t t, uint32_t t0, uint32_t s, uint32_t SPL) { return (t - t0) * SPL + (s >> 6); }
HZ_HD uint32_t dec_bit(uint32_t gbase, uint32_t s) { return gbase + (s & 63u); }
// the lane and the register that hold state s of the frame on the lanes from gbase on
HZ_HD uint32_t state_lane(uint32_t gbase, uint32_t s) { return gbase + (s & 63u); }
HZ_HD uint32_t state_reg(uint32_t s) { return s >> 6; }
// the state in register k of the frame's lane sl
HZ_HD uint32_t lane_state(uint32_t k, uint32_t sl) { return k * kLanes + sl; }
// The predecessors of the lane's states.  The states of registers k and k + SPL / 2 differ in their input bit alone and
// share the pair of predecessors number h = pair_of(k): p_b lives on lane pred_lane(b) in register pred_reg(h) --
// 2 h or 2 h + 1 by the lane's half (SPL = 1: register 0, and the lane stays inside the frame's group).
HZ_HD uint32_t pair_of(uint32_t k, uint32_t SPL) { return SPL > 1 ? (k & (SPL / 2 - 1)) : 0u; }
HZ_HD uint32_t pred_lane(uint32_t gbase, uint32_t sl, uint32_t b, uint32_t S, uint32_t SPL) {
    return SPL > 1 ? ((2u * sl + b) & 63u) : gbase + vm::predecessor(sl, b, S);
}
HZ_HD uint32_t pred_reg(uint32_t h, uint32_t sl, uint32_t SPL) { return SPL > 1 ? 2u * h + (sl >> 5) : 0u; }

}  // namespace vp
}  // namespace hz
