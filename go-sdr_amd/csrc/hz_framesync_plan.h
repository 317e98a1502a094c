// hz_framesync_plan.h -- the host arithmetic of the frame sync bank (include/hzsdr_framesync.h), HIP-free so that
// tests/host/framesync_plan.cpp can run it under the sanitizers: the validation of a bank's configuration, the history
// ring and where a window and a payload lie in it, the state's layout on the device and as the ABI moves it.  A wave
// owns one row (geom has why); the kernel is NOT a row-wave kernel: lane = float.
//
// Bits.  A row's bit stream is numbered from 0 at create or reset.  A push numbers the bits it consumes 0 ... m - 1
// (LOCAL bits); a tile is 64 consecutive local bits, tile t the bits 64 t ... 64 t + 63, one word (earliest bit
// lowest).  K = W + P - 1 is the span of a sync word and its payload less one: the frame that completes at bit g has
// its word at g - K ... g - P and its payload at g - P + 1 ... g.
//
// The ring.  HW = ceil(K / 64) words of history lie in front of a push's first tile, the LAST bit consumed so far in
// bit 63 of the last of them, zeros where the stream had not begun.  Numbering the words from the oldest history word
// (ring word 0), tile t is ring word HW + t, and the window of the frame that completes at bit l of tile t starts at
// ring bit 64 (HW + t) + l - K = 64 t + c + l with c = 64 HW - K in 0 ... 63: the same shift in every tile.  Ring word
// w lives in slot w & (RW - 1) of the wave's LDS, RW the power of two that holds HW words of history, the kChunk words
// of the tiles whose loads travel together, and one more; at most 256 words, 2 KiB.
// When a push ends behind m local bits the history is re-aligned: new history word j is the 64 ring bits from
// 64 j + m on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_framesync_math.h"
#include "hz_rowwave_plan.h"

namespace hz {
namespace fp {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count;

constexpr int kRealF32 = 32, kC64 = 1;  // HZSDR_SYMSYNC_REAL_F32, HZSDR_FMT_C64
constexpr uint32_t kMaxWord = 64, kMaxPayload = 8192, kMaxHyp = 4;
constexpr uint64_t kMaxHoldoff = 1ull << 31;
constexpr uint32_t kTileBits = 64;  // one tile: one wave-wide load, one ballot, one ring word
constexpr uint32_t kChunk = 16;     // tiles whose loads are in flight together, per wave
constexpr size_t kMaxPush = 0x7ffffff0u;  // symbols per row and push
constexpr int kFormComplex = 1, kFormDibit = 2, kFormDiff = 4;

struct Config {
    int kind;
    uint32_t B, W;
    uint64_t mask;
    uint32_t thr, H;
    uint64_t words[kMaxHyp];
    uint32_t maps[kMaxHyp];
    uint32_t P, diff;
    uint64_t holdoff;
};

// nullptr when the configuration makes a bank, else what is wrong with it (words and maps: H entries, not null)
inline const char *check_config(const Config &q) {
    if (q.kind != kRealF32 && q.kind != kC64) return "real float32 or complex64 rows";
    if (q.B != 1 && !(q.B == 2 && q.kind == kC64)) return "1 bit per symbol, or 2 on complex rows";
    if (q.W < q.B || q.W > kMaxWord || q.W % q.B) return "B <= W <= 64, W a multiple of B";
    if (q.P < q.B || q.P > kMaxPayload || q.P % q.B) return "B <= P <= 8192, P a multiple of B";
    if (q.H < 1 || q.H > kMaxHyp) return "1 ... 4 hypotheses";
    if (q.mask == 0 || (q.mask & ~fm::low_mask(q.W))) return "a mask of W bits, not zero";
    if (q.thr >= (uint32_t)__builtin_popcountll(q.mask)) return "thr < popcount(mask)";
    if (q.diff > 2 || (q.diff && q.B != 1)) return "diff is 0, 1 or 2, and 0 with B = 2";
    if (q.holdoff < 1 || q.holdoff > kMaxHoldoff) return "1 <= holdoff <= 2^31";
    for (uint32_t h = 0; h < q.H; h++) {
        if (q.words[h] & ~fm::low_mask(q.W)) return "a sync word of W bits";
        if (q.maps[h] >= (q.B == 2 ? 4u : 2u)) return "maps: 0 or 1 (B = 1), 0 ... 3 (B = 2)";
    }
    return nullptr;
}

struct Geom {
    uint32_t G, waves;  // rows per wave (the last wave may own fewer), waves: hz_rowwave_plan.h
    uint32_t K;         // W + P - 1: the history's bits
    uint32_t HW;        // the history's words: ceil(K / 64)
    uint32_t RW;        // the ring's words, a power of two
    uint32_t c;         // 64 HW - K: the shift of the window that completes at a tile's bit 0
    uint32_t FB;        // a frame's bytes: ceil(P / 8)
    uint32_t PW;        // a payload's words: ceil(P / 64)
    uint32_t per;       // a row's state on the device, in uint64 words: bits, hold, last, HW of history
    size_t lds_bytes;
};

constexpr uint32_t kStBits = 0, kStHold = 1, kStLast = 2, kStHist = 3;

// rows: 1 ... kMaxRows; a checked W and P
inline Geom geom(uint32_t rows, uint32_t W, uint32_t P) {
    Geom g{};
    // One row per wave at every R.  Dealt as the row-wave banks deal theirs (1024 waves before a wave takes a second
    // row, 8 rows per wave at 8192) the stage measured 5.3 times the device copy of its input at R = 8192: a wave spends
    // some 900 cycles on a tile, in the search's arithmetic and the ring's reads, and with ONE wave on a SIMD nothing
    // fills the gaps between its dependent instructions.  Nothing here is sequential along the rows of a wave, so
    // 8192 rows are 8192 waves and the SIMDs interleave as many of them as the registers allow.
    g.G = 1, g.waves = rows;
    g.K = W + P - 1;
    g.HW = (g.K + 63) / 64;
    g.RW = 1;
    while (g.RW < g.HW + kChunk + 1) g.RW *= 2;
    g.c = 64 * g.HW - g.K;
    g.FB = (P + 7) / 8;
    g.PW = (P + 63) / 64;
    g.per = kStHist + g.HW;
    g.lds_bytes = (size_t)g.RW * 8;
    return g;
}

// ---- where things lie in the ring (ring bits: 64 * ring word + bit) ----
// tile t (of the push) is ring word HW + t
HZ_HD uint32_t tile_word(uint32_t t, uint32_t HW) { return HW + t; }
HZ_HD uint32_t ring_slot(uint32_t word, uint32_t RW) { return word & (RW - 1); }
// the first ring bit of the window of the frame that completes at bit l of tile t; its payload starts W bits on
HZ_HD uint64_t window_bit(uint32_t t, uint32_t l, uint32_t c) { return (uint64_t)t * 64 + c + l; }

// ---- the history as the ABI moves it: K bits, oldest first, bit k in byte k / 8, bit 7 - k % 8 ----
inline size_t history_bytes(uint32_t K) { return (K + 7) / 8; }
inline void history_to_bytes(const uint64_t *words, const Geom &g, uint8_t *bytes) {
    for (size_t b = 0; b < history_bytes(g.K); b++) bytes[b] = 0;
    for (uint32_t k = 0; k < g.K; k++) {
        const uint32_t at = g.c + k;
        if ((words[at >> 6] >> (at & 63)) & 1ull) bytes[k >> 3] |= (uint8_t)(0x80u >> (k & 7));
    }
}
inline void history_from_bytes(const uint8_t *bytes, const Geom &g, uint64_t *words) {
    for (uint32_t w = 0; w < g.HW; w++) words[w] = 0;
    for (uint32_t k = 0; k < g.K; k++) {
        const uint32_t at = g.c + k;
        if (bytes[k >> 3] & (0x80u >> (k & 7))) words[at >> 6] |= 1ull << (at & 63);
    }
}

}  // namespace fp
}  // namespace hz
