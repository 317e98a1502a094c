// hz_bitring_plan.h -- the host arithmetic that the bit-ring banks share (the frame sync bank, hz_framesync_plan.h; the
// HDLC deframer bank, hz_hdlc_plan.h), HIP-free so that tests/host/bitring_plan.cpp can run it under the sanitizers: how
// the rows are dealt to waves, the tiles, the history ring and its slots, the history as the ABI moves it.  The device
// side of the shape is hz_bitring.h, the host side of the banks' objects hz_framebank.h.  A bit-ring kernel is NOT a
// row-wave kernel: a wave owns a row, but lane = float.
//
// Bits.  A row's bit stream is numbered from 0 at create or reset.  A push numbers the bits it consumes 0 ... m - 1
// (LOCAL bits); a tile is 64 consecutive local bits, tile t the bits 64 t ... 64 t + 63, one word (earliest bit
// lowest).  K is what a bank has to look back over from the bit that completes one of its objects: the history's bits.
//
// The ring.  HW = ceil(K / 64) words of history lie in front of a push's first tile, the LAST bit consumed so far in
// bit 63 of the last of them, zeros where the stream had not begun: the history's oldest bit is bit c = 64 HW - K, in
// 0 ... 63, of its first word.  Numbering the words from the oldest history word (ring word 0), tile t is ring word
// HW + t and local bit i is ring bit 64 HW + i.  Ring word w lives in slot w & (RW - 1) of the wave's LDS, RW the power
// of two that holds HW words of history, the kChunk words of the tiles whose loads travel together, and one more; at
// most 256 words, 2 KiB.  When a push ends behind m local bits the history is re-aligned: new history word j is the 64
// ring bits from 64 j + m on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_rowwave_plan.h"

namespace hz {
namespace br {

using rw::kMaxRows, rw::kLanes, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count;

constexpr int kRealF32 = 32, kC64 = 1;    // HZSDR_SYMSYNC_REAL_F32, HZSDR_FMT_C64
constexpr uint32_t kTileBits = 64;        // one tile: one wave-wide load, one ballot, one ring word
constexpr uint32_t kChunk = 16;           // tiles whose loads are in flight together, per wave
constexpr size_t kMaxPush = 0x7ffffff0u;  // symbols per row and push

struct Deal {
    uint32_t G, waves;  // rows per wave (the last wave may own fewer), waves: hz_rowwave_plan.h
};

// rows: 1 ... kMaxRows
inline Deal deal(uint32_t rows) {
    // One row per wave at every R.  Dealt as the row-wave banks deal theirs (1024 waves before a wave takes a second
    // row, 8 rows per wave at 8192) the frame sync stage measured 5.3 times the device copy of its input at R = 8192: a
    // wave spends some 900 cycles on a tile, in the search's arithmetic and the ring's reads, and with ONE wave on a SIMD
    // nothing fills the gaps between its dependent instructions.  Nothing here is sequential along the rows of a wave, so
    // 8192 rows are 8192 waves and the SIMDs interleave as many of them as the registers allow.
    return Deal{1, rows};
}

struct Ring {
    uint32_t K;   // the history's bits
    uint32_t HW;  // the history's words: ceil(K / 64)
    uint32_t RW;  // the ring's words, a power of two
    uint32_t c;   // 64 HW - K: where the history's oldest bit lies in its first word
};

// K: 1 ... 64 (256 - kChunk - 1)
inline Ring ring(uint32_t K) {
    Ring g{};
    g.K = K;
    g.HW = (K + 63) / 64;
    g.RW = 1;
    while (g.RW < g.HW + kChunk + 1) g.RW *= 2;
    g.c = 64 * g.HW - K;
    return g;
}

// ---- where things lie in the ring (ring bits: 64 * ring word + bit) ----
// tile t (of the push) is ring word HW + t
HZ_HD uint32_t tile_word(uint32_t t, uint32_t HW) { return HW + t; }
HZ_HD uint32_t ring_slot(uint32_t word, uint32_t RW) { return word & (RW - 1); }

// ---- the history as the ABI moves it: K bits, oldest first, bit k in byte k / 8, bit 7 - k % 8 ----
inline size_t history_bytes(uint32_t K) { return (K + 7) / 8; }
inline void history_to_bytes(const uint64_t *words, const Ring &g, uint8_t *bytes) {
    for (size_t b = 0; b < history_bytes(g.K); b++) bytes[b] = 0;
    for (uint32_t k = 0; k < g.K; k++) {
        const uint32_t at = g.c + k;
        if ((words[at >> 6] >> (at & 63)) & 1ull) bytes[k >> 3] |= (uint8_t)(0x80u >> (k & 7));
    }
}
inline void history_from_bytes(const uint8_t *bytes, const Ring &g, uint64_t *words) {
    for (uint32_t w = 0; w < g.HW; w++) words[w] = 0;
    for (uint32_t k = 0; k < g.K; k++) {
        const uint32_t at = g.c + k;
        if (bytes[k >> 3] & (0x80u >> (k & 7))) words[at >> 6] |= 1ull << (at & 63);
    }
}

}  // namespace br
}  // namespace hz
