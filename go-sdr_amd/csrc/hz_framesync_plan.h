// hz_framesync_plan.h -- the host arithmetic of the frame sync bank (include/hzsdr_framesync.h), HIP-free so that
// tests/host/framesync_plan.cpp can run it under the sanitizers: the validation of a bank's configuration, where a
// window and a payload lie in the history ring, the state's layout on the device.  The bits, the ring, the dealing of
// rows to waves and the history as the ABI moves it are the bit-ring banks': hz_bitring_plan.h.
//
// K = W + P - 1 is the span of a sync word and its payload less one: the frame that completes at bit g has its word at
// g - K ... g - P and its payload at g - P + 1 ... g.  The window of the frame that completes at bit l of tile t starts
// at ring bit 64 (HW + t) + l - K = 64 t + c + l: the same shift c in every tile.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_bitring_plan.h"
#include "hz_framesync_math.h"

namespace hz {
namespace fp {

using br::kMaxRows, br::kLanes, br::kLdsBudget, br::kTileBits, br::kChunk, br::kMaxPush, br::kRealF32, br::kC64;
using br::wave_first_row, br::wave_row_count, br::ring_slot, br::tile_word;
using br::history_bytes, br::history_to_bytes, br::history_from_bytes;

constexpr uint32_t kMaxWord = 64, kMaxPayload = 8192, kMaxHyp = 4;
constexpr uint64_t kMaxHoldoff = 1ull << 31;
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

// the ring's K is W + P - 1, its c the shift of the window that completes at a tile's bit 0
struct Geom : br::Ring, br::Deal {
    uint32_t FB;   // a frame's bytes: ceil(P / 8)
    uint32_t PW;   // a payload's words: ceil(P / 64)
    uint32_t per;  // a row's state on the device, in uint64 words: bits, hold, last, HW of history
    size_t lds_bytes;
};

constexpr uint32_t kStBits = 0, kStHold = 1, kStLast = 2, kStHist = 3;

// rows: 1 ... kMaxRows; a checked W and P
inline Geom geom(uint32_t rows, uint32_t W, uint32_t P) {
    Geom g{br::ring(W + P - 1), br::deal(rows)};
    g.FB = (P + 7) / 8;
    g.PW = (P + 63) / 64;
    g.per = kStHist + g.HW;
    g.lds_bytes = (size_t)g.RW * 8;
    return g;
}

// ---- where things lie in the ring (ring bits: 64 * ring word + bit) ----
// the first ring bit of the window of the frame that completes at bit l of tile t; its payload starts W bits on
HZ_HD uint64_t window_bit(uint32_t t, uint32_t l, uint32_t c) { return (uint64_t)t * 64 + c + l; }

}  // namespace fp
}  // namespace hz
