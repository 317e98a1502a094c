// hz_hdlc_plan.h -- the host arithmetic of the HDLC deframer bank (include/hzsdr_hdlc.h), HIP-free so that
// tests/host/hdlc_plan.cpp can run it under the sanitizers: the validation of a bank's configuration, where an event's
// window and a span lie in the history ring, the table of the FCS combine, the state's layout on the device.  The bits,
// the ring, the dealing of rows to waves and the history as the ABI moves it are the bit-ring banks': hz_bitring_plan.h.
//
// An event is kept as its END, the position of its last bit plus one: the abort at -1 that a row starts with has end 0,
// and for a flag the end is the first bit of the span behind it -- what `positions` reports.  For two flags of ends
// E1 < E2 the raw span is the L = E2 - E1 - 8 bits from E1 on (none when E2 - E1 <= 8).  Lmax = 8 max_bytes +
// floor(8 max_bytes / 5) is the longest span that can be well-formed, K = Lmax + 8 the history's bits: a span and its
// closing flag.  The window b[i-7 ... i] of local bit i starts at ring bit 64 HW + i - 7; the span that the flag of end
// E2 at local bit i closes starts at ring bit 64 HW + i + 1 - (E2 - E1), which is not negative while L <= Lmax.  Behind
// the ring lie OW = ceil(max_bytes / 8) + 1 words in which a frame's unstuffed bits are put together, and behind them the
// FCS's byte table, 256 words of 32 bits.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_bitring_plan.h"
#include "hz_framesync_math.h"
#include "hz_hdlc_math.h"

namespace hz {
namespace hp {

using br::kMaxRows, br::kLanes, br::kTileBits, br::kChunk, br::kMaxPush, br::kRealF32, br::kC64;
using br::wave_first_row, br::wave_row_count, br::ring_slot, br::tile_word;
using br::history_bytes, br::history_to_bytes, br::history_from_bytes;

constexpr uint32_t kMaxBytes = 1024;
constexpr uint32_t kMaxPass = 3;  // a span's words over the 64 lanes: ceil(154 / 64) passes at most
// The FCS of a frame of up to kWalkBytes bytes is walked byte by byte through a table in LDS; a longer frame's is
// combined from per-word registers (hz_hdlc.hip).  Measured, 1024 rows of traffic, per frame and wave: the walk 2.5 us
// at 32 bytes and 80 us at 1024, the combine 4.1 us and 6 us: they cross near 50 bytes.
// (A/B builds: make EXTRA=-DHZ_HDLC_WALK_BYTES=0 combines every frame, =1024 walks every frame.)
#ifndef HZ_HDLC_WALK_BYTES
#define HZ_HDLC_WALK_BYTES 48
#endif
constexpr uint32_t kWalkBytes = HZ_HDLC_WALK_BYTES, kTableBytes = 256 * 4;
constexpr int kFormComplex = 1, kFormDiff = 4, kFormFcs16 = 8, kFormFcs32 = 16, kFormMsbFirst = 32, kFormKeepBad = 64;
constexpr uint32_t kEvAbort = 0, kEvFlag = 1;

struct Config {
    int kind;
    uint32_t diff, fcs, min_bytes, max_bytes, msb_first, keep_bad;
};

// nullptr when the configuration makes a bank, else what is wrong with it
inline const char *check_config(const Config &q) {
    if (q.kind != kRealF32 && q.kind != kC64) return "real float32 or complex64 rows";
    if (q.diff > 2) return "diff is 0, 1 or 2";
    if (q.fcs != 0 && q.fcs != 16 && q.fcs != 32) return "fcs is 0, 16 or 32";
    if (q.min_bytes < 1 || q.min_bytes > q.max_bytes || q.max_bytes > kMaxBytes) return "1 <= min_bytes <= max_bytes <= 1024";
    if (q.min_bytes <= q.fcs / 8) return "min_bytes is above the FCS's bytes";
    if (q.msb_first > 1 || q.keep_bad > 1) return "msb_first and keep_bad are 0 or 1";
    return nullptr;
}

inline uint32_t span_max(uint32_t max_bytes) { return 8 * max_bytes + 8 * max_bytes / 5; }

// the ring's K is Lmax + 8
struct Geom : br::Ring, br::Deal {
    uint32_t Lmax;  // the longest raw span that can be well-formed
    uint32_t OW;    // the words in which a frame is put together
    uint32_t per;   // a row's state on the device, in uint64 words: bits, event end, event kind, last, HW of history
    size_t lds_bytes;
};

constexpr uint32_t kStBits = 0, kStEvEnd = 1, kStEvKind = 2, kStLast = 3, kStHist = 4;

// rows: 1 ... kMaxRows; a checked max_bytes
inline Geom geom(uint32_t rows, uint32_t max_bytes) {
    Geom g{br::ring(span_max(max_bytes) + 8), br::deal(rows)};
    g.Lmax = span_max(max_bytes);
    g.OW = (max_bytes + 7) / 8 + 1;
    g.per = kStHist + g.HW;
    g.lds_bytes = (size_t)(g.RW + g.OW) * 8 + kTableBytes;
    return g;
}

// ---- where things lie in the ring (ring bits: 64 * ring word + bit) ----
// the first ring bit of the window b[i-7 ... i] of bit l of tile t
HZ_HD uint64_t window_bit(uint32_t t, uint32_t l, uint32_t HW) { return ((uint64_t)HW + t) * 64 + l - 7; }
// the first ring bit of the span that the flag at bit l of tile t closes; d = E2 - E1, 8 < d <= K
HZ_HD uint64_t span_bit(uint32_t t, uint32_t l, uint32_t HW, uint32_t d) { return ((uint64_t)HW + t) * 64 + l + 1 - d; }
// a raw span of L bits can hold a well-formed frame
HZ_HD bool span_fits(uint64_t L, uint32_t min_bytes, uint32_t Lmax) { return L >= 8ull * min_bytes && L <= Lmax; }
HZ_HD bool well_formed(uint32_t u, uint32_t min_bytes, uint32_t max_bytes) { return u % 8 == 0 && u / 8 >= min_bytes && u / 8 <= max_bytes; }

// ---- the FCS combine: tab[k] = x^(64 k) in the register's form, k = 0 ... kMaxBytes / 8 - 1 ----
constexpr uint32_t kPowers = kMaxBytes / 8;
inline void fcs_powers(uint32_t fcs, uint32_t *tab) {
    if (fcs == 0) {
        for (uint32_t k = 0; k < kPowers; k++) tab[k] = 0;
        return;
    }
    uint32_t a = 1u << (fcs - 1);
    for (uint32_t k = 0; k < kPowers; k++) {
        tab[k] = a;
        for (int s = 0; s < 64; s++) a = hm::fcs_next_power(a, hm::fcs_poly(fcs));
    }
}

}  // namespace hp
}  // namespace hz
