// hz_equalizer_plan.h -- the host arithmetic of the equalizer bank (include/hzsdr_equalizer.h), HIP-free so that
// tests/host/equalizer_plan.cpp can run it under the sanitizers: how rows and taps are dealt to lanes and waves, the
// wave's LDS and its address maps (the kernel uses the same functions; the host program counts bank conflicts from
// them), the state's layout and the validation of the geometry and of a parameter set.
//
// Lane = tap.  A row takes Np consecutive lanes, Np = N rounded up to a power of two; a wave (a workgroup of its own,
// 64 lanes) owns G = min(8, 64 / Np, ceil(R / 1024)) consecutive rows for the whole push: as with the row-wave banks
// (hz_rowwave_plan.h) the rows are spread over as many waves as the chip has SIMDs before a wave takes a second row.
// Lane l of the wave is tap l % Np of the wave's row l / Np; lanes from G Np up idle.
//
// The LDS of a wave, in floats:
//   the segments   per plane (re, im) and row S floats: [N - 1 history | T = 256 symbols].  Slot s of a row's segment
//                  holds the input N - 1 - s symbols BEFORE the tile's first, so that tap i reads X[i] of the tile's
//                  symbol t at slot N - 1 + t - i: the row's lanes read consecutive floats.  S is the need rounded up
//                  to S % 64 == Np % 64: row r's lanes then fall on the banks r Np ... r Np + Np - 1 (mod 32, as a
//                  4-byte read is banked by groups of 32 lanes), which differ from row to row.  Taps from N up (the
//                  lanes that fill Np) read tap N - 1's slot: a broadcast, not a conflict.
//   the outputs    per plane and row T + 1 floats, then per row T + 1 floats of track: written by the row's first lane
//                  at slot t (the rows' banks differ by the odd pitch), read with lane = symbol.
//   the scratch    planes * 64 floats for the lane exchange that goes through the LDS (hz_equalizer.hip).
// At most 4 (2 * 8 * 264 + 3 * 8 * 257 + 128) = 41 KiB, under the family's 66 KiB.
//
// The state of a row, as get_state / set_state move it: the taps w[0 ... N - 1], then the N - 1 latest inputs, newest
// first; complex entries are (re, im) pairs: (2 N - 1) planes floats.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hz_rowwave_plan.h"
#include "hz_equalizer_math.h"

namespace hz {
namespace ep {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kSteps, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count;

constexpr uint32_t kParams = 2;  // mu, level
constexpr uint32_t kMaxTaps = 64;
constexpr int kRealF32 = 32, kC64 = 1;  // HZSDR_EQUALIZER_REAL_F32, HZSDR_FMT_C64
constexpr float kLow = 0x1p-64f, kHigh = 0x1p64f;
constexpr uint32_t kTile = kLanes * kSteps;  // T
constexpr uint32_t kOutPitch = kTile + 1;

struct Geom {
    uint32_t N, Np, c;  // taps, lanes per row, the centre tap
    uint32_t G;         // rows per wave (the last wave may own fewer)
    uint32_t waves;     // ceil(R / G)
    uint32_t K, T;      // symbols of a row per lane and tile; symbols per tile
    uint32_t S;         // floats of a row's segment
    uint32_t planes;    // 1: real rows, 2: complex rows
    uint32_t out_base;  // floats in front of the output tiles
    uint32_t xchg_base; // floats in front of the exchange's scratch: planes * 64 floats (HZ_EQ_EXCHANGE == 2 alone uses it)
    size_t lds_bytes;
};

inline uint32_t pow2_up(uint32_t n) {
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// nullptr when (taps, centre, mode, kind) make a bank, else what is wrong with them
inline const char *check_geom(long long taps, long long centre, int mode, bool complex_rows) {
    if (taps < 1 || taps > (long long)kMaxTaps) return "1 ... 64 taps";
    if (centre < 0 || centre >= taps) return "0 <= centre < taps";
    if (mode != em::kCma && mode != em::kDdBpsk && mode != em::kDdQpsk) return "the mode is CMA, DD_BPSK or DD_QPSK";
    if (mode == em::kDdQpsk && !complex_rows) return "DD_QPSK is for complex rows";
    return nullptr;
}

// rows: 1 ... kMaxRows; taps, centre: as check_geom accepts them
inline Geom equalizer_geom(uint32_t rows, uint32_t taps, uint32_t centre, bool complex_rows) {
    Geom g{};
    g.N = taps, g.Np = pow2_up(taps), g.c = centre;
    g.G = (rows + kWaves - 1) / kWaves;
    if (g.G > kLanes / g.Np) g.G = kLanes / g.Np;
    if (g.G > kMaxGroup) g.G = kMaxGroup;
    if (g.G < 1) g.G = 1;
    g.waves = (rows + g.G - 1) / g.G;
    g.K = kSteps, g.T = kTile;
    const uint32_t need = taps - 1 + g.T;
    g.S = need + (g.Np % kLanes + kLanes - need % kLanes) % kLanes;
    g.planes = complex_rows ? 2u : 1u;
    g.out_base = g.planes * g.G * g.S;
    g.xchg_base = g.out_base + (g.planes + 1) * g.G * kOutPitch;
    g.lds_bytes = (size_t)(g.xchg_base + g.planes * kLanes) * 4;
    return g;
}

// ---- the address maps, in floats from the start of the wave's LDS ----
// what a lane is to its wave
HZ_HD uint32_t lane_row(uint32_t lane, uint32_t Np) { return lane / Np; }
HZ_HD uint32_t lane_tap(uint32_t lane, uint32_t Np) { return lane % Np; }
// slot s of row r's segment, plane p
HZ_HD uint32_t seg_slot(uint32_t r, uint32_t p, uint32_t s, uint32_t G, uint32_t S) { return (p * G + r) * S + s; }
// the walk: X[tap] of the tile's symbol t (taps from N up read tap N - 1's)
HZ_HD uint32_t walk_slot(uint32_t tap, uint32_t t, uint32_t N) { return N - 1 + t - (tap < N ? tap : N - 1); }
// the loader: lane l, step k of K
HZ_HD uint32_t load_slot(uint32_t lane, uint32_t k, uint32_t N) { return N - 1 + lane + kLanes * k; }
// entry j of the history (X[j + 1] of the next symbol) in front of a tile
HZ_HD uint32_t history_slot(uint32_t j, uint32_t N) { return N - 2 - j; }
// the outputs: plane p (planes: the track) of row r, symbol t
HZ_HD uint32_t out_slot(uint32_t r, uint32_t p, uint32_t t, uint32_t G, uint32_t out_base) { return out_base + (p * G + r) * kOutPitch + t; }

// ---- the state ----
HZ_HD uint32_t state_row_floats(uint32_t N, uint32_t planes) { return (2 * N - 1) * planes; }
HZ_HD uint32_t state_tap(uint32_t i, uint32_t p, uint32_t planes) { return i * planes + p; }
HZ_HD uint32_t state_history(uint32_t j, uint32_t p, uint32_t N, uint32_t planes) { return (N + j) * planes + p; }
inline size_t state_floats(size_t rows, uint32_t N, uint32_t planes) { return rows * state_row_floats(N, planes); }

// nullptr when the two values make a set, else what is wrong with them
inline const char *check_params(const float *q) {
    if (!isfinite(q[0]) || !isfinite(q[1])) return "a parameter is not finite";
    if (!(q[0] >= 0.0f && q[0] <= 1.0f)) return "0 <= mu <= 1";
    if (!(q[1] >= kLow && q[1] <= kHigh)) return "2^-64 <= level <= 2^64";
    return nullptr;
}
inline em::Loop derive(const float *q) { return em::Loop{q[0], q[1]}; }

}  // namespace ep
}  // namespace hz
