// hz_rowwave_plan.h -- the host arithmetic that the row-wave banks share (the IIR bank, hz_iir_plan.h; the symbol-timing
// recovery bank, hz_symsync_plan.h; the carrier recovery bank, hz_carrier_plan.h; the AGC bank, hz_agc_plan.h), HIP-free
// so that tests/host/ can run it under the sanitizers: how the rows are dealt
// to waves, the sample tile, and the address maps of the tile that the kernels themselves use (a host program counts
// bank conflicts from the same functions).  The device side of the shape is hz_rowwave.h.
//
// One lane owns one row and walks time; a wave (a workgroup of its own, 64 lanes) owns `G` consecutive rows for the
// whole push.  A wave-instruction costs the SIMD the same whether 1 or 64 lanes are live, and the recursion is a chain
// of dependent steps that no second lane can shorten: the rows are therefore spread over as MANY waves as the chip has
// SIMDs (kWaves = 256 CUs x 4) before a wave takes a second row, G = ceil(R / kWaves), and 8192 rows come to 8 per wave.
//
// The tile: T consecutive samples of the wave's G rows, one float per (sample, row) and plane (re, im), stored
// TRANSPOSED -- sample t of row r at float t * P + r of its plane, P = G made odd.  The recursion reads and writes with
// t fixed and lane = row (consecutive floats); the loader writes and the storer reads with the row fixed and lane = t
// (floats P apart: P is odd, so the 32 lanes of a group of a 4-byte LDS access fall on 32 distinct banks).  Every access
// is 4 bytes wide: complex rows keep re and im in planes of their own, T * P floats apart.
//
// T = 64 K samples, lane l moving samples l + 64 k of a row: K instructions that together cover 64 K consecutive
// samples of the row, 512 bytes of the two-byte formats and more of the others.  K = 4, T = 256: the loads of a tile are
// issued one tile ahead, and the recursion over a tile must outlast the memory's latency for them to have arrived --
// measured with T = 64, a one-section tile (0.6 us of recursion) waited 1.6 us more for its samples.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace rw {

constexpr uint32_t kMaxRows = 8192, kLanes = 64;
constexpr uint32_t kWaves = 1024;   // the waves the rows are spread over before a wave takes a second row
constexpr uint32_t kMaxGroup = 8;   // rows per wave at most: kMaxRows / kWaves
static_assert(kMaxRows <= kWaves * kMaxGroup, "a wave's rows are unrolled kMaxGroup times");
constexpr uint32_t kSteps = 4;      // K: samples of a row per lane and tile
// the family's LDS budget per workgroup (hz_demod_plan.h, hz_resampler_plan.h): below 66 KiB
constexpr size_t kLdsBudget = 66 * 1024;

struct Geom {
    uint32_t G;       // rows per wave (the last wave may own fewer)
    uint32_t waves;   // ceil(R / G)
    uint32_t P;       // floats from one sample of the tile to the next: G made odd
    uint32_t K;       // samples of a row per lane and tile
    uint32_t T;       // samples per tile: 64 K
    uint32_t planes;  // 1: real rows, 2: complex rows (re, im)
};

// rows: 1 ... kMaxRows; complex_rows: two values per sample
inline Geom geom(uint32_t rows, bool complex_rows) {
    Geom g{};
    g.G = (rows + kWaves - 1) / kWaves;
    if (g.G < 1) g.G = 1;
    if (g.G > kMaxGroup) g.G = kMaxGroup;
    g.waves = (rows + g.G - 1) / g.G;
    g.P = g.G | 1u;
    g.K = kSteps;
    g.T = kLanes * g.K;
    g.planes = complex_rows ? 2u : 1u;
    return g;
}
inline uint32_t tile_floats(const Geom &g) { return g.planes * g.T * g.P; }

// the rows of wave w: [first, first + count)
HZ_HD uint32_t wave_first_row(uint32_t w, uint32_t G) { return w * G; }
HZ_HD uint32_t wave_row_count(uint32_t w, uint32_t G, uint32_t rows) {
    const uint32_t first = w * G;
    return first >= rows ? 0u : (rows - first < G ? rows - first : G);
}

// ---- the tile's address maps, in floats from the start of the wave's LDS ----
// sample t of row r (of the wave), plane p
HZ_HD uint32_t tile_slot(uint32_t t, uint32_t r, uint32_t p, uint32_t P, uint32_t T) { return p * T * P + t * P + r; }
// the loader and the storer: lane l, step k of K, row r
HZ_HD uint32_t move_slot(uint32_t lane, uint32_t k, uint32_t r, uint32_t p, uint32_t P, uint32_t T) {
    return tile_slot(lane + kLanes * k, r, p, P, T);
}
// the walk: lane l owns row l, at sample t
HZ_HD uint32_t walk_slot(uint32_t lane, uint32_t t, uint32_t p, uint32_t P, uint32_t T) { return tile_slot(t, lane, p, P, T); }

}  // namespace rw
}  // namespace hz
