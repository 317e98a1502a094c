// hz_tuner_plan.h -- the host arithmetic of the tuner bank (include/hzsdr_tuner.h), HIP-free so that
// tests/host/tuner_plan.cpp can run it under the sanitizers.  Everything that can overflow lives here.
//
// The stream position is hz_demod_plan.h's: the samples consumed N, the next output m = ceil(N / D) and
// rel = m D - N as running values (dp::State, dp::demod_step, dp::demod_flush_count hold for every D below 2^32).
// Beside it one running uint32 per tuner: the phase word (w D m) mod 2^32 of the next push's first output, advanced
// by step * count in wrapping arithmetic and never formed as a product with the stream length.
//
// The product is A (2K x 2Qp) times B (2Qp x outputs) on v_mfma_f32_16x16x4_f32.  A workgroup of four waves takes T
// outputs times `tile_rows` rows of A; a wave holds 2 x 2 accumulators of 16 x 16, i.e. 32 rows times 32 outputs, and
// the waves lie along the outputs first (T = 128: 4 x 1, T = 64: 2 x 2, T = 32: 1 x 4).  The tile's window of
// (T - 1) D + cq converted samples is staged in LDS as two planes (re, im), each transposed by D (transposed_slot, hz_plan.h); cq is
// the chunk of q staged at once, Qp wherever the window then fits the budget, otherwise the largest even count that
// does at T = 32, the accumulators carried from chunk to chunk.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_demod_plan.h"

namespace hz {
namespace tp {

constexpr uint32_t kMaxTuners = 256, kMaxDown = 256, kMaxTaps = 1024;
constexpr int kThreads = 256;
// The LDS budget of a workgroup, hz_resampler_plan.h's and hz_demod_plan.h's: 66 KiB, in floats.
constexpr uint32_t kLdsFloats = 16896;
constexpr uint32_t kWaveRows = 32, kWaveOutputs = 32;  // a wave's register tile: 2 x 2 accumulators of 16 x 16

using State = dp::State;
using Step = dp::Step;

// samples of the stream the object holds between pushes: the last Q - 1
inline uint32_t tuner_held(uint32_t Q) { return Q - 1; }

// ---- the running phase words -------------------------------------------------------------------------
// the phase step from one output to the next, (w D) mod 2^32
HZ_HD uint32_t phase_step(uint32_t w, uint32_t D) { return w * D; }
// the word of output m, (w D m) mod 2^32 = step * (m mod 2^32) mod 2^32: at create, reset and retune
inline uint32_t phase_at(uint32_t step, uint64_t m) { return step * (uint32_t)m; }
// behind a push of `count` outputs
HZ_HD uint32_t phase_advance(uint32_t p, uint32_t step, uint64_t count) { return p + step * (uint32_t)count; }

// ---- the window's layout ------------------------------------------------------------------------------
// floor(w / D) for w < 2^16 is div_by_magic(w, div_magic(D)) (hz_plan.h): D <= 256 and w < 2^16 keep w D below 2^32.
constexpr uint32_t kDivRange = 1u << 16;

// Where window sample w lives in a plane.  Lane l of a B-operand read holds output (l & 15) of a 16-column tile: the
// 16 lanes of one k are samples D apart.  Stored transposed, D rows of J floats, sample w in row w mod D at column
// floor(w / D), they are 16 consecutive floats for every D.  The two halves of a 32-lane service group read the SAME
// slots of the re plane and of the im plane (k = 0, 1: the re and im term of one q), so the plane pitch is 16 modulo
// 32: distinct banks for every D.  The slot is transposed_slot(w, D, J) (hz_plan.h).
inline uint32_t tuner_plane(uint32_t D, uint32_t J) {
    const uint32_t p = D * J;
    return p + (48u - p % 32u) % 32u;
}

struct Geom {
    uint32_t T;          // outputs per workgroup: 128, 64 or 32
    uint32_t tile_rows;  // rows of A per workgroup: 32, 64 or 128 (two per tuner)
    uint32_t waves_out;  // waves along the outputs: T / 32
    uint32_t Qp, steps;  // Q rounded up to even; the k-steps of the whole sum, Qp / 2
    uint32_t cq, chunks; // q per staged chunk (even), and the chunks: ceil(Qp / cq)
    uint32_t window;     // samples staged per chunk: (T - 1) D + cq
    uint32_t J, plane;   // columns of a transposed plane; floats from the re plane to the im plane
    uint32_t row_tiles;  // 16-row tiles of A in device memory: 2K rounded up to whole wave tiles
    size_t lds_bytes, a_floats;
};

// J for a window of `window` samples: odd where that still fits (the staging stores of consecutive samples then fall
// on distinct banks), as it is otherwise; 0: the window does not fit the budget
inline uint32_t tuner_columns(uint32_t D, uint32_t window) {
    const uint32_t j = (window + D - 1) / D;
    if (2 * (uint64_t)tuner_plane(D, j | 1u) <= kLdsFloats) return j | 1u;
    if (2 * (uint64_t)tuner_plane(D, j) <= kLdsFloats) return j;
    return 0;
}

inline Geom tuner_geom(uint32_t K, uint32_t D, uint32_t Q) {
    Geom g{};
    g.Qp = (Q + 1) & ~1u;
    g.steps = g.Qp / 2;
    g.cq = g.Qp;
    for (uint32_t T : {128u, 64u, 32u}) {
        g.T = T;
        g.J = tuner_columns(D, (T - 1) * D + g.Qp);
        if (g.J) break;
    }
    // (31 D + 2 <= 7938 samples fit for every D <= 256: the search ends)
    while (!g.J) {
        g.cq -= 2;
        g.J = tuner_columns(D, (g.T - 1) * D + g.cq);
    }
    g.chunks = (g.Qp + g.cq - 1) / g.cq;
    g.window = (g.T - 1) * D + g.cq;
    g.plane = tuner_plane(D, g.J);
    g.waves_out = g.T / kWaveOutputs;
    g.tile_rows = (kThreads / 64 / g.waves_out) * kWaveRows;
    g.row_tiles = (2 * K + kWaveRows - 1) / kWaveRows * (kWaveRows / 16);
    g.lds_bytes = (size_t)2 * g.plane * 4;
    g.a_floats = (size_t)g.row_tiles * g.steps * 64;
    return g;
}

// ---- A in MFMA operand order ---------------------------------------------------------------------------
// Element (row, j) of A, j = 2 q + c the inner index (c = 0: the factor of a.re, c = 1: of a.im).  Lane l of
// v_mfma_f32_16x16x4_f32 holds A[l & 15][l >> 4] of a 16 x 4 block: for each 16-row tile and each k-step the 64 lanes'
// values are contiguous.
HZ_HD size_t tuner_a_index(uint32_t row, uint32_t j, uint32_t steps) {
    return ((size_t)(row / 16) * steps + j / 4) * 64 + (j % 4) * 16 + row % 16;
}

// tile `tile` of a push whose first output has `rel`, chunk `chunk`: the relative index (from the push's first sample)
// of window sample 0, which is the sample of the tile's first output at the chunk's LAST q, qa + cq - 1
HZ_HD int64_t tuner_window_base(uint32_t rel, uint32_t D, uint32_t T, uint32_t cq, uint64_t tile, uint32_t chunk) {
    return (int64_t)(rel + tile * ((uint64_t)T * D)) - (int64_t)((uint64_t)chunk * cq + cq - 1);  // below 2^63: Step.ok
}

}  // namespace tp
}  // namespace hz
