// hz_demod_plan.h -- the host arithmetic of the demodulator bank (include/hzsdr_demod.h), HIP-free so that
// tests/host/demod_plan.cpp can run it under the sanitizers.  Everything that can overflow lives here.
//
// The stream position is kept as RUNNING values: the samples consumed N, the next output m = ceil(N / D), and
// rel = m D - N, the next output's own sample counted from the next push's first one, in [0, D).  Nothing is ever
// recomputed as a product with the stream length.
//
// The device sees a 64-bit scalar per workgroup, formed from the tile index (demod_tile), and 32-bit per-lane window
// indices below (T - 1) D + Q < 2^17, divided by D with a reciprocal (div_by_magic, hz_plan.h) that is exact on that range.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace dp {

constexpr uint32_t kMaxDown = 64, kMaxTaps = 1024, kMaxStreams = 8192;
constexpr int kThreads = 256;
// The LDS budget of a workgroup, hz_resampler_plan.h's: below 66 KiB, so that at least two workgroups are resident on a
// CU's 160 KiB.  The window holds one float per detector value; the taps are not in LDS (wave-uniform scalars).
constexpr uint32_t kWindowMax = 16896;  // floats of the tile's window, its layout's padding included
// a push's outputs times D stay below this (the tile base is a 64-bit product of the tile index)
constexpr uint64_t kSpanMax = (uint64_t)1 << 62;

struct State {
    uint64_t n = 0, m = 0;  // samples consumed, index of the next output
    uint32_t rel = 0;       // m D - n
};

struct Step {
    bool ok;         // false: the push is too long for 64-bit counts (nothing else is valid then)
    uint64_t count;  // outputs the push writes
    State next;
    size_t held;     // samples of the stream the held tail carries afterwards: min(N, Q), zeros in front of them
};

// what a push of n_in samples does to the state
inline Step demod_step(const State &s, uint32_t D, uint32_t Q, uint64_t n_in) {
    Step r{false, 0, s, 0};
    const uint64_t count = n_in > s.rel ? (n_in - s.rel - 1) / D + 1 : 0;  // outputs k with rel + k D < n_in
    if (count > (kSpanMax - 1) / D || s.n + n_in < s.n || s.m + count < s.m) return r;  // (count D >= kSpanMax)
    r.ok = true;
    r.count = count;
    r.next.n = s.n + n_in;
    r.next.m = s.m + count;
    r.next.rel = (uint32_t)(s.rel + count * D - n_in);  // below D again
    r.held = r.next.n < Q ? (size_t)r.next.n : Q;
    return r;
}

// the outputs a flush writes: m with ceil(N / D) <= m and m D <= N + Q - 2, i.e. k with rel + k D <= Q - 2
inline uint64_t demod_flush_count(const State &s, uint32_t D, uint32_t Q) {
    if (s.n == 0 || Q < 2 + s.rel) return 0;
    return (Q - 2 - s.rel) / D + 1;
}

struct Tile {
    uint64_t i0;      // the own sample of the tile's first output, relative to the push's first sample
    uint32_t window;  // detector values the tile's outputs read: relative indices [i0 - (Q - 1), i0 - (Q - 1) + window)
};

// tile `tile` of a push whose first output has `rel`: T outputs from output tile * T of the push
HZ_HD Tile demod_tile(uint32_t rel, uint32_t D, uint32_t Q, uint32_t T, uint64_t tile) {
    Tile t;
    t.i0 = rel + tile * ((uint64_t)T * D);  // below 2^63: Step.ok
    t.window = (T - 1) * D + Q;
    return t;
}

// floor(w / D) for w < 2^22 is div_by_magic(w, div_magic(D)) (hz_plan.h): D <= 64 and w < 2^22 keep w D below 2^32.
constexpr uint32_t kDivRange = 1u << 22;

// Where window value w lives in LDS.  For a given tap, lane l of a wave reads value l D + c: 4 bytes each, serviced 32
// lanes at a time over 32 banks.  The window is stored TRANSPOSED, D rows of J floats, value w in row w mod D at
// column floor(w / D): the lanes of one read then sit in ONE row at consecutive columns, one lane per bank for every
// D, odd or even, and every c.  Along the taps the slot is stepped, never divided: from w to w - 1 it goes one row up
// (slot - J), and from row 0 to row D - 1 of the column before (slot + (D - 1) J - 1); the row is c mod D, the same for
// every lane and every chain, so the stepping is scalar work common to a wave.  The slot is transposed_slot(w, D, J)
// (hz_plan.h).

// the kernel's shape for (D, Q), chosen once at create
struct Geom {
    uint32_t T;        // outputs per workgroup
    bool half;         // T = kThreads / 2: the upper half of the lanes fills the window and owns no output
    uint32_t window;   // detector values of a tile: (T - 1) D + Q
    uint32_t J;        // columns of the transposed window: ceil(window / D), made odd
    uint32_t row0, slot0;  // of the newest value of output 0 of the tile, w = Q - 1: its row and its slot
    size_t lds_bytes;
};

// The largest T of 4, 2, 1 chains per lane whose window fits the budget.  255 D + Q alone passes it at D = 64 with
// Q > 512 (and at D = 63 with Q > 756): there a workgroup takes kThreads / 2 outputs, at most 127 * 64 + 1024 values.
inline Geom demod_geom(uint32_t D, uint32_t Q) {
    Geom g{};
    for (uint32_t T : {4u * kThreads, 2u * kThreads, 1u * kThreads, kThreads / 2u}) {
        g.T = T;
        g.window = (T - 1) * D + Q;
        g.J = ((g.window + D - 1) / D) | 1u;
        if (D * g.J <= kWindowMax) break;
    }
    g.half = g.T < (uint32_t)kThreads;
    g.row0 = (Q - 1) % D;
    g.slot0 = transposed_slot(Q - 1, D, g.J);
    g.lds_bytes = (size_t)D * g.J * 4;
    return g;
}

}  // namespace dp
}  // namespace hz
