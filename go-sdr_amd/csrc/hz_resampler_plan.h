// hz_resampler_plan.h -- the host arithmetic of the polyphase resampler (include/hzsdr_resampler.h), HIP-free so that
// tests/host/resampler_plan.cpp can run it under the sanitizers.  Everything that can overflow lives here.
//
// The stream position is kept as RUNNING values: the samples consumed N, the next output m, and beside them
// phi = (m D) mod U and rel = floor(m D / U) - N, the next output's newest sample counted from the next push's first
// one.  m D - N U = rel U + phi lies in [0, D + U): an output is written as soon as its newest sample has arrived
// (m D < N U), so rel >= 0, and the one before it was written, so rel U + phi < D + U.  A push updates them with
// 128-bit integers; nothing is ever recomputed as a product with the stream length.
//
// The device sees a 64-bit scalar per workgroup, formed from the tile index (resampler_tile), and 32-bit per-lane
// offsets below U + T D < 2^22, divided by U with a reciprocal (div_by_magic, hz_plan.h) that is exact on that range.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace rs {

constexpr uint32_t kMaxRate = 1024, kMaxTaps = 65536, kMaxPhaseTaps = 256, kMaxStreams = 8192;
constexpr int kThreads = 256;
// The LDS budget of a workgroup: window (its padding included) and table together stay below 66 KiB, so that at least
// two workgroups are resident on a CU's 160 KiB; a workgroup asks for what its shape needs, which is mostly far less.
constexpr uint32_t kWindowMax = 5120;  // samples of the tile's window (8 bytes each)
constexpr uint32_t kTableMax = 6144;   // floats of the polyphase table
// a push's outputs times D stay below this (the tile base is a 64-bit product of the tile index)
constexpr uint64_t kSpanMax = (uint64_t)1 << 62;

struct State {
    uint64_t n = 0, m = 0;      // samples consumed, index of the next output
    uint32_t phi = 0, rel = 0;  // (m D) mod U; floor(m D / U) - n
};

struct Step {
    bool ok;         // false: the push is too long for 64-bit counts (nothing else is valid then)
    uint64_t count;  // outputs the push writes
    State next;
    size_t held;     // samples of the stream the held tail carries afterwards: min(N, Q - 1), zeros in front of them
};

// what a push of n_in samples does to the state
inline Step resampler_step(const State &s, uint32_t U, uint32_t D, uint32_t Q, uint64_t n_in) {
    Step r{false, 0, s, 0};
    const unsigned __int128 span = (unsigned __int128)n_in * U;  // the push in units of 1/U sample
    const unsigned __int128 t = (unsigned __int128)s.rel * U + s.phi;
    unsigned __int128 count = span > t ? (span - t + D - 1) / D : 0;  // outputs k with t + k D < span
    if (count * D >= kSpanMax || s.n + n_in < s.n || s.m + (uint64_t)count < s.m) return r;
    const unsigned __int128 t2 = t + count * D - span;  // below D + U again
    r.ok = true;
    r.count = (uint64_t)count;
    r.next.n = s.n + n_in;
    r.next.m = s.m + r.count;
    r.next.rel = (uint32_t)(t2 / U);
    r.next.phi = (uint32_t)(t2 % U);
    r.held = r.next.n < Q - 1 ? (size_t)r.next.n : Q - 1;
    return r;
}

// the outputs a flush writes: m with M(N) <= m and m D <= (N - 1) U + L - 1, i.e. k with t + k D < L - U
inline uint64_t resampler_flush_count(const State &s, uint32_t U, uint32_t D, uint32_t L) {
    const uint64_t t = (uint64_t)s.rel * U + s.phi;
    if (s.n == 0 || (uint64_t)L <= U + t) return 0;
    return (L - U - t + D - 1) / D;
}

struct Tile {
    uint64_t i0;      // newest sample of the tile's first output, relative to the push's first sample
    uint32_t phi;     // phase of the tile's first output
    uint32_t window;  // samples the tile's outputs read: relative indices [i0 - (Q - 1), i0 - (Q - 1) + window)
};

// tile `tile` of a push whose first output has (rel, phi): T outputs from output tile * T of the push
HZ_HD Tile resampler_tile(uint32_t rel, uint32_t phi, uint32_t U, uint32_t D, uint32_t Q, uint32_t T, uint64_t tile) {
    const uint64_t tt = (uint64_t)rel * U + phi + tile * ((uint64_t)T * D);  // below 2^63: Step.ok
    Tile t;
    t.i0 = tt / U;
    t.phi = (uint32_t)(tt - t.i0 * U);
    t.window = (t.phi + (T - 1) * D) / U + Q;
    return t;
}

// floor(u / U) for u < 2^22 is div_by_magic(u, div_magic(U)) (hz_plan.h): U <= 1024 and u < 2^22 keep u U below 2^32.
constexpr uint32_t kDivRange = 1u << 22;

// the kernel's shape for (U, D, Q), chosen once at create
struct Geom {
    uint32_t T;          // outputs per workgroup: kThreads lanes, T / kThreads chains per lane
    bool direct;         // no window in LDS: every lane reads its samples from memory
    bool taps_global;    // the table stays in memory
    bool taps_uniform;   // U divides D: every output has phase 0, the one row of the table is read as wave-uniform scalars
    uint32_t pitch;      // floats per row of the table hp[phi][q] = h[phi + q U]
    uint32_t window;     // the largest window a tile can have (0 in the direct form)
    bool pad;            // the window is stored with one empty slot behind every 32 samples (resampler_slot)
    uint32_t step_i, step_phi;  // kThreads * D = step_i * U + step_phi: from one chain of a lane to its next
    size_t lds_bytes;
};

// The pitch: Q rounded up to a multiple of 4 floats (rows are read 16 bytes at a time) and then to an odd number of
// 16-byte units, so that consecutive rows start 16 bytes further round the 64 banks.
inline uint32_t resampler_pitch(uint32_t Q) {
    uint32_t p = (Q + 3) / 4;
    return 4 * (p | 1);
}

// Where window sample w lives in LDS.  Lane l of a wave reads sample floor(l D / U) + const: 8 bytes each, serviced 32
// lanes at a time over 64 banks, so the 32 samples of a group must differ mod 32.  At D/U >= 2 they do not (D/U = 4:
// four lanes per bank); one empty slot behind every 32 samples makes them differ for D/U = 2, 4, 8, 16, 32 and nearly
// so between those.  Below 2 the plain layout has at most two lanes per bank, and the two operations per read that the
// padded index costs are not worth paying.
HZ_HD uint32_t resampler_slot(uint32_t w, bool pad) { return pad ? w + (w >> 5) : w; }

inline Geom resampler_geom(uint32_t U, uint32_t D, uint32_t Q) {
    Geom g{};
    g.pitch = resampler_pitch(Q);
    g.taps_global = (uint64_t)U * g.pitch > kTableMax;
    auto window = [&](uint32_t T) { return (U - 1 + (T - 1) * D) / U + Q; };
    if (window(4 * kThreads) <= kWindowMax) {
        g.T = 4 * kThreads;
        g.window = window(g.T);
    } else if (window(kThreads) <= kWindowMax) {
        g.T = kThreads;
        g.window = window(g.T);
    } else {
        g.T = kThreads;
        g.direct = true;
    }
    g.step_i = (uint32_t)kThreads * D / U;
    g.step_phi = (uint32_t)kThreads * D % U;
    g.pad = !g.direct && D >= 2 * U;
    g.taps_uniform = !g.direct && !g.taps_global && D % U == 0;
    g.lds_bytes = (size_t)(g.window ? resampler_slot(g.window - 1, g.pad) + 1 : 0) * 8 + (g.taps_global || g.taps_uniform ? 0 : (size_t)U * g.pitch * 4);
    return g;
}

}  // namespace rs
}  // namespace hz
