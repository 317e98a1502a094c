// hz_symsync_plan.h -- the host arithmetic of the symbol-timing recovery bank (include/hzsdr_symsync.h), HIP-free so that
// tests/host/symsync_plan.cpp can run it under the sanitizers.  The bank is a row-wave bank: how the rows are dealt to
// waves, the sample tile and its address maps are hz_rowwave_plan.h, with the reasons.  Here: the symbol tile, its
// address maps (a host program counts bank conflicts from the same functions) and the LDS request of both tiles, the
// derivation and validation of a row's loop constants, the bound on a push's symbols and the indices of the kept state.
//
// The output is ragged.  A strobe is found at most once per sample and the flag alternates between the
// mid-symbol and the symbol strobe whatever the data, so a tile of T samples emits at most T / 2 + 1 symbols per row
// (tile_symbols; T / 2 when T is even, one more kept in hand).  The SYMBOL TILE holds them apart from the sample tile:
// the k-th symbol of the tile of row r at float k * P + r of its plane, (T / 2 + 1) * P floats per plane.  The walk
// writes it with lane = row; behind the walk the rows are stored one after the other with lane = symbol (floats P
// apart: P is odd, so the 32 lanes of a group fall on 32 distinct banks).  The walk's own write is conflict-free while
// the rows of a wave have emitted equally many symbols (equal clocks, the common case); rows whose counts differ may
// share a bank, which costs a cycle and nothing else.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "hz_rowwave_plan.h"
#include "hz_symsync_math.h"

namespace hz {
namespace sp {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kSteps, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count, rw::tile_slot, rw::move_slot, rw::walk_slot;

constexpr uint32_t kParams = 4;        // sps, limit, g_mu, g_omega
constexpr size_t kLdsOwn = 28 * 1024;  // what both tiles of this bank stay under

// the most symbols of one row out of a tile of T samples
constexpr uint32_t tile_symbols(uint32_t T) { return T / 2 + 1; }

struct Geom : rw::Geom {  // (P is also the floats from one symbol of the symbol tile to the next)
    uint32_t Y;         // symbols per row the symbol tile holds: tile_symbols(T)
    uint32_t sym_base;  // floats from the start of the LDS to the symbol tile
    size_t lds_bytes;
};

inline Geom symsync_geom(uint32_t rows, bool complex_rows) {
    Geom g{rw::geom(rows, complex_rows), 0, 0, 0};
    g.Y = tile_symbols(g.T);
    g.sym_base = rw::tile_floats(g);
    g.lds_bytes = ((size_t)g.sym_base + (size_t)g.planes * g.Y * g.P) * 4;
    return g;
}

// ---- the symbol tile's address maps, in floats from its own start (Geom::sym_base) ----
// symbol k of the tile of row r, plane p; Y = tile_symbols(T)
HZ_HD uint32_t sym_slot(uint32_t k, uint32_t r, uint32_t p, uint32_t P, uint32_t Y) { return p * Y * P + k * P + r; }
// the walk: lane l owns row l and writes its k-th symbol of the tile
HZ_HD uint32_t emit_slot(uint32_t lane, uint32_t k, uint32_t p, uint32_t P, uint32_t Y) { return sym_slot(k, lane, p, P, Y); }
// the storer: lane l, step j, row r: symbol l + 64 j
HZ_HD uint32_t store_slot(uint32_t lane, uint32_t j, uint32_t r, uint32_t p, uint32_t P, uint32_t Y) {
    return sym_slot(lane + kLanes * j, r, p, P, Y);
}

// ---- the loop constants ----
struct Derived {
    float h0;  // sps / 2: the half period at create and reset
    sm::Loop loop;
};

// (sps, limit, g_mu, g_omega) -> h0 = sps / 2, hmin = h0 (1 - limit), hmax = h0 (1 + limit), each computed in float64 and
// rounded to float32
inline Derived derive(const float *q) {
    const double h0 = (double)q[0] / 2.0;
    Derived d;
    d.h0 = (float)h0;
    d.loop.g_mu = q[2];
    d.loop.g_omega = q[3];
    d.loop.hmin = (float)(h0 * (1.0 - (double)q[1]));
    d.loop.hmax = (float)(h0 * (1.0 + (double)q[1]));
    return d;
}

// nullptr when the four values make a loop, else what is wrong with them.  The last condition, in float32 exactly as the
// kernel sees it (the smallest advance is fmaf(g_mu, -1, hmin)), keeps every advance at 1 or above: at most one strobe
// per sample, and a counter that never goes below 0.
inline const char *check_params(const float *q) {
    for (uint32_t k = 0; k < kParams; k++)
        if (!isfinite(q[k])) return "a parameter is not finite";
    if (!(q[0] > 2.0f && q[0] <= 256.0f)) return "2 < sps <= 256";
    if (!(q[1] >= 0.0f && q[1] <= 0.25f)) return "0 <= limit <= 0.25";
    if (!(q[2] >= 0.0f && q[3] >= 0.0f)) return "the gains are not negative";
    const Derived d = derive(q);
    const volatile float least = d.loop.hmin - d.loop.g_mu;
    if (!(least >= 1.0f)) return "hmin - g_mu is below 1: more than one strobe per sample";
    return nullptr;
}

// hmin - g_mu of a row in float64, from the float32 values the kernel holds
inline double least_advance(const float *q) {
    const Derived d = derive(q);
    return (double)d.loop.hmin - (double)d.loop.g_mu;
}

// The most symbols a push of n samples writes into one row.  A symbol strobe and the next are a mid-symbol advance
// (h >= hmin) and a symbol advance (>= hmin - g_mu) apart, so at least 2 amin, amin the smallest hmin - g_mu over the
// rows; the float32 counter rounds each of its sums and differences by at most 2^-24 relative, which the margin of
// 2^-20 on amin covers.  n samples hold at most floor(n / (2 amin)) + 1 strobes that far apart; one more for the one
// interval that may be shorter: behind set_params the next mid-symbol advance is still the old h (at least 1, as
// every accepted h is), so two symbols may be 1 + amin apart, once.  0 for an empty push.
inline uint64_t max_symbols(uint64_t n, double amin) {
    if (n == 0) return 0;
    const double a = amin * (1.0 - 1.0 / 1048576.0);
    return (uint64_t)floor((double)n / (2.0 * a)) + 2;
}

// ---- the kept state (include/hzsdr_symsync.h): row-major, per row c, h, flag, y_prev, y_mid, x1, x2, x3, the five
// sample-valued entries as (re, im) pairs for complex rows ----
enum { kStC = 0, kStH = 1, kStFlag = 2, kStYp = 3, kStYm = 4, kStX1 = 5, kStX2 = 6, kStX3 = 7 };
HZ_HD uint32_t state_row_floats(uint32_t planes) { return 3 + 5 * planes; }
// entry: kStC ... kStX3; p: the plane of a sample-valued entry
HZ_HD size_t state_index(size_t row, uint32_t entry, uint32_t p, uint32_t planes) {
    return row * (3 + 5 * planes) + (entry < 3 ? entry : 3 + (entry - 3) * planes + p);
}
inline size_t state_floats(uint32_t rows, uint32_t planes) { return (size_t)rows * state_row_floats(planes); }

}  // namespace sp
}  // namespace hz
