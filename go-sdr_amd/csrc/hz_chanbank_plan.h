// hz_chanbank_plan.h -- the host arithmetic of the channel bank (include/hzsdr_chanbank.h), HIP-free so that
// tests/host/chanbank_plan.cpp can run it under the sanitizers and tests/host/chanbank_ref.cpp can transcribe the
// kernel's indexing from the same functions.  Everything that can overflow lives here.
//
// The stream position, what a push does to it, the rotation and the position map are the polyphase banks' own
// (hz_polyphase_plan.h), taken by `using` and by their old names below.
//
// The product is A (2M x 2Mp, the DFT table as a real matrix, MFMA operand order, device memory and -- where it fits
// beside B -- LDS) times B (2Mp x T, the folded frames of one tile, LDS) on v_mfma_f32_16x16x4_f32.  A workgroup of four
// waves takes T = 64 or 32 consecutive frames of a push and ALL rows of A: the 16-row tiles of A are dealt to the
// waves in groups of two, a wave holds 2 x T/16 accumulators of 16 x 16, so eight or four independent chains cover
// the instruction's dependent latency.
//
// The LDS budget of a workgroup is hz_tuner_plan.h's: 66 KiB (16896 floats), two workgroups per CU with room to spare
// in the CU's 160 KiB.  B takes 2 Mp (T + 1) floats; T is 64 where B fits (M <= 128) and 32 otherwise (T = 32 fits for
// every M: 2 * 256 * 33 = 16896), A is staged behind B where both fit.  The tile does not depend on P, D or the format:
// the window is not staged, the fold reads it through the caches.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hz_chanbank_math.h"
#include "hz_polyphase_plan.h"

namespace hz {
namespace cp {

constexpr uint32_t kMinChannels = (uint32_t)ppp::kMatrixRule.lo, kMaxChannels = (uint32_t)ppp::kMatrixRule.hi, kMaxTapsPerChannel = ppp::kMaxTapsPerChannel;
constexpr int kThreads = 256, kWaves = 4;
constexpr uint32_t kGroupTiles = 2;  // 16-row tiles of A a wave works on at once
constexpr uint32_t kLdsFloats = 16896;  // 66 KiB

// ---- the counts, the rotation and the position map: the polyphase banks' own (hz_polyphase_plan.h) ------------
using ppp::kPushMax;
using ppp::State;
using ppp::Step;
// (under the names the kernel, tests/host/chanbank_plan.cpp and tests/host/chanbank_ref.cpp call them by)
HZ_HD uint32_t chanbank_rot(uint32_t rot, uint64_t f, uint32_t D, uint32_t M) { return ppp::rot(rot, f, D, M); }
inline Step chanbank_step(const State &s, uint32_t M, uint32_t L, uint32_t D, uint64_t n) { return ppp::step(s, M, L, D, n); }
HZ_HD uint32_t chanbank_pos(uint32_t k, uint32_t M, bool negative_first) { return ppp::pos(k, M, negative_first); }

// ---- the tile --------------------------------------------------------------------------------------------
struct Geom {
    uint32_t M, Mp;        // channels; M rounded up to even
    uint32_t T, col_tiles; // frames per workgroup: 64 or 32; T / 16
    uint32_t pitch;        // complex slots of one r of B: T + 1 (odd: the fold's stores of consecutive r spread over the banks)
    uint32_t steps;        // k-steps of the product: 2 Mp / 4
    uint32_t row_tiles;    // 16-row tiles of A, 2M rounded up to whole groups (the rows behind 2M are +0)
    uint32_t groups;       // row_tiles / kGroupTiles, dealt to the waves round robin
    uint32_t fold_shift;   // the fold gives 2^fold_shift lanes to a frame (the power of two at or above Mp, at most 64)
    bool a_lds;            // A is staged in LDS behind B
    uint32_t b_floats;
    size_t a_floats, lds_bytes;
};

inline uint32_t chanbank_b_floats(uint32_t Mp, uint32_t T) { return 2 * Mp * (T + 1); }

// (out of line, as chanbank_fill_a is: both stay in the library's symbol table)
__attribute__((noinline)) inline Geom chanbank_geom(uint32_t M) {
    Geom g{};
    g.M = M;
    g.Mp = (M + 1) & ~1u;
    g.steps = g.Mp / 2;
    g.T = chanbank_b_floats(g.Mp, 64) <= kLdsFloats ? 64 : 32;  // (a smaller tile where the larger does not fit)
    g.col_tiles = g.T / 16;
    g.pitch = g.T + 1;
    g.row_tiles = ((2 * M + 15) / 16 + kGroupTiles - 1) / kGroupTiles * kGroupTiles;
    g.groups = g.row_tiles / kGroupTiles;
    g.fold_shift = 1;
    while (g.fold_shift < 6 && (1u << g.fold_shift) < g.Mp) g.fold_shift++;
    g.b_floats = chanbank_b_floats(g.Mp, g.T);
    g.a_floats = (size_t)g.row_tiles * g.steps * 64;
    g.a_lds = g.b_floats + g.a_floats <= kLdsFloats;
    g.lds_bytes = ((size_t)g.b_floats + (g.a_lds ? g.a_floats : 0)) * sizeof(float);
    return g;
}

// ---- both operand layouts --------------------------------------------------------------------------------
// Element (row, j) of A, j = 2 r + c the inner index (c = 0: the factor of u.re, c = 1: of u.im).  Lane l of
// v_mfma_f32_16x16x4_f32 holds A[l & 15][l >> 4] of a 16 x 4 block: for each 16-row tile and each k-step the 64 lanes'
// values are contiguous (hz_tuner_plan.h's order).
HZ_HD size_t chanbank_a_index(uint32_t row, uint32_t j, uint32_t steps) {
    return ((size_t)(row / 16) * steps + j / 4) * 64 + (j % 4) * 16 + row % 16;
}
// Element (j, f) of B, f the frame of the tile: (re, im) of one r side by side, the frames of one r consecutive.  Lane l
// of a B-operand read holds B[4 s + (l >> 4)][l & 15]: lanes 0 .. 31 (k = 0, 1: re and im of one r) read 32 consecutive
// floats, lanes 32 .. 63 the 32 of r + 1 -- ds_read_b32 serves the halves apart and its banks are the address modulo
// 32 floats, so every read is free of conflicts whatever the pitch.
HZ_HD uint32_t chanbank_b_index(uint32_t j, uint32_t f, uint32_t pitch) { return ((j >> 1) * pitch + f) * 2 + (j & 1u); }

// floor(w / M) is div_by_magic(w, div_magic(M)) (hz_plan.h): the fold's rotation of frame fl of a tile is
// (rot0 + fl D) mod M with rot0 + fl D <= 254 + 63 * 255, and M <= 255 keeps w M far below 2^32

// frame offset of fold output r at tap row 0 for a frame whose rotation is s: (r - s) mod M
HZ_HD uint32_t chanbank_offset(uint32_t r, uint32_t s, uint32_t M) { return r >= s ? r - s : r + M - s; }

}  // namespace cp
}  // namespace hz

// Host only from here on: the table.
#include <math.h>

namespace hz {
namespace cp {

// (cos, sin) of 2 pi n / M, 0 <= n < M, in float64.  The integer phase is first reduced, exactly, to the first half
// quadrant: 4 n = quad M + p with 0 <= p < M is the angle quad pi/2 + (pi/2) p / M, mirrored at pi/4 where 2 p > M.  The
// values on the axes are exact: cos = 1, sin = +0 at n = 0; cos = +0, sin = 1 at 4 n = M.
inline void chanbank_unit(uint32_t n, uint32_t M, double *c, double *s) {
    const uint32_t quad = 4 * n / M, p = 4 * n - quad * M;
    const double k = 1.5707963267948966192313216916398 / (double)M;
    double cr, sr;
    if (2 * p <= M) {
        cr = cos(p * k), sr = sin(p * k);
    } else {
        cr = sin((M - p) * k), sr = cos((M - p) * k);
    }
    if (p == 0) cr = 1.0, sr = 0.0;
    switch (quad) {
    case 0: *c = cr, *s = sr; break;
    case 1: *c = 0.0 - sr, *s = cr; break;
    case 2: *c = 0.0 - cr, *s = 0.0 - sr; break;
    default: *c = sr, *s = 0.0 - cr; break;
    }
}

// W[k][r] = exp(-2 pi i ((k r) mod M) / M), each component rounded once; +0 + 0i for r >= M
inline cb::c32 chanbank_table(uint32_t k, uint32_t r, uint32_t M) {
    if (r >= M) return cb::c32{0.0f, 0.0f};
    double c, s;
    chanbank_unit(k * r % M, M, &c, &s);
    return cb::c32{(float)c, (float)(0.0 - s)};
}

// the table, M rows of Mp entries
inline std::vector<cb::c32> chanbank_tables(uint32_t M) {
    const uint32_t Mp = (M + 1) & ~1u;
    std::vector<cb::c32> W((size_t)M * Mp);
    for (uint32_t k = 0; k < M; k++)
        for (uint32_t r = 0; r < Mp; r++) W[(size_t)k * Mp + r] = chanbank_table(k, r, M);
    return W;
}

// A in operand order from the table: row 2k is (w.re, -w.im) interleaved over r, row 2k + 1 is (w.im, w.re); the rows
// behind 2M are +0
__attribute__((noinline)) inline std::vector<float> chanbank_fill_a(const Geom &g, const std::vector<cb::c32> &W) {
    std::vector<float> A(g.a_floats, 0.0f);
    for (uint32_t k = 0; k < g.M; k++)
        for (uint32_t r = 0; r < g.Mp; r++) {
            const cb::c32 w = W[(size_t)k * g.Mp + r];
            A[chanbank_a_index(2 * k, 2 * r, g.steps)] = w.re;
            A[chanbank_a_index(2 * k, 2 * r + 1, g.steps)] = -w.im;
            A[chanbank_a_index(2 * k + 1, 2 * r, g.steps)] = w.im;
            A[chanbank_a_index(2 * k + 1, 2 * r + 1, g.steps)] = w.re;
        }
    return A;
}

}  // namespace cp
}  // namespace hz
