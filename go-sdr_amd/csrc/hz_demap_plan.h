// hz_demap_plan.h -- the host arithmetic of the demapper bank (include/hzsdr_demap.h), HIP-free so that
// tests/host/demap_plan.cpp can run it under the sanitizers: the validation of a bank's scalars and of the caller's
// arrays (no entry of perm indexes anything before it is checked), the validation of a call on top of the decoder banks'
// (hz_decodebank_plan.h: the slot arithmetic and slot_frame are theirs), how frames are dealt to workgroups and threads,
// and the LDS request.
//
// Threads.  Lane = symbol: a frame has T threads, S rounded up to whole waves, kMaxFrameThreads at the most; thread t takes the
// symbols t, t + T, ... and then the outputs t, t + T, ...  A workgroup takes G frames side by side, G * T <= 1024,
// G <= kMaxGroup, as many as kLdsBudget holds; workgroup w takes the frame slots [w G, (w + 1) G) (slot = row * cap +
// frame), then those a grid further on.
//
// LDS.  G frames of frame_floats = S m rounded up to 4 floats each: a frame's values L[s m + j], written symbol by symbol
// and read in output order.  The largest frame asks 64 KiB, so two workgroups of 1024 threads fit a CU.
// HZ_DEMAP_BLOCK, HZ_DEMAP_FRAME_THREADS and HZ_DEMAP_TREE_FROM are build-time switches for A/B measurements (the Makefile's
// EXTRA); only HZ_DEMAP_TREE_FROM has been measured, the other two stand at the values first written.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_decodebank_plan.h"
#include "hz_demap_math.h"

namespace hz {
namespace dmp {

using dbp::kMaxRows, dbp::kMaxFrames;
constexpr int kC64 = 1, kRealF32 = 32, kLlrF32 = 33;       // HZSDR_DEMAP_C64, _REAL_F32, _LLR_F32
constexpr int kFormGrouped = 1, kFormPerm = 2, kFormTree = 4;  // HZSDR_DEMAP_FORM_*
constexpr uint32_t kMaxBits = 8, kMaxSymbols = 8192, kMaxLlrs = 16384, kMaxOut = 8192;
#ifndef HZ_DEMAP_BLOCK
#define HZ_DEMAP_BLOCK 1024
#endif
#ifndef HZ_DEMAP_FRAME_THREADS
#define HZ_DEMAP_FRAME_THREADS 1024
#endif
constexpr uint32_t kLanes = 64, kMaxThreads = HZ_DEMAP_BLOCK, kMaxFrameThreads = HZ_DEMAP_FRAME_THREADS, kMaxGroup = 8, kMaxGrid = 4096;
constexpr size_t kLdsBudget = 64 * 1024;
// from this m on the kernel takes the minima by the two-sided tree (measured: DESIGN.md section 4)
#ifndef HZ_DEMAP_TREE_FROM
#define HZ_DEMAP_TREE_FROM 7
#endif
constexpr uint32_t kTreeFrom = HZ_DEMAP_TREE_FROM;

inline bool known(int kind) { return kind == kC64 || kind == kRealF32 || kind == kLlrF32; }
inline bool finite(float v) { return v - v == 0.0f; }

struct Config {
    int kind;
    uint64_t m, S, N;
    bool has_points, has_perm;
    uint64_t n_gains, rows;
};

// nullptr when the scalars make a bank, else what is wrong with them (the kind is the caller's to check first)
inline const char *check_config(const Config &q) {
    if (q.rows < 1 || q.rows > kMaxRows) return "1 ... 8192 rows";
    if (q.m < 1 || q.m > kMaxBits) return "1 <= bits_per_symbol <= 8";
    if (q.kind == kLlrF32 && (q.m != 1 || q.has_points)) return "values that are per-bit already have one bit per symbol and no points";
    if (q.kind != kLlrF32 && !q.has_points) return "null points";
    if (q.S < 1 || q.S > kMaxSymbols) return "1 <= symbols <= 8192";
    if (q.S * q.m > kMaxLlrs) return "symbols * bits_per_symbol <= 16384";
    if (q.N < 1 || q.N > kMaxOut) return "1 <= received <= 8192";
    if (!q.has_perm && q.N != q.S * q.m) return "without perm received is symbols * bits_per_symbol";
    if (q.n_gains != 1 && q.n_gains != q.rows) return "one gain, or one per row";
    return nullptr;
}

// the caller's arrays under checked scalars: points has 2 M or M floats, perm N entries, gains n_gains
inline const char *check_arrays(const Config &q, const float *points, const uint32_t *perm, const float *gains) {
    const uint32_t count = q.kind == kLlrF32 ? 0 : (uint32_t)((q.kind == kC64 ? 2u : 1u) << q.m);
    for (uint32_t i = 0; i < count; i++)
        if (!finite(points[i])) return "every point is finite";
    if (!gains) return "null gains";
    for (uint64_t i = 0; i < q.n_gains; i++)
        if (!(gains[i] > 0.0f) || !finite(gains[i])) return "a gain is finite and positive";
    if (q.has_perm) {
        const uint32_t L = (uint32_t)(q.S * q.m);
        for (uint64_t k = 0; k < q.N; k++)
            if (perm[k] >= L && perm[k] != dm::kErased) return "a perm entry is below symbols * bits_per_symbol, or HZSDR_DEMAP_ERASED";
    }
    return nullptr;
}

inline uint32_t up(uint32_t v, uint32_t to) { return (v + to - 1) / to * to; }

struct Geom {
    uint32_t S, W, m, N, L;  // L = S m
    uint32_t T, G;           // threads per frame; frames per workgroup
    uint32_t frame_floats;   // frame g at float g * frame_floats of the LDS
    int form;
    size_t lds_bytes;
};

// a checked configuration
inline Geom geom(const Config &q) {
    Geom g{};
    g.S = (uint32_t)q.S, g.m = (uint32_t)q.m, g.N = (uint32_t)q.N, g.L = g.S * g.m;
    g.W = q.kind == kC64 ? 2 * g.S : g.S;
    g.T = up(g.S, kLanes);
    if (g.T > kMaxFrameThreads) g.T = kMaxFrameThreads;
    g.frame_floats = up(g.L, 4);
    g.G = kMaxThreads / g.T;
    if (g.G > kMaxGroup) g.G = kMaxGroup;
    const size_t room = kLdsBudget / (4 * (size_t)g.frame_floats);
    if (g.G > room) g.G = (uint32_t)room;
    g.form = (g.G > 1 ? kFormGrouped : 0) | (q.has_perm ? kFormPerm : 0) | (q.kind != kLlrF32 && g.m >= kTreeFrom ? kFormTree : 0);
    g.lds_bytes = (size_t)g.G * g.frame_floats * 4;
    return g;
}

// the workgroups of a call over `slots` frame slots
inline uint32_t groups_for(const Geom &g, size_t slots) {
    const size_t w = (slots + g.G - 1) / g.G;
    return (uint32_t)(w < kMaxGrid ? w : kMaxGrid);
}

// ---- a call ----
inline dbp::Slots slots_of(const Geom &g) { return {g.W, g.N, false, "in_stride is below cap frames", "out_stride is below cap frames"}; }
// the decoder banks' check (this bank has no info word: has_info is true), then: the two blocks lie apart
inline int check_run(const Geom &g, const dbp::Call &c, const char **why) {
    const int bad = dbp::check_call(slots_of(g), c, why);
    if (bad) return bad;
    // (strides beyond any address space are refused before they are multiplied: 2^13 rows of 2^40 floats fit 64 bits)
    const size_t lim = (size_t)1 << 40;
    if (c.rows > 1 && (c.in_stride > lim || c.out_stride > lim)) return *why = "a stride beyond 2^40", dbp::kInvalid;
    const uint64_t ispan = 4 * ((uint64_t)(c.rows - 1) * (c.rows > 1 ? c.in_stride : 0) + (uint64_t)c.cap * g.W);
    const uint64_t ospan = 4 * ((uint64_t)(c.rows - 1) * (c.rows > 1 ? c.out_stride : 0) + (uint64_t)c.cap * g.N);
    if ((uint64_t)c.in < (uint64_t)c.out + ospan && (uint64_t)c.out < (uint64_t)c.in + ispan) return *why = "in and out overlap", dbp::kInvalid;
    return dbp::kOk;
}

}  // namespace dmp
}  // namespace hz
