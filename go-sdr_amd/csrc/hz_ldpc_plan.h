// hz_ldpc_plan.h -- the host arithmetic of the LDPC decoder bank (include/hzsdr_ldpc.h), HIP-free so that
// tests/host/ldpc_plan.cpp can run it under the sanitizers: the validation of a bank's scalars and of the caller's two
// arrays (no field of an array indexes anything before it is checked), the edge tables the kernel reads, how frames are
// dealt to workgroups and threads, and the LDS layout and request.
//
// Tables.  The kernel walks the code twice per iteration: check by check (row_ptr, col: the caller's arrays, col
// narrowed to 16 bits since n <= 16384) and variable by variable (vptr uint32[n + 1], vedge uint16[E]: the numbers of a
// variable's edges, ascending -- E <= 65536, so an edge number fits 16 bits).  Both walks are made once at create.
//
// Threads.  A frame has T threads, a multiple of 64 (a wave never holds two frames' threads), enough for a check and for
// two variables per thread where 1024 allow it; thread t of a frame takes the checks t, t + T, ... and the variables
// t, t + T, ...  A workgroup decodes G frames side by side, G * T <= 1024, G <= kMaxGroup, as many as the LDS holds;
// workgroup w takes the frame slots [w G, (w + 1) G) (slot = row * cap + frame), then those a grid further on.
//
// LDS.  [0, kHeadBytes): the unsatisfied-check counters, two generations of G words; then, where they fit beside ONE
// frame's state (FORM_TABLES_LDS), the four tables; then G frames of frame_bytes each: P int16[n], q int8[n], the
// messages int8[E].  The largest code asks 32 + 16 + 64 KiB for its frame and reads its tables through the cache
// (FORM_TABLES_CACHE).  The budget is the 160 KiB a CU has.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hz_decodebank_plan.h"
#include "hz_ldpc_math.h"

namespace hz {
namespace lp {

using dbp::kBits, dbp::kSoftF32, dbp::kMaxRows, dbp::kMaxFrames;  // HZSDR_LDPC_BITS, HZSDR_LDPC_SOFT_F32
constexpr int kFormTablesLds = 1, kFormTablesCache = 2;  // HZSDR_LDPC_FORM_*
constexpr uint32_t kMaxChecks = 16384, kMaxVars = 16384, kMaxEdges = 65536, kMaxDegree = 64, kMinCheckDegree = 2;
constexpr uint32_t kMaxBits = 8192, kMaxIters = 255, kMaxNorm = 16, kMaxOffset = 126, kMaxLevel = 127;
constexpr uint32_t kLanes = 64, kMaxThreads = 1024, kMaxGroup = 8, kMaxGrid = 2048;
constexpr uint32_t kHeadBytes = 2 * kMaxGroup * 4;
constexpr size_t kLdsBudget = 160 * 1024;

struct Config {
    int kind;
    uint64_t m, n, E, head, N, D;
    float scale;
    uint32_t level, max_iters, a, beta;
};

// nullptr when the scalars make a bank, else what is wrong with them (the kind is the caller's to check first)
inline const char *check_config(const Config &q) {
    if (q.m < 1 || q.m > kMaxChecks) return "1 <= checks <= 16384";
    if (q.n < 2 || q.n > kMaxVars) return "2 <= variables <= 16384";
    if (q.E < 1 || q.E > kMaxEdges) return "1 <= edges <= 65536";
    if (q.N < 1 || q.N > kMaxBits) return "1 <= received <= 8192";
    if (q.head > q.n || q.N > q.n - q.head) return "head + received <= variables";
    if (q.D < 1 || q.D > q.n) return "1 <= data_bits <= variables";
    if (q.max_iters < 1 || q.max_iters > kMaxIters) return "1 <= max_iters <= 255";
    if (q.a < 1 || q.a > kMaxNorm) return "1 <= norm <= 16";
    if (q.beta > kMaxOffset) return "offset <= 126";
    if (const char *why = q.kind == kSoftF32 ? dbp::check_scale(q.scale) : nullptr) return why;
    if (q.kind == kBits && (q.level < 1 || q.level > kMaxLevel)) return "1 <= level <= 127";
    return nullptr;
}

// the caller's arrays under checked scalars: row_ptr has m + 1 entries, col has E
inline const char *check_code(const Config &q, const uint32_t *row_ptr, const uint32_t *col) {
    const uint32_t m = (uint32_t)q.m, n = (uint32_t)q.n, E = (uint32_t)q.E;
    if (row_ptr[0] != 0) return "row_ptr[0] is 0";
    for (uint32_t c = 0; c < m; c++) {
        const uint32_t a = row_ptr[c], b = row_ptr[c + 1];
        if (b < a) return "row_ptr does not descend";
        if (b - a < kMinCheckDegree || b - a > kMaxDegree) return "every check has degree 2 ... 64";
        if (b > E) return "row_ptr stays inside the edges";
    }
    if (row_ptr[m] != E) return "row_ptr[checks] is edges";
    std::vector<uint8_t> deg(n, 0);
    for (uint32_t c = 0; c < m; c++) {
        for (uint32_t e = row_ptr[c]; e < row_ptr[c + 1]; e++) {
            const uint32_t v = col[e];
            if (v >= n) return "a column is below variables";
            if (e > row_ptr[c] && v <= col[e - 1]) return "columns ascend strictly inside a check";
            if (deg[v] == kMaxDegree) return "every variable has degree 1 ... 64";
            deg[v]++;
        }
    }
    for (uint32_t v = 0; v < n; v++)
        if (deg[v] == 0) return "every variable has degree 1 ... 64";
    return nullptr;
}

struct Tables {
    std::vector<uint32_t> row_ptr, vptr;  // m + 1, n + 1
    std::vector<uint16_t> col, vedge;     // E, E
};

// a checked code
inline void build_tables(const Config &q, const uint32_t *row_ptr, const uint32_t *col, Tables &t) {
    const uint32_t m = (uint32_t)q.m, n = (uint32_t)q.n, E = (uint32_t)q.E;
    t.row_ptr.assign(row_ptr, row_ptr + m + 1);
    t.col.resize(E);
    t.vptr.assign(n + 1, 0);
    for (uint32_t e = 0; e < E; e++) t.col[e] = (uint16_t)col[e], t.vptr[col[e] + 1]++;
    for (uint32_t v = 0; v < n; v++) t.vptr[v + 1] += t.vptr[v];
    t.vedge.resize(E);
    std::vector<uint32_t> at(t.vptr.begin(), t.vptr.end() - 1);
    for (uint32_t e = 0; e < E; e++) t.vedge[at[col[e]]++] = (uint16_t)e;
}

inline uint32_t up(uint32_t v, uint32_t to) { return (v + to - 1) / to * to; }

struct Geom {
    uint32_t m, n, E, head, N, D, FB, DB;
    uint32_t T, G;  // threads per frame; frames per workgroup
    int form;
    uint32_t off_rowptr, off_vptr, off_col, off_vedge;  // LDS, bytes (FORM_TABLES_LDS)
    uint32_t off_frames, frame_bytes;                   // frame g at off_frames + g * frame_bytes
    uint32_t off_q, off_r;                              // inside a frame: P at 0, q, the messages
    uint32_t table_bytes;
    size_t lds_bytes;
};

// a checked configuration
inline Geom geom(const Config &q) {
    Geom g{};
    g.m = (uint32_t)q.m, g.n = (uint32_t)q.n, g.E = (uint32_t)q.E, g.head = (uint32_t)q.head, g.N = (uint32_t)q.N, g.D = (uint32_t)q.D;
    g.FB = dbp::packed_bytes(g.N), g.DB = dbp::packed_bytes(g.D);
    uint32_t want = g.m > (g.n + 1) / 2 ? g.m : (g.n + 1) / 2;
    g.T = up(want, kLanes);
    if (g.T > kMaxThreads) g.T = kMaxThreads;
    g.off_q = up(2 * g.n, 4);
    g.off_r = g.off_q + up(g.n, 4);
    g.frame_bytes = up(g.off_r + g.E, 16);
    g.table_bytes = up(4 * (g.m + 1) + 4 * (g.n + 1) + 2 * g.E + 2 * g.E, 16);
    const bool in_lds = (size_t)kHeadBytes + g.table_bytes + g.frame_bytes <= kLdsBudget;
    g.form = in_lds ? kFormTablesLds : kFormTablesCache;
    g.off_rowptr = kHeadBytes;
    g.off_vptr = g.off_rowptr + 4 * (g.m + 1);
    g.off_col = g.off_vptr + 4 * (g.n + 1);
    g.off_vedge = g.off_col + 2 * g.E;
    g.off_frames = kHeadBytes + (in_lds ? g.table_bytes : 0);
    g.G = kMaxThreads / g.T;
    if (g.G > kMaxGroup) g.G = kMaxGroup;
    const size_t room = (kLdsBudget - g.off_frames) / g.frame_bytes;
    if (g.G > room) g.G = (uint32_t)room;
    g.lds_bytes = (size_t)g.off_frames + (size_t)g.G * g.frame_bytes;
    return g;
}

// the workgroups of a call over `slots` frame slots
inline uint32_t groups_for(const Geom &g, size_t slots) {
    const size_t w = (slots + g.G - 1) / g.G;
    return (uint32_t)(w < kMaxGrid ? w : kMaxGrid);
}

}  // namespace lp
}  // namespace hz
