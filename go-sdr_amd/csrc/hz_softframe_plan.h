// hz_softframe_plan.h -- the index arithmetic of the soft frame bank (include/hzsdr_softframe.h), HIP-free so that
// tests/host/softframe_plan.cpp can run it under the sanitizers and tests/host/softframe_ref.cpp can restate the bank
// with it: the validation of a configuration and of a push, the window test in uint64, where a payload's floats lie,
// the maps on bit patterns, the history's update and the sizes.
//
// Floats.  A row's stream of DECISION FLOATS has B floats per symbol: a real row's floats, a complex row's Re parts
// (B = 1) or its re, im, re, im ... (B = 2).  Decision float j of a push lies `in_step` input floats from the one before
// it (2 on complex rows read Re only, else 1).  Ps = P / B symbols make a payload, Kh = Ps - 1 symbols are kept per row:
// HF = Kh * B = P - B history floats, oldest first.
//
// The line.  In front of a push that consumes c symbols from p0 on, a row is the LINE history ++ input: HF + c * B
// floats, line float 0 being decision float (p0 - Kh) * B of the stream.  A served frame at symbol s starts at line
// float (s + Kh - p0) * B and ends inside the line; line float v is history float v when v < HF, else decision float
// v - HF of the push.  The new history is the line from float c * B on: HF floats.  A short push (c < Kh) takes some
// of them from the old history, which is why the history is written into a second buffer and the two change places.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace sfp {

constexpr int kRealF32 = 32, kC64 = 1;  // HZSDR_SYMSYNC_REAL_F32, HZSDR_FMT_C64
constexpr uint32_t kMaxRows = 8192, kMaxPayload = 8192, kMaxHyp = 4;
constexpr uint64_t kMaxSlots = 1ull << 22;     // rows * cap of a push
constexpr uint64_t kMaxPush = 0x7ffffff0u;     // symbols per row and push
constexpr uint64_t kMaxPosition = ~0ull >> 2;  // set_state: a position of at most 2^62 - 1
constexpr uint32_t kThreads = 256;             // a workgroup of the gather and of the history update
constexpr uint32_t kQuietNaN = 0x7FC00000u;    // what a frame outside the window is filled with
constexpr uint32_t kSignBit = 0x80000000u;
constexpr uint32_t kServed = 0, kOutside = 1, kNoHypothesis = 2;  // status
constexpr int kFormComplex = 1, kFormDibit = 2;
constexpr int kOk = 0, kInvalid = 1, kDstTooSmall = 2;

struct Config {
    int kind;
    uint32_t B, P, H;
    uint32_t maps[kMaxHyp];
};

// nullptr when the configuration makes a bank, else what is wrong with it (the kind is checked by the caller first)
inline const char *check_config(const Config &q) {
    if (q.kind != kRealF32 && q.kind != kC64) return "real float32 or complex64 rows";
    if (q.B != 1 && !(q.B == 2 && q.kind == kC64)) return "1 bit per symbol, or 2 on complex rows";
    if (q.P < q.B || q.P > kMaxPayload || q.P % q.B) return "B <= P <= 8192, P a multiple of B";
    if (q.H < 1 || q.H > kMaxHyp) return "1 ... 4 hypotheses";
    for (uint32_t h = 0; h < q.H; h++)
        if (q.maps[h] >= (q.B == 2 ? 4u : 2u)) return "maps: 0 or 1 (B = 1), 0 ... 3 (B = 2)";
    return nullptr;
}

struct Geom {
    uint32_t Ps;       // a payload's symbols: P / B
    uint32_t Kh;       // symbols kept per row: Ps - 1
    uint32_t HF;       // history floats per row: Kh * B
    uint32_t in_step;  // input floats from one decision float to the next
    uint32_t sym_floats;  // input floats per symbol: 2 on complex rows
    uint32_t step;     // floats a workgroup of the gather moves per step: one per lane, one pair per lane at B = 2
};

// a checked configuration
inline Geom geom(const Config &q) {
    Geom g{};
    g.Ps = q.P / q.B;
    g.Kh = g.Ps - 1;
    g.HF = g.Kh * q.B;
    g.sym_floats = q.kind == kC64 ? 2 : 1;
    g.in_step = q.kind == kC64 && q.B == 1 ? 2 : 1;
    g.step = kThreads * q.B;
    return g;
}

inline int form(const Config &q) { return (q.kind == kC64 ? kFormComplex : 0) | (q.B == 2 ? kFormDibit : 0); }

struct Call {
    uint64_t n, in_stride, cap, out_stride, rows;
    bool has_in, has_positions, has_info, has_counts, has_out, has_status;
};

// kOk, or why a push is refused before anything is launched
inline int check_call(const Config &q, const Call &c, const char **why) {
    *why = nullptr;
    if (c.rows > 1 && c.in_stride < c.n) return *why = "in_stride is below the symbols of the push", kInvalid;
    if (c.n > kMaxPush) return *why = "the push is too long", kInvalid;
    if (c.cap > kMaxSlots || c.rows * c.cap > kMaxSlots) return *why = "rows * cap is above 2^22", kInvalid;
    if (c.n && !c.has_in) return *why = "null input", kInvalid;
    if (c.cap && !(c.has_positions && c.has_info && c.has_counts && c.has_out && c.has_status))
        return *why = "null positions, info, counts, out or status", kInvalid;
    if (c.rows > 1 && c.out_stride < c.cap * q.P) return *why = "out_stride is below cap frames", kDstTooSmall;
    return kOk;
}

// the symbols a row consumes of a push
HZ_HD uint64_t consumed(uint64_t count, uint64_t n) { return count < n ? count : n; }

// The window test, without a sum that can wrap: is the frame at symbol s, under hypothesis h, served by the push that
// consumes [p0, p1)?  s + Kh >= p0 and s + Ps <= p1, Ps = Kh + 1; p1 = p0 + c is below 2^63.
HZ_HD uint32_t window_status(uint64_t s, uint32_t h, uint32_t H, uint64_t p0, uint64_t p1, uint32_t Kh) {
    if (h >= H) return kNoHypothesis;
    const uint64_t Ps = (uint64_t)Kh + 1;
    const bool from = p0 <= Kh || s >= p0 - Kh;
    const bool to = p1 >= Ps && s <= p1 - Ps;
    return from && to ? kServed : kOutside;
}

// a SERVED frame's first line float: (s + Kh - p0) * B, at most (c - 1) * B
HZ_HD uint64_t line_start(uint64_t s, uint64_t p0, uint32_t Kh, uint32_t B) { return (s + Kh - p0) * B; }

// line float v: in the history (slot v) or in the push's input (decision float v - HF)?
HZ_HD bool in_history(uint64_t v, uint32_t HF) { return v < HF; }
HZ_HD uint64_t input_float(uint64_t v, uint32_t HF, uint32_t in_step) { return (v - HF) * in_step; }

// the new history's float j is line float c * B + j
HZ_HD uint64_t carried_float(uint64_t c, uint32_t B, uint32_t j) { return c * B + j; }

// The maps, float by float: payload float k comes from the frame's float map_source(k) with its sign bit flipped when
// map_flip(k).  B = 1: map 1 flips.  B = 2, q times (x0, x1) -> (x1, -x0): q = 1: (x1, -x0), 2: (-x0, -x1), 3: (-x1, x0).
HZ_HD uint32_t map_source(uint32_t k, uint32_t map, uint32_t B) { return B == 2 ? k ^ (map & 1u) : k; }
HZ_HD uint32_t map_flip(uint32_t k, uint32_t map, uint32_t B) {
    if (B != 2) return (map & 1u) ? kSignBit : 0u;
    const uint32_t q = map & 3u;
    return ((k & 1u) ? (q == 1 || q == 2) : (q >= 2)) ? kSignBit : 0u;
}
// one pair at once (B = 2): (x0, x1) -> the mapped pair
HZ_HD void map_pair(uint32_t &x0, uint32_t &x1, uint32_t map) {
    const uint32_t a = (map & 1u) ? x1 : x0, b = (map & 1u) ? x0 : x1;
    x0 = a ^ map_flip(0, map, 2);
    x1 = b ^ map_flip(1, map, 2);
}

}  // namespace sfp
}  // namespace hz
