// hz_polyphase_plan.h -- the host arithmetic the polyphase banks (hz_channelizer.hip, hz_synthesizer.hip,
// hz_chanbank.hip) share, HIP-free so that tests/host/polyphase_plan.cpp can run it under the sanitizers: the stream
// position and what a push does to it, the rotation, the position map, the argument check of a create and the
// synthesis bank's counts of one group of frames.  Everything that can overflow lives here; nothing here knows which
// bank it serves.
//
// The stream position is three running values: the samples held (converted, below L), the rotation (position of the
// next frame's first sample) mod M and the index of the next frame.  No product with the stream length is ever formed.
// The forms are the general ones, for any M: for a power of two they equal the `& (M - 1)` forms that the transform
// kernels keep (the test proves it).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace ppp {

constexpr uint32_t kMaxTapsPerChannel = 32;
constexpr uint64_t kPushMax = (uint64_t)1 << 62;  // samples of one push: held + n and every index below 2^63

// ---- the stream position ----------------------------------------------------------------------------------
struct State {
    uint64_t held = 0;   // samples held for the next frame (below L); the synthesis bank: partial sums held, 0 or L - D
    uint32_t rot = 0;    // (stream position of the next frame's first sample) mod M
    uint64_t frame = 0;  // index of the next frame
};

struct Step {
    bool ok;        // false: the push is too long for the counts
    uint64_t V, F;  // samples of the virtual buffer held ++ in; frames that complete in the push
    State next;
};

// (rot + f D) mod M without a product of the stream length: f is reduced first
HZ_HD uint32_t rot(uint32_t rot, uint64_t f, uint32_t D, uint32_t M) {
    return (uint32_t)((rot + (f % M) * D) % M);  // below M + (M - 1) M, M at most 8192
}

// what a push of n samples does to an analysis bank of M channels, L taps and hop D
inline Step step(const State &s, uint32_t M, uint32_t L, uint32_t D, uint64_t n) {
    Step p{};
    if (n > kPushMax) return p;
    p.ok = true;
    p.V = s.held + n;
    p.F = p.V >= L ? (p.V - L) / D + 1 : 0;
    p.next.held = p.V - p.F * D;  // (D <= M <= L: never a gap; below L)
    p.next.rot = rot(s.rot, p.F, D, M);
    p.next.frame = s.frame + p.F;
    return p;
}

// ---- the position map -------------------------------------------------------------------------------------
// ascending signed frequency for NegativeFirst: position 0 is channel ceil(M / 2), i.e. -floor(M / 2) fs / M
HZ_HD uint32_t pos(uint32_t k, uint32_t M, bool negative_first) {
    if (!negative_first) return k;
    const uint32_t p = k + M / 2;
    return p >= M ? p - M : p;
}

// ---- the arguments of a create ----------------------------------------------------------------------------
// a bank's own rule for M
struct ChannelRule {
    size_t lo, hi;
    bool pow2;
};
constexpr ChannelRule kTransformRule{256, 8192, true};  // the channelizer and the synthesis bank: the sizes of hz_fftv.h
constexpr ChannelRule kMatrixRule{2, 255, false};       // the channel bank

constexpr int kOrderZeroFirst = 0, kOrderNegativeFirst = 1;  // HZSDR_ORDER_*
constexpr int kFrameMajor = 0, kChannelMajor = 1;            // HZSDR_CHANNELIZER_*_MAJOR

// which refusal fired: the first in this order, kArgsOk for none
enum Refusal { kArgsOk = 0, kBadChannels, kNullTaps, kBadTaps, kBadHop, kBadOrder, kBadLayout };

inline Refusal check_args(const ChannelRule &r, size_t m, bool has_taps, size_t n_taps, size_t hop, int order, int layout) {
    if (m < r.lo || m > r.hi || (r.pow2 && (m & (m - 1)) != 0)) return kBadChannels;
    if (!has_taps) return kNullTaps;
    if (n_taps == 0 || n_taps % m != 0 || n_taps > kMaxTapsPerChannel * m) return kBadTaps;
    if (hop == 0 || hop > m) return kBadHop;
    if (order != kOrderZeroFirst && order != kOrderNegativeFirst) return kBadOrder;
    if (layout != kFrameMajor && layout != kChannelMajor) return kBadLayout;
    return kArgsOk;
}

// ---- the synthesis bank's groups --------------------------------------------------------------------------
// The scratch one group of frames may take (group_frames * M * 8 bytes): small enough to stay in the memory-side cache
// between the two kernels, large enough that the launches of a group do not show.
constexpr size_t kSynthScratchBytes = (size_t)16 << 20;
constexpr size_t group_frames(size_t M) { return kSynthScratchBytes / (M * 8); }
// frames the scratch has room for after a push of n frames (grow-only)
constexpr size_t scratch_frames(size_t n, size_t M) { return n < group_frames(M) ? n : group_frames(M); }

// The overlap-add of one group of F frames (F at most group_frames(M)): n_out = F D sums are finished, total =
// F D + L - D positions are touched, `held` of them start from an old partial sum.  Each fits 32 bits for every legal
// (M, L, D): group_frames(M) M + 32 M is 2^21 + 2^18 at most.
constexpr uint64_t group_bound(uint64_t M) { return group_frames(M) * M + kMaxTapsPerChannel * M; }
static_assert(group_bound(256) < ((uint64_t)1 << 32) && group_bound(512) < ((uint64_t)1 << 32) && group_bound(1024) < ((uint64_t)1 << 32) &&
                  group_bound(2048) < ((uint64_t)1 << 32) && group_bound(4096) < ((uint64_t)1 << 32) && group_bound(8192) < ((uint64_t)1 << 32),
              "a group's counts fit 32 bits");
static_assert(group_frames(8192) >= 1, "a group holds a frame");
struct Group {
    uint32_t F, n_out, total, held;
};
inline Group group(const State &s, uint32_t L, uint32_t D, size_t F) {
    return {(uint32_t)F, (uint32_t)(F * D), (uint32_t)(F * D + (L - D)), (uint32_t)s.held};
}
// the flush: no frames, the sums held are finished
inline Group flush_group(const State &s) { return {0u, (uint32_t)s.held, (uint32_t)s.held, (uint32_t)s.held}; }
// the position behind a group
inline State after_group(const State &s, uint32_t M, uint32_t L, uint32_t D, size_t F) { return {(uint64_t)(L - D), rot(s.rot, F, D, M), s.frame + F}; }

}  // namespace ppp
}  // namespace hz
