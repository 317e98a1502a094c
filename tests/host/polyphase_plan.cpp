// polyphase_plan.cpp -- the host arithmetic the polyphase banks share (csrc/hz_polyphase_plan.h) as a stand-alone program
// for the sanitizers (tests/test_polyphase_plan.py builds it with -fsanitize=address,undefined).
//
//   polyphase_plan SEED STREAMS
//
//   1. For STREAMS random streams of random (M, P, D) -- M a power of two from 256 to 8192 (the channelizer's and the
//      synthesis bank's range) or any M from 2 to 255 (the channel bank's), P from 1 to 32, D from 1 to M -- from random
//      positions: the counts of every push against the closed form in 128-bit integers, the rotation of a frame inside
//      the push, and the last sample a frame's fold loads against the virtual buffer.  The pushes: 0, 1, L - 1, L,
//      L + D - 1, L + D, random lengths, around 2^62 (the largest push) and near ~0.
//   2. For every power of two M from 256 to 8192: rot and pos equal the `& (M - 1)` forms of the transform kernels, and
//      for every M of either range pos is a permutation with position 0 at -floor(M / 2).
//   3. The argument check under each bank's rule for M: every refusal fires alone, and of two faults the earlier wins.
//   4. The synthesis bank's counts of one group at every legal corner: below 2^32, and equal to the 128-bit closed form;
//      group_frames at least 1; the scratch grows to the group and no further; a stream of groups walks the rotation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_polyphase_plan.h"

using namespace hz;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (fails++ < 20) {                  \
                fprintf(stdout, "FAIL %s: ", #cond); \
                fprintf(stdout, __VA_ARGS__);    \
                fprintf(stdout, "\n");           \
            }                                    \
        }                                        \
    } while (0)

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static u128 frames_after(u128 n, uint32_t L, uint32_t D) { return n >= L ? (n - L) / D + 1 : 0; }

static uint32_t pick_channels(int index) {
    if (index % 2) return 2 + (uint32_t)below(254);
    return 256u << below(6);
}

// ---- 1. the streams -----------------------------------------------------------------------------------------
static size_t too_long_seen = 0, pushes_seen = 0;

static void check_stream(int index) {
    const uint32_t M = pick_channels(index);
    const uint32_t pick_p[] = {1, 2, 32, 1 + (uint32_t)below(32)}, P = pick_p[below(4)];
    const uint32_t pick_d[] = {1, M, 1 + (uint32_t)below(M)}, D = pick_d[below(3)];
    const uint32_t L = P * M;
    ppp::State st{};
    u128 N = 0;  // samples pushed so far
    for (int push = 0; push < 16; push++) {
        const uint64_t pick_n[] = {0, 1, below(10), below(3 * (uint64_t)L + 1), below(100000), L - 1, L, (uint64_t)L + D - 1, (uint64_t)L + D,
                                   below((uint64_t)1 << 33), below((uint64_t)1 << 52),
                                   ((uint64_t)1 << 62) - below(3), ((uint64_t)1 << 62) + 1 + below(1000), ~(uint64_t)0 - below(3)};
        const uint64_t n = pick_n[index % 4 < 2 ? below(14) : below(9)];
        const ppp::Step p = ppp::step(st, M, L, D, n);
        CHECK(p.ok == (n <= ppp::kPushMax), "push of %llu", (unsigned long long)n);
        if (!p.ok) {
            too_long_seen++;
            continue;
        }
        pushes_seen++;
        const u128 f0 = frames_after(N, L, D), f1 = frames_after(N + n, L, D);
        CHECK((u128)p.F == f1 - f0 && (u128)p.V == (u128)st.held + n, "M=%u P=%u D=%u: frames of a push", M, P, D);
        CHECK((u128)p.next.held == N + n - f1 * D && p.next.held < L, "M=%u P=%u D=%u: held %llu", M, P, D, (unsigned long long)p.next.held);
        CHECK((u128)p.next.rot == f1 * D % M, "M=%u P=%u D=%u: rotation", M, P, D);
        CHECK((u128)p.next.frame == (f1 & (u128) ~(uint64_t)0), "M=%u P=%u D=%u: frame index", M, P, D);
        // a frame inside the push: its rotation, and the loads of its fold inside held ++ in
        if (p.F) {
            const uint64_t pick_f[] = {0, p.F - 1, below(p.F)};
            for (uint64_t f : pick_f) {
                CHECK(ppp::rot(st.rot, f, D, M) == (uint32_t)((u128)(st.rot + (u128)f * D) % M), "rotation of frame %llu", (unsigned long long)f);
                CHECK((u128)ppp::rot(st.rot, f, D, M) == (f0 + f) * D % M, "rotation against the stream position");
                const u128 last = (u128)f * D + (M - 1) + (u128)(P - 1) * M;
                CHECK(last < p.V && last < ((u128)1 << 63), "the last sample of frame %llu", (unsigned long long)f);
            }
        }
        st = p.next;
        N += n;
    }
}

// the named pushes, each from the start of a stream and each behind a held sample, at the corners of every M
static void check_named_pushes(uint32_t M) {
    for (uint32_t P : {1u, 2u, 32u})
        for (uint32_t D : {1u, M / 2 ? M / 2 : 1u, M}) {
            const uint32_t L = P * M;
            const uint64_t ns[] = {0, 1, L - 1, L, (uint64_t)L + D - 1, (uint64_t)L + D, ppp::kPushMax - 1, ppp::kPushMax, ppp::kPushMax + 1, ~(uint64_t)0};
            for (uint64_t held : {(uint64_t)0, (uint64_t)1, (uint64_t)L - 1})
                for (uint64_t n : ns) {
                    const ppp::State st{held, (uint32_t)(held % M), 7};
                    const ppp::Step p = ppp::step(st, M, L, D, n);
                    CHECK(p.ok == (n <= ppp::kPushMax), "M=%u n=%llu", M, (unsigned long long)n);
                    if (!p.ok) continue;
                    const u128 V = (u128)held + n, F = frames_after(V, L, D);
                    CHECK((u128)p.V == V && (u128)p.F == F && (u128)p.next.held == V - F * D && p.next.held < L, "M=%u P=%u D=%u n=%llu", M, P, D, (unsigned long long)n);
                    CHECK((u128)p.next.rot == (held + F * D) % M && (u128)p.next.frame == 7 + F, "M=%u P=%u D=%u n=%llu: position", M, P, D, (unsigned long long)n);
                }
        }
}

// ---- 2. the general forms against the transform kernels' ---------------------------------------------------------
static void check_pow2_forms(uint32_t M) {
    for (uint32_t k = 0; k < M; k++) {
        CHECK(ppp::pos(k, M, false) == k, "M=%u", M);
        CHECK(ppp::pos(k, M, true) == ((k + M / 2) & (M - 1)), "M=%u pos(%u)", M, k);
    }
    for (int i = 0; i < 4000; i++) {
        const uint32_t r = (uint32_t)below(M), D = 1 + (uint32_t)below(M);
        const uint64_t pick_f[] = {below(10), below(M), below((uint64_t)1 << 40), ppp::kPushMax - below(3), ~(uint64_t)0 - below(3)};
        const uint64_t f = pick_f[below(5)];
        CHECK(ppp::rot(r, f, D, M) == ((r + (f & (M - 1)) * D) & (M - 1)), "M=%u rot(%u, %llu, %u)", M, r, (unsigned long long)f, D);
    }
    // the corners of the reduction: the largest rotation, frame count and hop
    CHECK(ppp::rot(M - 1, M - 1, M, M) == ((M - 1 + (uint64_t)(M - 1) * M) & (M - 1)), "M=%u", M);
    CHECK(ppp::rot(M - 1, ~(uint64_t)0, M - 1, M) == ((M - 1 + ((~(uint64_t)0) & (M - 1)) * (M - 1)) & (M - 1)), "M=%u", M);
}

static void check_pos(uint32_t M) {
    std::vector<uint8_t> seen(M, 0);
    for (uint32_t k = 0; k < M; k++) {
        CHECK(ppp::pos(k, M, false) == k, "M=%u", M);
        const uint32_t p = ppp::pos(k, M, true);
        CHECK(p < M && p == (k + M / 2) % M, "M=%u pos(%u) = %u", M, k, p);
        if (p < M) seen[p]++;
        // ascending signed frequency: position p holds the signed channel p - floor(M / 2)
        const int signed_k = k > (M - 1) / 2 ? (int)k - (int)M : (int)k;
        CHECK((int)p - (int)(M / 2) == signed_k, "M=%u: channel %u at position %u", M, k, p);
    }
    for (uint32_t k = 0; k < M; k++) CHECK(seen[k] == 1, "M=%u", M);
}

// ---- 3. the argument check ------------------------------------------------------------------------------------
struct Args {
    size_t m;
    bool has_taps;
    size_t n_taps, hop;
    int order, layout;
};
static ppp::Refusal run(const ppp::ChannelRule &r, const Args &a) { return ppp::check_args(r, a.m, a.has_taps, a.n_taps, a.hop, a.order, a.layout); }

struct Fault {
    ppp::Refusal want;
    void (*plant)(Args &, const ppp::ChannelRule &);
};
static size_t refusals_seen = 0, pairs_seen = 0;

static void check_refusals(const ppp::ChannelRule &r, size_t good_m) {
    // in the order of precedence; several ways to each refusal
    const std::vector<Fault> faults = {
        {ppp::kBadChannels, [](Args &a, const ppp::ChannelRule &q) { a.m = q.lo - 1; }},
        {ppp::kBadChannels, [](Args &a, const ppp::ChannelRule &q) { a.m = q.hi + 1; }},
        {ppp::kBadChannels, [](Args &a, const ppp::ChannelRule &) { a.m = 0; }},
        {ppp::kNullTaps, [](Args &a, const ppp::ChannelRule &) { a.has_taps = false; }},
        {ppp::kBadTaps, [](Args &a, const ppp::ChannelRule &) { a.n_taps = 0; }},
        {ppp::kBadTaps, [](Args &a, const ppp::ChannelRule &) { a.n_taps += 1; }},
        {ppp::kBadTaps, [](Args &a, const ppp::ChannelRule &) { a.n_taps = 33 * a.n_taps / 2; }},
        {ppp::kBadHop, [](Args &a, const ppp::ChannelRule &) { a.hop = 0; }},
        {ppp::kBadHop, [](Args &a, const ppp::ChannelRule &) { a.hop = ~(size_t)0; }},
        {ppp::kBadOrder, [](Args &a, const ppp::ChannelRule &) { a.order = 2; }},
        {ppp::kBadOrder, [](Args &a, const ppp::ChannelRule &) { a.order = -1; }},
        {ppp::kBadLayout, [](Args &a, const ppp::ChannelRule &) { a.layout = 2; }},
        {ppp::kBadLayout, [](Args &a, const ppp::ChannelRule &) { a.layout = -1; }},
    };
    const Args good{good_m, true, 2 * good_m, good_m, ppp::kOrderNegativeFirst, ppp::kChannelMajor};
    CHECK(run(r, good) == ppp::kArgsOk, "m=%zu", good_m);
    for (size_t i = 0; i < faults.size(); i++) {
        Args a = good;
        faults[i].plant(a, r);
        CHECK(run(r, a) == faults[i].want, "m=%zu fault %zu alone", good_m, i);
        refusals_seen++;
        for (size_t j = 0; j < faults.size(); j++) {
            if (faults[j].want == faults[i].want) continue;
            Args b = good;
            // (planted in either order of time: the order of precedence decides)
            if (j < i) faults[j].plant(b, r), faults[i].plant(b, r);
            else faults[i].plant(b, r), faults[j].plant(b, r);
            const ppp::Refusal first = faults[i].want < faults[j].want ? faults[i].want : faults[j].want;
            CHECK(run(r, b) == first, "m=%zu faults %zu and %zu", good_m, i, j);
            pairs_seen++;
        }
    }
    // the limits themselves are legal
    for (size_t m : {r.lo, r.hi}) {
        for (size_t P : {(size_t)1, (size_t)32})
            for (size_t D : {(size_t)1, m}) CHECK(run(r, Args{m, true, P * m, D, ppp::kOrderZeroFirst, ppp::kFrameMajor}) == ppp::kArgsOk, "m=%zu", m);
        CHECK(run(r, Args{m, true, 33 * m, 1, 0, 0}) == ppp::kBadTaps && run(r, Args{m, true, m, m + 1, 0, 0}) == ppp::kBadHop, "m=%zu", m);
    }
    if (r.pow2) {
        for (size_t m = r.lo; m <= r.hi; m++) CHECK((run(r, Args{m, true, m, m, 0, 0}) == ppp::kArgsOk) == ((m & (m - 1)) == 0), "m=%zu", m);
    } else {
        for (size_t m = r.lo; m <= r.hi; m++) CHECK(run(r, Args{m, true, m, m, 0, 0}) == ppp::kArgsOk, "m=%zu", m);
    }
}

// ---- 4. the synthesis bank's groups -----------------------------------------------------------------------------
static size_t largest_total = 0;

static void check_groups(uint32_t M) {
    const size_t G = ppp::group_frames(M);
    CHECK(G >= 1 && G * M * 8 <= ppp::kSynthScratchBytes && (G + 1) * M * 8 > ppp::kSynthScratchBytes, "M=%u group %zu", M, G);
    CHECK(ppp::scratch_frames(0, M) == 0 && ppp::scratch_frames(1, M) == 1 && ppp::scratch_frames(G, M) == G && ppp::scratch_frames(G + 1, M) == G &&
              ppp::scratch_frames(~(size_t)0, M) == G,
          "M=%u scratch", M);
    const u128 lim = (u128)1 << 32;
    for (uint32_t P : {1u, 2u, 31u, 32u})
        for (uint32_t D : {1u, 2u, M / 2, M - 1, M}) {
            const uint32_t L = P * M;
            for (size_t F : {(size_t)1, (size_t)2, G - 1 ? G - 1 : 1, G})
                for (uint64_t held : {(uint64_t)0, (uint64_t)(L - D)}) {
                    const ppp::State st{held, (uint32_t)below(M), below((uint64_t)1 << 50)};
                    const u128 n_out = (u128)F * D, total = n_out + L - D;
                    CHECK(n_out < lim && total < lim && held < lim && (u128)F < lim, "M=%u P=%u D=%u F=%zu: a count beyond 32 bits", M, P, D, F);
                    const ppp::Group g = ppp::group(st, L, D, F);
                    CHECK(g.F == F && (u128)g.n_out == n_out && (u128)g.total == total && g.held == held, "M=%u P=%u D=%u F=%zu", M, P, D, F);
                    CHECK(g.held <= g.total && g.n_out <= g.total && g.total - g.n_out == L - D, "M=%u P=%u D=%u F=%zu: the sums held", M, P, D, F);
                    if ((size_t)total > largest_total) largest_total = (size_t)total;
                    const ppp::State nx = ppp::after_group(st, M, L, D, F);
                    CHECK(nx.held == L - D && nx.frame == st.frame + F && (u128)nx.rot == ((u128)st.rot + (u128)F * D) % M, "M=%u P=%u D=%u F=%zu: behind a group", M, P, D, F);
                    const ppp::Group fl = ppp::flush_group(nx);
                    CHECK(fl.F == 0 && fl.n_out == L - D && fl.total == L - D && fl.held == L - D, "M=%u P=%u D=%u: the flush", M, P, D);
                }
        }
    CHECK(ppp::group_bound(M) < lim, "M=%u", M);
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: polyphase_plan SEED STREAMS\n");
        return 64;
    }
    rng_state = strtoull(argv[1], nullptr, 10);
    const int streams = atoi(argv[2]);
    for (int i = 0; i < streams; i++) check_stream(i);
    for (uint32_t M = 2; M <= 255; M++) check_named_pushes(M), check_pos(M);
    for (uint32_t M = 256; M <= 8192; M *= 2) check_named_pushes(M), check_pos(M), check_pow2_forms(M), check_groups(M);
    for (size_t m : {(size_t)256, (size_t)1024, (size_t)8192}) check_refusals(ppp::kTransformRule, m);
    for (size_t m : {(size_t)2, (size_t)3, (size_t)100, (size_t)255}) check_refusals(ppp::kMatrixRule, m);
    printf("pushes: %zu\n", pushes_seen);
    printf("too long: %zu\n", too_long_seen);
    printf("refusals: %zu %zu\n", refusals_seen, pairs_seen);
    printf("largest group total: %zu\n", largest_total);
    if (fails) {
        printf("polyphase_plan: %d check(s) failed\n", fails);
        return 1;
    }
    printf("polyphase_plan ok\n");
    return 0;
}
