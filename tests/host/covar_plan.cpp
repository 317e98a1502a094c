// covar_plan.cpp -- the covariance bank's host arithmetic (csrc/hz_covar_plan.h) as a stand-alone program, built with
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_covar_plan.py, which checks the printed values against
// Python integers.
//
//   covar_plan <seed> <pushes>
// prints
//   "lds: N bytes rows tiles"              for every N: the LDS request of the segment kernel
//   "push: B consumed open n | ..."        random pushes from positions up to 2^62: the planner's counts
//   "flush: B open | ..."                  the flush of such a state
//   "tree: nseg hash"                      for every nseg <= 2^16: the shape the kernels' dealing and counters build
//   "covar_plan ok"
// and checks by itself: that the regions' items cover the segments of a push exactly once, in order, inside held ++ in;
// that every node of the tree joins two adjacent runs of segments, the earlier one on the left; that a block resumed at
// any segment builds the same tree; both operand layouts as bijections and the staged chunk's reads as free of bank
// conflicts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "hz_covar_plan.h"

using namespace hz;

static void fail(const char *what, unsigned long long a = 0, unsigned long long b = 0) {
    printf("FAILED: %s (%llu, %llu)\n", what, a, b);
    exit(1);
}

static uint64_t rng_state;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- a symbolic value: a run of segments and the shape of its tree ----------------------------------------------------
struct Sym {
    uint64_t hash;
    uint32_t lo, hi;
};
static uint64_t mix(uint64_t l, uint64_t r) { return (l * 0x9E3779B97F4A7C15ull) ^ (r + 0xBF58476D1CE4E5B9ull + (l << 7) + (l >> 3)); }
struct SymAdd {
    Sym operator()(Sym l, Sym r) const {
        if (l.hi != r.lo) fail("a node joins runs that are not adjacent, or in the wrong order", l.hi, r.lo);
        return Sym{mix(l.hash, r.hash), l.lo, r.hi};
    }
};
static Sym leaf(uint32_t s) { return Sym{1, s, s + 1}; }

// the segment kernel's item: a segment, or a group through the three-level counter in registers
static Sym item_node(const vp::Item &item) {
    if (item.count == 1) return leaf(item.seg);
    if (item.seg % vp::kGroup) fail("a group is not aligned", item.seg);
    // (every group has the shape of the first: past the first 4096 segments it is taken from there, to keep the run short)
    static uint64_t group_hash = 0;
    if (item.seg >= 4096 && group_hash) return Sym{group_hash, item.seg, item.seg + item.count};
    Sym s0{}, s1{}, s2{}, v{};
    for (uint32_t s = 0; s < item.count; s++) {
        v = leaf(item.seg + s);
        if (s & 1u) {
            v = SymAdd{}(s0, v);
            if (s & 2u) {
                v = SymAdd{}(s1, v);
                if (s & 4u)
                    v = SymAdd{}(s2, v);
                else
                    s2 = v;
            } else
                s1 = v;
        } else
            s0 = v;
    }
    if (!group_hash) group_hash = v.hash;
    if (v.hash != group_hash) fail("two groups of different shape", item.seg);
    return v;
}

// the walker over one block of a region: the counter goes in and comes out
static void walk(const vp::Region &r, Sym *col, uint32_t &count) {
    if (count != r.seg0) fail("the counter does not stand at the region's first segment", count, r.seg0);
    uint32_t it = 0;
    for (; it < r.head; it++) vp::covar_counter_push(col, count, item_node(vp::covar_item(r, it)), 0u, SymAdd{});
    for (uint32_t g = 0; g < r.groups;) {
        if (vp::covar_walk_many(count, vp::kGroupLog, r.groups - g)) {
            Sym v[vp::kWalk];
            for (uint32_t k = 0; k < vp::kWalk; k++) v[k] = item_node(vp::covar_item(r, it + k));
            for (uint32_t w = 1; w < vp::kWalk; w *= 2)
                for (uint32_t k = 0; k < vp::kWalk; k += 2 * w) v[k] = SymAdd{}(v[k], v[k + w]);
            vp::covar_counter_push(col, count, v[0], vp::kGroupLog + vp::kWalkLog, SymAdd{});
            g += vp::kWalk, it += vp::kWalk;
        } else {
            vp::covar_counter_push(col, count, item_node(vp::covar_item(r, it)), vp::kGroupLog, SymAdd{});
            g++, it++;
        }
    }
    for (uint32_t k = 0; k < r.tail; k++, it++) vp::covar_counter_push(col, count, item_node(vp::covar_item(r, it)), 0u, SymAdd{});
    if (count != r.seg1) fail("the counter does not end at the region's last segment", count, r.seg1);
}

// a block of nseg segments built in the pieces [0, c1), [c1, c2), ... -> the root
static Sym build(uint32_t nseg, const std::vector<uint32_t> &cuts) {
    Sym col[vp::kLevels + 1];
    uint32_t count = 0, at = 0;
    for (size_t k = 0; k <= cuts.size(); k++) {
        const uint32_t to = k < cuts.size() ? cuts[k] : nseg;
        vp::Region r{};
        r.seg0 = at, r.seg1 = to, r.blocks = 1, r.limit = nseg * vp::kSeg;
        vp::covar_deal(r);
        walk(r, col, count);
        at = to;
    }
    const Sym root = vp::covar_counter_collapse(col, count, SymAdd{});
    if (root.lo != 0 || root.hi != nseg) fail("the tree does not cover the block", root.lo, root.hi);
    return root;
}

// ---- the regions of a push against the stream -------------------------------------------------------------------------
// every segment of every region lies inside held ++ in, the regions follow each other without a gap, and with the held
// snapshots they account for all of V.  Blocks of a region are alike: one is walked, the count multiplies.
static void check_work(const vp::State &s, uint32_t B, const vp::Step &p, bool flush) {
    const vp::Work &w = p.w;
    unsigned __int128 covered = 0;
    uint64_t next_v = 0, nodes = 0, blocks = 0;
    for (uint32_t ri = 0; ri < w.regions; ri++) {
        const vp::Region &r = w.r[ri];
        if (r.head + r.groups * vp::kGroup + r.tail != r.seg1 - r.seg0 || r.items != r.head + r.groups + r.tail) fail("items do not cover the segments");
        if (r.node0 != nodes) fail("node slots", r.node0, nodes);
        if (r.v0 != next_v) fail("a gap between regions", r.v0, next_v);
        if (r.resume != (r.seg0 > 0) || (ri > 0 && r.seg0 != 0)) fail("resume");
        uint64_t per_block = 0;
        uint32_t seg = r.seg0;
        for (uint32_t it = 0; it < r.items; it++) {
            const vp::Item item = vp::covar_item(r, it);
            if (item.seg != seg) fail("items out of order", item.seg, seg);
            if (item.count == vp::kGroup && item.seg % vp::kGroup) fail("group alignment");
            for (uint32_t k = 0; k < item.count; k++) {
                const uint32_t len = vp::covar_seg_len(r, seg + k);
                if (len == 0 || len > vp::kSeg) fail("segment length", len);
                if (vp::covar_seg_start(r, 0, seg + k, B) != r.v0 + per_block) fail("segment start");
                if (len < vp::kSeg && !(r.complete && seg + k + 1 == r.seg1)) fail("a short segment inside a block");
                per_block += len;
            }
            seg += item.count;
        }
        const uint64_t span = r.complete && !flush ? (uint64_t)B - (uint64_t)r.seg0 * vp::kSeg : per_block;
        if (per_block != span) fail("a complete block's segments do not end at B", per_block, span);
        if (vp::covar_seg_start(r, r.blocks - 1, r.seg0, B) != r.v0 + (r.blocks - 1) * (uint64_t)B) fail("block pitch");
        covered += (unsigned __int128)per_block * r.blocks;
        next_v = r.v0 + (uint64_t)((unsigned __int128)per_block * r.blocks);
        nodes += r.items * r.blocks, blocks += r.blocks;
    }
    if (nodes != w.nodes || nodes != w.items || blocks != w.blocks) fail("totals");
    // regions may be absent where nothing completes (no finished segment): then everything is held
    if (covered + w.held_out != w.V) fail("the push is not accounted for", (unsigned long long)covered, w.V);
    if (w.held_in != s.open % vp::kSeg) fail("held_in");
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: covar_plan <seed> <pushes>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10);
    const int pushes = atoi(argv[2]);

    // ---- the tile ----
    for (uint32_t N = vp::kMinChannels; N <= vp::kMaxChannels; N++) {
        const uint32_t rows = vp::covar_rows(N), tiles = vp::covar_tiles(N), NF = vp::covar_node_floats(N);
        printf("lds: %u %u %u %u\n", N, vp::covar_lds_bytes(N), rows, tiles);
        if (rows < 2 * N) fail("rows");
        // the node: every entry (p, q) of the upper tiles has a slot of its own; the lower tile mirrors
        std::vector<int> seen(NF, 0);
        for (uint32_t p = 0; p < rows; p++)
            for (uint32_t q = 0; q < rows; q++) {
                const uint32_t e = vp::covar_node_index(p, q);
                if (e >= NF) fail("node index out of range", p, q);
                if ((p >> 4) > (q >> 4)) {
                    if (e != vp::covar_node_index(q, p)) fail("the lower tile does not mirror");
                    continue;
                }
                seen[e]++;
                // the slot is where the accumulator holds D[p][q]: lane = column + 16 * (row / 4), register = row % 4
                const uint32_t tile = e / vp::kTile, lane = (e % vp::kTile) / 4, reg = e % 4;
                if (vp::covar_tile_a(tile) + (lane >> 4) * 4 + reg != p || vp::covar_tile_b(tile) + (lane & 15u) != q) fail("node index against the D layout", p, q);
            }
        for (uint32_t e = 0; e < NF; e++)
            if (seen[e] != 1) fail("node index is no bijection", N, e);
        // the staged chunk: distinct addresses, and per half wave 32 different banks at every step
        std::vector<int> used(rows * vp::kPitch, 0);
        for (uint32_t row = 0; row < rows; row++)
            for (uint32_t n = 0; n < vp::kChunk; n++) {
                const uint32_t a = vp::covar_lds_index(row, n);
                if (a * 4 + 4 > vp::covar_lds_bytes(N) || used[a]++) fail("lds index", row, n);
            }
        for (uint32_t base = 0; base < rows; base += 16)
            for (uint32_t t = 0; t < vp::kChunk / 4; t++)
                for (uint32_t half = 0; half < 2; half++) {
                    uint32_t banks = 0;
                    for (uint32_t lane = half * 32; lane < half * 32 + 32; lane++) banks |= 1u << (vp::covar_lds_index(base + (lane & 15u), 4 * t + (lane >> 4)) % 32);
                    if (banks != 0xFFFFFFFFu) fail("bank conflict", base, t);
                }
    }

    // ---- the counts ----
    for (int k = 0; k < pushes; k++) {
        uint32_t B;
        switch (rnd() % 4) {
        case 0: B = 1 + (uint32_t)(rnd() % 600); break;
        case 1: B = vp::kSeg * (1 + (uint32_t)(rnd() % 64)) + (uint32_t)(rnd() % 3) - 1; break;
        case 2: B = 1 + (uint32_t)(rnd() % vp::kMaxBlock); break;
        default: B = vp::kMaxBlock - (uint32_t)(rnd() % 3); break;
        }
        vp::State s;
        s.consumed = rnd() >> (2 + rnd() % 62);  // up to 2^62
        s.block = s.consumed / B, s.open = (uint32_t)(s.consumed % B);
        uint64_t n;
        switch (rnd() % 4) {
        case 0: n = rnd() % 1000; break;
        case 1: n = rnd() % (4ull * B + 1); break;
        case 2: n = rnd() >> (2 + rnd() % 62); break;
        default: n = vp::kPushMax - rnd() % 2; break;
        }
        if (s.consumed + n > vp::kPushMax) n = vp::kPushMax - s.consumed;
        const vp::Step p = vp::covar_step(s, B, n);
        if (!p.ok) fail("a push inside the range was refused");
        check_work(s, B, p, false);
        printf("push: %u %llu %u %llu | %llu %llu %llu %u %llu %llu %llu %llu %u\n", B, (unsigned long long)s.consumed, s.open, (unsigned long long)n,
               (unsigned long long)p.w.written, (unsigned long long)p.next.consumed, (unsigned long long)p.next.block, p.next.open,
               (unsigned long long)p.w.held_in, (unsigned long long)p.w.held_out, (unsigned long long)p.w.V, (unsigned long long)p.w.items, p.w.keep);
        const vp::Step f = vp::covar_flush(s);
        check_work(s, B, f, true);
        printf("flush: %u %u | %llu %llu %llu %llu\n", B, s.open, (unsigned long long)f.w.written, (unsigned long long)f.w.items,
               (unsigned long long)f.w.held_in, (unsigned long long)f.next.consumed);
    }
    if (vp::covar_step(vp::State{}, 1, vp::kPushMax + 1).ok) fail("a push above the range was accepted");

    // ---- the tree ----
    for (uint32_t nseg = 1; nseg <= (1u << 16); nseg++) {
        const Sym whole = build(nseg, {});
        printf("tree: %u %llu\n", nseg, (unsigned long long)whole.hash);
        // resumed once or twice at random segments: the same tree (every nseg up to 4096, every 61st above)
        if (nseg > 4096 && nseg % 61) continue;
        std::vector<uint32_t> cuts;
        if (nseg > 1) cuts.push_back(1 + (uint32_t)(rnd() % (nseg - 1)));
        if (nseg > 2 && rnd() % 2) {
            const uint32_t c = 1 + (uint32_t)(rnd() % (nseg - 1));
            if (c > cuts[0]) cuts.push_back(c);
            if (c < cuts[0]) cuts.insert(cuts.begin(), c);
        }
        if (build(nseg, cuts).hash != whole.hash) fail("a resumed block builds another tree", nseg);
    }
    printf("covar_plan ok\n");
    return 0;
}
