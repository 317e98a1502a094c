// hz_covar_plan.h -- the host arithmetic of the covariance bank (include/hzsdr_covar.h), HIP-free so that
// tests/host/covar_plan.cpp can run it under the sanitizers and tests/host/covar_ref.cpp can transcribe the kernels'
// indexing from the same functions.  Everything that can overflow lives here.
//
// The stream position is three running values: the snapshots consumed per row, the index of the open block and the
// snapshots the open block holds (below B).  Out of the last come the finished segments of the open block (open / 256:
// the binary counter of the tree, whose set bits say which levels of the bank's stack of group sums are in use) and
// the raw snapshots of the open segment (open % 256: kept converted on the device).
//
// A push is cut into at most three regions of blocks that all look alike: the rest of the open block, the whole blocks
// behind it, and the new open block.  Inside a block of a region the segments [seg0, seg1) are dealt out as items: head
// segments one by one up to the next multiple of kGroup, then aligned groups of kGroup segments, then the segments
// left one by one.  One wave computes one item -- a segment is 64 steps of v_mfma_f32_16x16x4_f32 per accumulator
// tile, a group is the balanced tree over its kGroup segments, held in registers -- and writes one node: 256 floats
// per tile, in accumulator order.  The second kernel gives one workgroup to every block of a region and walks its
// nodes in order through the binary counter (levels 0 or log2 kGroup; sixteen aligned group nodes at a time as one
// balanced tree), then collapses the counter from the smallest group upward, combines and writes R -- or, for the new
// open block, leaves the counter in the bank's stack.  The stack is two buffers: a push reads one and writes the other
// (Work::keep says that it wrote), because the workgroup that closes the resumed block and the one that leaves the new
// open block run side by side in one launch and may use the same levels.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_covar_math.h"

namespace hz {
namespace vp {

constexpr uint32_t kMinChannels = 2, kMaxChannels = 16;
constexpr uint32_t kMaxBlock = 1u << 24;
constexpr uint32_t kSeg = 256;          // snapshots of a segment
constexpr uint32_t kChunk = 128;        // snapshots staged in LDS at once: half a segment
constexpr uint32_t kPitch = kChunk + 2; // floats of one row of the staged chunk: 2 mod 32, see covar_lds_index
constexpr uint32_t kGroup = 8, kGroupLog = 3;  // segments of one wave's group
constexpr uint32_t kWalk = 16, kWalkLog = 4;   // group nodes the walker takes at once
constexpr uint32_t kLevels = 17;        // a block has at most 2^16 segments: counter bits 0 .. 16
constexpr uint32_t kTile = 256;         // floats of one 16 x 16 accumulator tile
constexpr int kSegThreads = 64, kWalkThreads = 256;
constexpr uint64_t kPushMax = (uint64_t)1 << 62;  // snapshots of one push: every position stays below 2^63
constexpr uint32_t kLdsBudget = 66 * 1024;        // a workgroup's LDS budget (hz_tuner_plan.h's)
// snapshots per row of one launch round: bounds the node scratch (a push longer than this is cut, which the contract
// allows: the bits do not depend on the cut)
constexpr uint64_t kRoundSegments = 8192;

// ---- the tile --------------------------------------------------------------------------------------------
// rows of V: 2N rounded up to whole accumulator tiles
HZ_HD uint32_t covar_rows(uint32_t N) { return N <= 8 ? 16u : 32u; }
// accumulator tiles: (0,0) alone, or (0,0), (0,1), (1,1)
HZ_HD uint32_t covar_tiles(uint32_t N) { return N <= 8 ? 1u : 3u; }
HZ_HD uint32_t covar_node_floats(uint32_t N) { return covar_tiles(N) * kTile; }
HZ_HD uint32_t covar_lds_bytes(uint32_t N) { return covar_rows(N) * kPitch * 4u; }
// Element (row, n) of the staged chunk.  Lane l of the matrix instruction's A operand holds V[l & 15][4 t + (l >> 4)],
// and B = V^T wants the same element: one register serves both.  ds_read_b32 serves lanes 0 .. 31 and 32 .. 63 apart and
// its banks are the address modulo 32 floats: with a pitch of 2 mod 32 the 16 rows x 2 k-slots of a half wave fall on 32
// different banks.  The staging stores are consecutive floats of one row.
HZ_HD uint32_t covar_lds_index(uint32_t row, uint32_t n) { return row * kPitch + n; }
// Entry (p, q) of the Gram matrix inside a node.  An accumulator tile in D order is lane * 4 + reg with column lane & 15
// and row (lane >> 4) * 4 + reg; tile 0 is rows and columns 0 .. 15, tile 1 rows 0 .. 15 of columns 16 .. 31, tile 2 rows
// and columns 16 .. 31.  The lower tile is never computed: G is symmetric bit for bit (a product commutes), so (p, q)
// there is read as (q, p).
HZ_HD uint32_t covar_node_index(uint32_t p, uint32_t q) {
    if ((p >> 4) > (q >> 4)) {
        const uint32_t s = p;
        p = q, q = s;
    }
    const uint32_t tile = (p >> 4) + (q >> 4);
    const uint32_t lane = (q & 15u) + 16u * ((p & 15u) >> 2);
    return tile * kTile + lane * 4u + (p & 3u);
}
// the rows of V a tile's A and B operands come from: tile -> (first row of A, first row of B)
HZ_HD uint32_t covar_tile_a(uint32_t tile) { return tile == 2 ? 16u : 0u; }
HZ_HD uint32_t covar_tile_b(uint32_t tile) { return tile == 0 ? 0u : 16u; }

// ---- the counts --------------------------------------------------------------------------------------------
struct State {
    uint64_t consumed = 0;  // snapshots per row since create or reset
    uint64_t block = 0;     // index of the open block
    uint32_t open = 0;      // snapshots the open block holds, below B
};

// blocks of like shape: in each, segments [seg0, seg1) of the block are computed
struct Region {
    uint64_t v0;      // position, in held ++ in, of block-relative snapshot 256 seg0 of the region's first block
    uint64_t blocks;  // blocks of the region, B snapshots apart
    uint64_t node0;   // the region's first node
    uint64_t out0;    // the push's index of the region's first block (complete regions)
    uint32_t seg0, seg1;
    uint32_t limit;   // snapshots of the block that are present: segment s holds min(256, limit - 256 s) of them
    uint32_t head, groups, tail, items;  // items of one block: head + groups + tail
    uint32_t complete;  // the block ends in this push (or flush): collapse, combine, write
    uint32_t resume;    // the bank's stack comes in (seg0 > 0)
};

struct Work {
    Region r[3];
    uint32_t regions;
    uint64_t items, blocks, nodes;  // over all regions (nodes == items)
    uint64_t held_in, held_out;     // raw snapshots of the open segment before and after
    uint64_t V;                     // held_in + n
    uint64_t written;               // blocks the push writes
    uint32_t keep;                  // the last region leaves its counter in the bank's stack
};

struct Step {
    bool ok;
    Work w;
    State next;
};

HZ_HD uint32_t covar_block_segments(uint32_t B) { return (B + kSeg - 1) / kSeg; }

inline void covar_deal(Region &r) {
    const uint32_t up = (r.seg0 + kGroup - 1) / kGroup * kGroup;
    const uint32_t hend = up < r.seg1 ? up : r.seg1;
    r.head = hend - r.seg0;
    r.groups = (r.seg1 - hend) / kGroup;
    r.tail = r.seg1 - hend - r.groups * kGroup;
    r.items = r.head + r.groups + r.tail;
}

inline void covar_add_region(Work &w, Region r) {
    covar_deal(r);
    if (!r.complete && r.items == 0) return;  // (nothing to compute, nothing to write: the stack stays as it is)
    r.node0 = w.nodes;
    w.r[w.regions++] = r;
    w.items += r.blocks * r.items;
    w.nodes = w.items;
    w.blocks += r.blocks;
}

// a push of n snapshots per row
inline Step covar_step(const State &s, uint32_t B, uint64_t n) {
    Step p{};
    if (n > kPushMax || s.consumed > kPushMax) return p;
    p.ok = true;
    Work &w = p.w;
    const uint32_t q0 = s.open / kSeg, spb = covar_block_segments(B);
    w.held_in = s.open % kSeg;
    w.V = w.held_in + n;
    const uint64_t total = (uint64_t)s.open + n;  // snapshots of the open block and behind it
    const uint64_t done = total / B;
    const uint32_t open = (uint32_t)(total - done * B);
    w.written = done;
    if (done == 0) {
        Region r{};
        r.v0 = 0, r.blocks = 1, r.seg0 = q0, r.seg1 = open / kSeg, r.limit = B, r.resume = q0 > 0;
        covar_add_region(w, r);
    } else {
        Region a{};
        a.v0 = 0, a.blocks = 1, a.seg0 = q0, a.seg1 = spb, a.limit = B, a.complete = 1, a.resume = q0 > 0, a.out0 = 0;
        covar_add_region(w, a);
        const uint64_t first = (uint64_t)B - (uint64_t)q0 * kSeg;  // snapshots of held ++ in that the first block takes
        if (done > 1) {
            Region m{};
            m.v0 = first, m.blocks = done - 1, m.seg0 = 0, m.seg1 = spb, m.limit = B, m.complete = 1, m.out0 = 1;
            covar_add_region(w, m);
        }
        Region z{};
        z.v0 = first + (done - 1) * B, z.blocks = 1, z.seg0 = 0, z.seg1 = open / kSeg, z.limit = B;
        covar_add_region(w, z);
    }
    w.keep = w.regions && !w.r[w.regions - 1].complete;
    w.held_out = open % kSeg;
    p.next.consumed = s.consumed + n;
    p.next.block = s.block + done;
    p.next.open = open;
    return p;
}

// the flush: the open block with the snapshots present, no input
inline Step covar_flush(const State &s) {
    Step p{};
    p.ok = true;
    Work &w = p.w;
    w.held_in = s.open % kSeg;
    w.V = w.held_in;
    if (s.open) {
        Region r{};
        r.v0 = 0, r.blocks = 1, r.seg0 = s.open / kSeg, r.seg1 = covar_block_segments(s.open), r.limit = s.open, r.complete = 1;
        r.resume = r.seg0 > 0;
        covar_add_region(w, r);
        w.written = 1;
    }
    p.next = State{};
    return p;
}

// item `it` of a block of region r -> its first segment, its segments (1 or kGroup) and its level in the counter
struct Item {
    uint32_t seg, count, level;
};
HZ_HD Item covar_item(const Region &r, uint32_t it) {
    if (it < r.head) return Item{r.seg0 + it, 1u, 0u};
    it -= r.head;
    if (it < r.groups) return Item{r.seg0 + r.head + it * kGroup, kGroup, kGroupLog};
    it -= r.groups;
    return Item{r.seg0 + r.head + r.groups * kGroup + it, 1u, 0u};
}
// snapshots of segment `seg` that are present in a block of region r
HZ_HD uint32_t covar_seg_len(const Region &r, uint32_t seg) {
    const uint32_t at = seg * kSeg;
    if (at >= r.limit) return 0;
    return r.limit - at < kSeg ? r.limit - at : kSeg;
}
// position in held ++ in of the first snapshot of segment `seg` of block `blk` of region r
HZ_HD uint64_t covar_seg_start(const Region &r, uint64_t blk, uint32_t seg, uint32_t B) {
    return r.v0 + blk * B + (uint64_t)(seg - r.seg0) * kSeg;
}

// ---- the tree ----------------------------------------------------------------------------------------------
// The binary counter over one value; Add is the node.  `count` counts segments; a value of 2^level segments goes in
// where count is a multiple of 2^level.
// (`stack` is anything indexed by level: an array, or a lane's column of LDS)
template <class S, class T, class Add>
HZ_HD void covar_counter_push(S &&stack, uint32_t &count, T v, uint32_t level, Add add) {
    uint32_t c = count >> level, l = level;
    while (c & 1u) {
        v = add(stack[l], v);
        l++, c >>= 1;
    }
    stack[l] = v;
    count += 1u << level;
}
// the remainder collapses from the smallest group upward; count > 0
template <class S, class Add>
HZ_HD auto covar_counter_collapse(S &&stack, uint32_t count, Add add) {
    uint32_t l = 0;
    while (!((count >> l) & 1u)) l++;
    auto acc = stack[l];
    for (l++; (count >> l) != 0; l++)
        if ((count >> l) & 1u) acc = add(stack[l], acc);
    return acc;
}
// the walker may take kWalk group nodes at once where the counter is aligned to them
HZ_HD bool covar_walk_many(uint32_t count, uint32_t level, uint32_t left) {
    return level == kGroupLog && left >= kWalk && (count & ((kGroup * kWalk) - 1u)) == 0;
}

// samples per row of one launch round for block length B
inline uint64_t covar_round(uint32_t B) { return kRoundSegments * (B < kSeg ? B : kSeg); }

}  // namespace vp
}  // namespace hz
