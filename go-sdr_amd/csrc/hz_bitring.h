// hz_bitring.h -- the device side of the bit-ring banks (hz_framesync.hip, hz_hdlc.hip): what a kernel of the shape "a
// workgroup is ONE wave, it owns a row for the whole push, lane = float, the row's decided bits go by in a ring of
// 64-bit words in the wave's own LDS" is made of, apart from what it looks for in the ring.  The bits, the ring and the
// reasons for the shape are hz_bitring_plan.h; the host side of the banks' objects is hz_framebank.h.
//
// Time goes by in tiles of 64 floats, one coalesced 256-byte load each, kChunk tiles' loads in flight in registers
// while the chunk before them is worked on.  A kernel is
//     Row w = open_row(...);                the count clamped, the state's common words, the history into the ring
//     fetch(cur, ...);
//     for each chunk of kChunk tiles:
//         fetch(nxt, ...);                  the next chunk's loads
//         chunk_words(...);                 this chunk's words into the ring
//         for each tile of the chunk: ...   the bank's own work, lane = the tile's bit
//         rotate(cur, nxt);
//     close_row(...);                       the ring re-aligned into the history, the common words, the counts
// The loop stays WRITTEN OUT in each kernel over these leaves, as in hz_rowwave.h.  As one template over a per-tile
// callable (for_tiles(a, ring, in, m, carry, lane, [&](t, tn) { ... })) the frame sync kernel compiled to 126 VGPRs and
// 20 bytes of scratch a lane (a stack slot of its scalar spills that the compiler did not get back into registers)
// where the written-out loop has 121 / 123 VGPRs and none, as the kernel had before this header;
// profiles/bitring_time.txt has the resource table of both forms and the times of the one kept.
#pragma once
#include "hz_bitring_plan.h"
#include "hz_framesync_math.h"
#include "hz_rowwave.h"

namespace hz {
namespace br {

// the leading part of both kernels' arguments
struct RowArgs {
    const uint32_t *in;  // the rows' floats as their bit patterns; row r starts r * in_stride floats in
    size_t in_stride;
    uint64_t n;  // symbols a row may hold in the push
    const uint32_t *in_counts;
    uint8_t *out;
    size_t out_stride;  // bytes
    uint64_t *positions;
    uint32_t *info, *counts;
    uint32_t cap;
    uint64_t *state;  // R rows of `per` words: the bits consumed, the bank's own words, the last raw decision, HW of history
    uint32_t *maxc;
    uint32_t R, G;
    uint32_t HW, RW, per;
    uint32_t step;  // floats from one decision's float to the next: 2 on complex rows read Re only
    uint32_t diff;
};

// kChunk tiles of a row from tile t0 on into registers: lane = float
__device__ __forceinline__ void fetch(uint32_t (&raw)[kChunk], const uint32_t *in, uint32_t step, uint32_t t0, uint32_t m, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < kChunk; k++) {
        const uint64_t bit = (uint64_t)(t0 + k) * kTileBits + lane;
        if (bit < m) raw[k] = in[bit * step];
    }
}

// the 64 ring bits from ring bit `bit` on
__device__ __forceinline__ uint64_t ring_bits(const uint64_t *ring, uint64_t bit, uint32_t RW) {
    const uint32_t w = (uint32_t)(bit >> 6);
    return fm::funnel(ring[ring_slot(w, RW)], ring[ring_slot(w + 1, RW)], (uint32_t)bit & 63u);
}

__device__ __forceinline__ uint32_t tiles_of(uint32_t m) { return m / kTileBits + (m % kTileBits ? 1u : 0u); }
// the bits of tile t that the push consumes
__device__ __forceinline__ uint32_t tile_bits(uint32_t t, uint32_t m) {
    const uint32_t left = m - t * kTileBits;
    return left < kTileBits ? left : kTileBits;
}

struct Row {
    uint64_t *z;         // the row's state
    const uint32_t *in;  // the row's floats
    uint32_t m;          // the bits this push consumes (n is below 2^31)
    uint64_t bits0;      // the bits consumed before it
    uint32_t carry;      // the last raw decision
};

// The row's opening: the count clamped, the common state words read, the history copied into the ring.  bits: per
// symbol; last_at, hist_at: where the state keeps the last raw decision and the history's first word.
__device__ __forceinline__ Row open_row(const RowArgs &a, uint64_t *ring, size_t row, uint32_t bits, uint32_t last_at, uint32_t hist_at, uint32_t lane) {
    uint64_t cnt = a.in_counts ? a.in_counts[row] : a.n;
    if (cnt > a.n) cnt = a.n;
    uint64_t *z = a.state + row * a.per;
    const Row w{z, a.in + row * a.in_stride, (uint32_t)cnt * bits, z[0], (uint32_t)z[last_at] & 1u};
    for (uint32_t j = lane; j < a.HW; j += kLanes) ring[ring_slot(j, a.RW)] = z[hist_at + j];
    rw::wave_sync();
    return w;
}

// The words of the chunk's tiles from t0 on into the ring: per tile a ballot of the sign tests, the differential
// decoding under the carried raw bit, lane 0's store.  A push's last word is masked to the bits the push consumes, as
// the HDLC kernel was written.  The frame sync kernel was written without the mask and never reads the bits above them:
// its windows and payloads end at or below the completing bit, the re-alignment ends at ring bit 64 HW + m.  So the one
// form serves both, and the mask's `and` is all that this header changes in what the frame sync kernel computes.
__device__ __forceinline__ void chunk_words(const RowArgs &a, uint64_t *ring, const uint32_t (&cur)[kChunk], uint32_t t0, uint32_t tiles, uint32_t m,
                                            uint32_t &carry, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < kChunk; k++) {
        const uint32_t t = t0 + k;
        if (t < tiles) {
            const uint32_t tn = tile_bits(t, m);
            const uint64_t raw = __ballot(lane < tn && fm::decide(cur[k]) != 0);
            const uint64_t w = fm::diff_word(raw, carry, (int)a.diff) & fm::low_mask(tn);
            carry = (uint32_t)(raw >> (tn - 1)) & 1u;
            if (lane == 0) ring[ring_slot(tile_word(t, a.HW), a.RW)] = w;
        }
    }
    rw::wave_sync();
}

// behind a chunk's tiles: the loads that travelled under them become the chunk
__device__ __forceinline__ void rotate(uint32_t (&cur)[kChunk], const uint32_t (&nxt)[kChunk]) {
    rw::wave_sync();  // (the next chunk's words overwrite the oldest)
#pragma unroll
    for (uint32_t k = 0; k < kChunk; k++) cur[k] = nxt[k];
}

// The row's closing, behind the bank's own state words: the ring re-aligned behind the m bits of the push into the
// history, the common state words, the row's count of frames f.
__device__ __forceinline__ void close_row(const RowArgs &a, const uint64_t *ring, const Row &w, size_t row, uint32_t m, uint64_t bits0, uint32_t carry,
                                          uint32_t f, uint32_t last_at, uint32_t hist_at, uint32_t lane) {
    if (m) {
        for (uint32_t j = lane; j < a.HW; j += kLanes) w.z[hist_at + j] = ring_bits(ring, 64ull * j + m, a.RW);
    }
    if (lane == 0) {
        w.z[0] = bits0 + m;
        w.z[last_at] = carry;
        a.counts[row] = f;
        if (a.maxc) atomicMax(a.maxc, f);
    }
    rw::wave_sync();  // (the next row's history overwrites the ring)
}

// output word j of a frame at dst, of which nb bytes (1 ... 8) are the frame's: a whole 64-bit word where the
// destination is aligned, else byte by byte
__device__ __forceinline__ void store_out_word(uint8_t *dst, uint32_t j, uint64_t y, uint32_t nb) {
    uint8_t *q = dst + 8 * (size_t)j;
    if (nb == 8 && ((uintptr_t)q & 7u) == 0) {
        *(uint64_t *)q = y;
    } else {
        for (uint32_t b = 0; b < nb; b++) q[b] = (uint8_t)(y >> (8 * b));
    }
}

}  // namespace br
}  // namespace hz
