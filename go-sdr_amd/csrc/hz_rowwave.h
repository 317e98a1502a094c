// hz_rowwave.h -- the device side of the row-wave banks (hz_iir.hip, hz_symsync.hip, hz_carrier.hip, hz_agc.hip): what a
// kernel of the shape "a workgroup is ONE wave, it owns G consecutive rows for the whole push, lane = row walks time" is
// made of, apart from its walk and its state.  The host arithmetic and the reasons for the shape are
// hz_rowwave_plan.h; the host side of the banks' objects is hz_loopbank.h.
//
// Time goes by in tiles of T = 64 K samples through the wave's own LDS, so nothing ever waits for another wave:
//   1. the tile's raw samples, fetched a tile ahead into registers by all 64 lanes (row fixed, lane = sample: K
//      instructions per row), are converted and written into the tile TRANSPOSED, sample t of row r at float t P + r
//      (P odd: one lane per bank), by rw::move_slot;
//   2. fetch: the loads of the NEXT tile are issued, and stay in flight under
//   3. the bank's walk, lane = row, t = 0 ... tn - 1, by rw::walk_slot;
//   4. the tile is read back row by row (lane = sample again) and stored likewise -- or the bank's own read-out, where
//      what the walk leaves is not one value per sample;
// with a wave_sync between the steps.  The loop, and steps 1 and 4 in it, stay written out in each kernel: as helpers
// (tile_put / tile_get over a conversion) they reach the kernel optimised on their own first, which reorders the
// instructions of every kernel of the two banks there were then; measured so, the symbol-timing bank's complex rows
// were 1.9 % slower at R = 100 and the IIR bank 1 to 3 % faster (profiles/rowwave_time.txt), and this header is to
// change no kernel.
#pragma once
#include "hz_rowwave_plan.h"

namespace hz {
namespace rw {

// The wave's own LDS traffic in program order: what its lanes wrote is what its lanes read.  The workgroup IS the wave,
// so no other wave is waited for.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A value loaded before the tile loop is waited for HERE, not at its first use inside the loop: a wait placed in the loop
// would, on every trip, also wait for the next tile's loads that are meant to stay in flight under the walk.
// (V: float or uint32_t, one register)
template <typename V> __device__ __forceinline__ void settle(V v) {
    static_assert(sizeof(V) == 4, "one VGPR");
    asm volatile("" ::"v"(v));
}

// what a lane is to its wave: the wave's rows are [row0, row0 + g), and lane l < g owns row l of them
struct Wave {
    uint32_t lane, row0, g;
    bool own;
    size_t row;  // (the lane's row, where it owns one)
};
// a: the kernel's arguments, of which G (Geom::G) and R (the bank's rows) are read
template <typename Args> __device__ __forceinline__ Wave wave(const Args &a) {
    const uint32_t lane = threadIdx.x, row0 = wave_first_row(blockIdx.x, a.G), g = wave_row_count(blockIdx.x, a.G, a.R);
    return {lane, row0, g, lane < g, (size_t)row0 + lane};
}

// the tile's samples of the wave's rows into registers: lane = sample, K steps of 64 samples per row
template <typename RT, int K>
__device__ __forceinline__ void fetch(RT (&raw)[kMaxGroup][K], const RT *in, size_t in_stride, uint32_t g, uint64_t t0, uint64_t n, uint32_t lane) {
#pragma unroll
    for (uint32_t r = 0; r < kMaxGroup; r++) {
        if (r < g) {
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint64_t t = t0 + lane + kLanes * k;
                if (t < n) raw[r][k] = in[r * in_stride + t];
            }
        }
    }
}

}  // namespace rw
}  // namespace hz
