// hz_polyphase.h -- what the two polyphase banks share on the device: the channelizer (hz_channelizer.hip) and the
// synthesis bank (hz_synthesizer.hip) place channel k at the same position and deal frames to workgroups alike.
#pragma once
#include <hip/hip_runtime.h>

namespace hz {

// output position of ZeroFirst channel k (FrequencySlice.Shift, fft/result.go:82-97)
__device__ __forceinline__ unsigned chan_pos(unsigned k, unsigned m, bool neg_first) { return neg_first ? (k + m / 2) & (m - 1) : k; }

// The XCD-aware deal: the hardware hands consecutive workgroup ids to the eight XCDs in turn; this maps the ids that
// share an XCD to a contiguous run of frame groups (bijective for any grid), so that the L/D frames that read one
// sample, and the neighbouring frames that complete one 64-byte segment of a channel-major row, meet in one L2.
// A speed choice only: every workgroup computes the frames of its group whatever the placement.
__device__ __forceinline__ size_t chan_group(unsigned id, unsigned nwg) {
    const unsigned q = nwg / 8, r = nwg % 8, x = id % 8;
    return (size_t)(x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + id / 8;
}

}  // namespace hz
