// hz_polyphase.h -- what the frame-by-frame banks share.  On the device: the channelizer (hz_channelizer.hip) and the
// synthesis bank (hz_synthesizer.hip) place channel k at the same position and deal frames to workgroups alike; the
// channelizer, the spectrum (hz_spectrum.hip) and the channel bank (hz_chanbank.hip) keep the samples that the next
// frame still needs with ONE kernel (held_samples_kernel) and one launcher (hold_samples).  On the host: the argument checks of the
// three polyphase objects' create (check_polyphase_args).
#pragma once
#include "hz_chain_host.h"
#include "../../include/hzsdr_channelizer.h"

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

// The samples held for the next frame: V[start .. start + cnt) converted, where V = tail[0 .. held) ++ convert(in[0 ..))
// is the push's virtual buffer (the samples held before it, then its own).
template <int FMT>
__global__ __launch_bounds__(kThreads) void held_samples_kernel(const void *in, const float2 *tail, size_t held, size_t start, size_t cnt,
                                                                float2 *__restrict__ tail_out) {
    using R = typename Raw<FMT>::t;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < cnt; i += (size_t)gridDim.x * kThreads) {
        const size_t v = start + i;
        tail_out[i] = v < held ? tail[v] : Raw<FMT>::cvt(((const R *)in)[v - held]);
    }
}

// its one launcher (hz_channelizer.hip: the kernel is part of that unit's code object alone)
int hold_samples(hzsdr_ctx *ctx, int fmt, const void *in, const float2 *tail, size_t held, size_t start, size_t cnt, float2 *tail_out);

// What the channelizer, the synthesis bank and the channel bank ask of a prototype of n_taps taps over m channels (the
// rule for m itself stays with each), of the hop, the order and the layout.
inline int check_polyphase_args(hzsdr_ctx *ctx, const char *who, size_t m, size_t n_taps, size_t hop, int order, int layout) {
    const std::string w = std::string(who) + ": ";
    if (n_taps == 0 || n_taps % m != 0 || n_taps > 32 * m)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "the prototype has P * channels taps, 1 <= P <= 32");
    if (hop == 0 || hop > m) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "the hop is 1 ... channels");
    if (order != HZSDR_ORDER_ZERO_FIRST && order != HZSDR_ORDER_NEGATIVE_FIRST) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "unknown fft order");
    if (layout != HZSDR_CHANNELIZER_FRAME_MAJOR && layout != HZSDR_CHANNELIZER_CHANNEL_MAJOR)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "unknown layout");
    return HZSDR_OK;
}

}  // namespace hz
