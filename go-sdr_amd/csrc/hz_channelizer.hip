// hz_channelizer.hip -- the polyphase channelizer (include/hzsdr_channelizer.h): frames of a raw IQ stream converted
// in the loads, folded with the prototype's taps into M values indexed by absolute time modulo M, transformed by the
// workgroup core of hz_fftv.h and stored as complex rows (frame-major) or as one stream per channel (channel-major).
// One pass over the raw samples; the samples the next frame still needs (converted complex64) and the rotation
// jD mod M stay with the object between pushes.
//
// One kernel form: every frame of a push on its own transform group (fv::tpt(M) lanes, sixteen fold outputs per
// lane in the first pass's edge layout).  The rotation is applied AT LOAD TIME: fold output r of frame j takes the
// frame offsets i_p = ((r - jD) mod M) + pM, for the samples and for the taps alike, so the transform's input is
// u_j in natural order and nothing follows the transform but the store.  A sample is read by L/D frames: consecutive
// frames are dealt to workgroups that share an XCD (and so an L2), which keeps the re-reads and the taps in that L2.
//
// This file: the kernel, its arguments, its dispatch and the ABI functions.  The object's host side (create, the push
// around the launch, frames_for, pending, reset, free) is hz_polyphase.h, the stream arithmetic hz_polyphase_plan.h.
#include "hz_chain_host.h"
#include "../../include/hzsdr_channelizer.h"
#include "hz_polyphase.h"

struct hzsdr_channelizer : hz::pp::Bank {
    static constexpr const char *noun = "channelizer", *create_name = "channelizer_create";
    static constexpr const char *format_why = "unknown source format", *channels_why = "the channel count is a power of two, 256 ... 8192";
    static constexpr hz::ppp::ChannelRule rule = hz::ppp::kTransformRule;
    static constexpr auto destroy = hzsdr_channelizer_free;
    hz::fv::FvTabs tabs{};
};

namespace hz {

// The frames of one launch.  Frame f (0-based within the push) starts at virtual index f*hop of
// V = tail[0 .. held) ++ convert(in[0 ..)); its rotation is (rot + f*hop) mod M.
struct ChanArgs {
    const void *in;
    const float2 *tail;
    size_t held, hop, F;
    const float *taps;
    const cf4 *tab;
    unsigned rot, P;
};

// one term of the fold: THE expression every path evaluates (one fused multiply-add per component)
__device__ __forceinline__ cf chan_fold(cf acc, float g, float2 x) { return cf{__fmaf_rn(g, x.x, acc.x), __fmaf_rn(g, x.y, acc.y)}; }

// a value every lane of the wave holds the same of, as a scalar
__device__ __forceinline__ int64_t chan_uniform(int64_t v) {
    return (int64_t)(((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
                     (unsigned)__builtin_amdgcn_readfirstlane((int)v));
}

// waves per SIMD the register allocator is asked to leave room for (the fold is loads: it wants waves to hide them)
constexpr int chan_occupancy(int m) { return fv::block(m) >= 512 ? 2 : 4; }

template <int M, int FMT, int LAYOUT>
__global__ __launch_bounds__(fv::block(M), chan_occupancy(M)) void channelizer_frames_kernel(ChanArgs a, float2 *__restrict__ out, size_t stride, int neg_first) {
    constexpr int TPT = fv::tpt(M), XPB = fv::xpb(M), R0 = fv::first_radix(M);
    constexpr bool WAVE = TPT <= 64;
    using RT = typename Raw<FMT>::t;
    const int sub = XPB == 1 ? 0 : threadIdx.x / TPT, lane = XPB == 1 ? (int)threadIdx.x : threadIdx.x % TPT;
    cf *lds = fv_lds() + sub * fv::lds_elems(M);
    const size_t f0 = chan_group(blockIdx.x, gridDim.x) * XPB, f = f0 + sub;
    const bool live = f < a.F;
    const size_t base = (live ? f : a.F - 1) * a.hop;  // (dead transforms fold the last frame and drop it)
    const unsigned s = (unsigned)((a.rot + base) & (M - 1));
    cf v[16];
    if (base >= a.held) {  // the frame lies wholly in the input
        // One loop-invariant scalar base per stream and one 32-bit lane offset per fold output, p * M added to it
        // inside the loop (the workgroup's frames differ in the offset): every load is "scalar base + 32-bit lane
        // offset", no 64-bit address per load kept across the loop (64 registers otherwise).
        // The offsets at p = 0 are contiguous across the lanes but for the rotation's wrap point.
        const RT *x = (const RT *)a.in + chan_uniform((int64_t)(f0 * a.hop) - (int64_t)a.held);
        const float *g = a.taps;
        const unsigned rel = (unsigned)(base - f0 * a.hop);
        unsigned i0[16];
#pragma unroll
        for (int q = 0; q < 16; q++) {
            i0[q] = ((unsigned)(fv::edge_off<M, R0>(q) + lane) - s) & (M - 1);
            v[q] = cf{0.f, 0.f};
        }
        const char *xb = (const char *)x, *gb = (const char *)g;  // (32-bit byte offsets from the scalar bases)
#pragma unroll 1
        for (unsigned p = 0, pm = 0; p < a.P; p++, pm += M) {
            RT r[16];
            float t[16];
#pragma unroll
            for (int q = 0; q < 16; q++) {
                r[q] = *(const RT *)(xb + (rel + i0[q] + pm) * (unsigned)sizeof(RT));
                t[q] = *(const float *)(gb + (i0[q] + pm) * (unsigned)sizeof(float));
            }
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = chan_fold(v[q], t[q], Raw<FMT>::cvt(r[q]));
            // (all thirty-two loads in flight before the first use: left alone, the scheduler pairs every load
            // with its use to save registers, and a wave then waits for one load at a time)
            __builtin_amdgcn_sched_group_barrier(0x020, 32, 0);  // the trip's 32 loads first,
            __builtin_amdgcn_sched_group_barrier(0x002, 512, 0);  // then its arithmetic
        }
    } else {
        // (it starts in the held samples: at most L/D frames of a push.  One fold output at a time, p innermost,
        // through the transform's LDS region -- the same terms in the same order, and no registers to speak of)
#pragma unroll 1
        for (int t = 0; t < 16; t++) {
            const unsigned r = lane + t * TPT;
            const size_t o0 = (r - s) & (M - 1);
            cf acc = cf{0.f, 0.f};
#pragma unroll 1
            for (unsigned p = 0; p < a.P; p++) {
                const size_t o = (size_t)p * M + o0, i = base + o;
                const float2 x = i < a.held ? a.tail[i] : Raw<FMT>::cvt(((const RT *)a.in)[i - a.held]);
                acc = chan_fold(acc, a.taps[o], x);
            }
            lds[fv::pad(r)] = acc;
        }
        fv::sync<WAVE>();
        fv::load_lds<M, R0>(v, lds, lane);
    }
    // the transform: one wave per transform up to M = 1024 (the wave orders its own LDS operations), a workgroup
    // beyond.  (FROM_LDS: a barrier in front of its first store, for the lanes still loading above.)
    fv::forward<M, true, WAVE>(v, lds, a.tab, lane);
    if (!live) return;
    if constexpr (LAYOUT == HZSDR_CHANNELIZER_FRAME_MAJOR) {
        float2 *o = out + f * M;
#pragma unroll
        for (int q = 0; q < 16; q++) o[chan_pos(lane + q * TPT, M, neg_first)] = fv::to2(v[q]);
    } else {
        float2 *o = out + f;
#pragma unroll
        for (int q = 0; q < 16; q++) o[(size_t)chan_pos(lane + q * TPT, M, neg_first) * stride] = fv::to2(v[q]);
    }
}

int hold_samples(hzsdr_ctx *ctx, int fmt, const void *in, const float2 *tail, size_t held, size_t start, size_t cnt, float2 *tail_out) {
    with_format(fmt, [&](auto f) {
        hipLaunchKernelGGL(held_samples_kernel<decltype(f)::value>, dim3(blocks_for(ctx, cnt)), dim3(kThreads), 0, ctx->stream, in, tail, held,
                           start, cnt, tail_out);
    });
    HZ_HIP(ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int M, int FMT>
static int chan_launch_m(hzsdr_channelizer *c, const ChanArgs &a, float2 *out, size_t stride) {
    constexpr int XPB = fv::xpb(M);
    const dim3 grid((unsigned)((a.F + XPB - 1) / XPB)), block(fv::block(M));
    const size_t lds = (size_t)XPB * fv::lds_elems(M) * sizeof(cf);
    HZ_TRY(pp::with_layout(c->layout, [&](auto l) {
        return launch_fv(channelizer_frames_kernel<M, FMT, decltype(l)::value>, grid, block, lds, c->ctx->stream, a, out, stride, (int)c->negative_first());
    }));
    HZ_HIP(c->ctx, hipGetLastError());
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_channelizer_create(hzsdr_ctx *ctx, int src_format, size_t channels, const float *taps, size_t n_taps, size_t hop,
                             int order, int layout, hzsdr_channelizer **out) {
    using namespace hz;
    // (plan-time: the transform's tables, not inside the first push)
    return pp::create(ctx, src_format, channels, taps, n_taps, hop, order, layout, out,
                      [&](hzsdr_channelizer *c, std::vector<Table> &) { return get_fv_tables(ctx, c->M, &c->tabs); });
}

int hzsdr_channelizer_frames_for(const hzsdr_channelizer *c, size_t n_in, size_t *frames) { return hz::pp::frames_for(c, n_in, frames); }

int hzsdr_channelizer_push(hzsdr_channelizer *c, const void *in, size_t n_in, void *out, size_t out_frames_cap, size_t out_stride,
                           size_t *frames_written) {
    using namespace hz;
    return pp::push_frames(c, in, n_in, out, out_frames_cap, out_stride, frames_written, [&](const void *din, float2 *dout, size_t dstride, const ppp::Step &p) {
        const ChanArgs a{din, c->held.now(), (size_t)c->st.held, c->D, (size_t)p.F, c->taps, c->tabs.fwd, c->st.rot, c->L / c->M};
        return with_format(c->fmt, [&](auto f) {
            return pp::with_fv_size(c->M, [&](auto m) { return chan_launch_m<decltype(m)::value, decltype(f)::value>(c, a, dout, dstride); });
        });
    });
}

int hzsdr_channelizer_pending(const hzsdr_channelizer *c, size_t *samples_held, uint64_t *frame_index) { return hz::pp::pending(c, samples_held, frame_index); }

int hzsdr_channelizer_reset(hzsdr_channelizer *c) { return hz::pp::reset(c); }

int hzsdr_channelizer_free(hzsdr_channelizer *c) { return hz::pp::release(c); }

}  // extern "C"
