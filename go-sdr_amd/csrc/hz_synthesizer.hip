// hz_synthesizer.hip -- the polyphase synthesis bank (include/hzsdr_synthesizer.h), the adjoint of the channelizer of
// hz_channelizer.hip: every input frame of M channel values goes through one backward transform of the workgroup core
// of hz_fftv.h, and the output stream is the overlap-add of the transforms' outputs, repeated with period M and
// weighted by the prototype's taps.  The L - D partial sums behind the samples written and the rotation
// (stream position of the next frame) mod M stay with the object between pushes.
//
// Two kernels per group of frames.  synthesizer_frames_kernel: a frame per transform group (fv::tpt(M) lanes), the
// sixteen inputs of a lane loaded straight into the backward transform's first-pass slots from pos(k), w_j stored in
// natural order to a device scratch.  synthesizer_ola_kernel: a lane per output position, the terms of the frames that
// cover it in ascending order.  A position is covered by ceil(L / D) frames: consecutive frames are dealt to workgroups
// that share an XCD, so that the second kernel's re-reads of w meet in one L2.  The held state makes a cut between two
// frames free, so a push of any length is processed in groups whose scratch stays within ppp::kSynthScratchBytes.
//
// This file: the kernels, their arguments, their dispatch, the push over the groups and the flush.  What the object
// shares with the channelizer and the channel bank on the host is hz_polyphase.h; the counts of a group and the position
// behind it are hz_polyphase_plan.h.
#include "hz_chain_host.h"
#include "../../include/hzsdr_synthesizer.h"
#include "hz_polyphase.h"

struct hzsdr_synthesizer : hz::pp::Bank {
    static constexpr const char *noun = "synthesizer", *create_name = "synthesizer_create";
    static constexpr const char *format_why = "unknown destination format", *channels_why = "the channel count is a power of two, 256 ... 8192";
    static constexpr hz::ppp::ChannelRule rule = hz::ppp::kTransformRule;
    static constexpr auto destroy = hzsdr_synthesizer_free;
    hz::fv::FvTabs tabs{};
    float2 *w = nullptr;  // the transforms' outputs of one group of frames
    size_t wcap = 0;      // ... frames it has room for
};

namespace hz {

// one term of the overlap-add: THE expression every path evaluates (one fused multiply-add per component)
__device__ __forceinline__ float2 synth_term(float2 acc, float g, float2 w) { return make_float2(__fmaf_rn(g, w.x, acc.x), __fmaf_rn(g, w.y, acc.y)); }

// hzsdr_convert's c64 -> dst arithmetic (hz_convert.hip: conv1<C64_*>) on one finished sum
template <int FMT> struct SynthDst;
template <> struct SynthDst<HZSDR_FMT_C64> {
    using t = float2;
    static __device__ __forceinline__ t cvt(float2 v) { return v; }
};
template <> struct SynthDst<HZSDR_FMT_U8> {
    using t = uint16_t;
    static __device__ __forceinline__ t cvt(float2 v) { return (uint16_t)(f32_to_u8(v.x) | (f32_to_u8(v.y) << 8)); }
};
template <> struct SynthDst<HZSDR_FMT_I8> {
    using t = uint16_t;
    static __device__ __forceinline__ t cvt(float2 v) { return (uint16_t)(f32_to_i8(v.x) | (f32_to_i8(v.y) << 8)); }
};
template <> struct SynthDst<HZSDR_FMT_I16> {
    using t = uint32_t;
    static __device__ __forceinline__ t cvt(float2 v) { return f32_to_i16(v.x) | (f32_to_i16(v.y) << 16); }
};

// w[f][.] = M * IDFT_M(Y[f][.]) for the F frames of a group.  Frame-major: in[f * M + pos(k)]; channel-major:
// in[pos(k) * stride + f].
template <int M, int LAYOUT>
__global__ __launch_bounds__(fv::block(M)) void synthesizer_frames_kernel(const float2 *__restrict__ in, size_t stride, size_t F, const cf4 *tab,
                                                                          float2 *__restrict__ w, int neg_first) {
    constexpr int TPT = fv::tpt(M), XPB = fv::xpb(M), R0 = fv::first_radix(M);
    constexpr bool WAVE = TPT <= 64;
    const int sub = XPB == 1 ? 0 : threadIdx.x / TPT, lane = XPB == 1 ? (int)threadIdx.x : threadIdx.x % TPT;
    cf *lds = fv_lds() + sub * fv::lds_elems(M);
    const size_t f = chan_group(blockIdx.x, gridDim.x) * XPB + sub;
    const bool live = f < F;
    const size_t fr = live ? f : F - 1;  // (dead transforms run the last frame and drop it)
    cf v[16];
    // frequency side = the radix-16 edge layout of the backward transform's first pass
    if constexpr (LAYOUT == HZSDR_CHANNELIZER_FRAME_MAJOR) {
        const float2 *x = in + fr * M;
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = fv::from2(x[chan_pos(fv::edge_off<M, 16>(q) + lane, M, neg_first)]);
    } else {
        const float2 *x = in + fr;
#pragma unroll
        for (int q = 0; q < 16; q++) v[q] = fv::from2(x[(size_t)chan_pos(fv::edge_off<M, 16>(q) + lane, M, neg_first) * stride]);
    }
    // one wave per transform up to M = 1024 (the wave orders its own LDS operations), a workgroup beyond
    fv::backward<M, WAVE>(v, lds, tab, lane);
    if (!live) return;
    // time side = the edge layout of the last pass's radix
    float2 *o = w + f * M + lane;
#pragma unroll
    for (int q = 0; q < 16; q++) o[fv::edge_off<M, R0>(q)] = fv::to2(v[q]);
}

// The overlap-add of one group.  Positions u count from the group's first frame; the stream position is T0 + u with
// T0 mod M = rot.  Frame j of the group covers [jD, jD + L).
struct SynthOla {
    const float2 *w;        // F rows of M
    const float *taps;      // L
    const float2 *hold_in;  // `held` partial sums at u = 0 ..
    float2 *hold_out;       // receives the sums at u = n_out ..
    unsigned F, D, L, mask;  // mask = M - 1
    unsigned rot, held, n_out, total;
};

// One lane per position u < total: acc = the old partial sum where one exists, else +0; then the group's frames that
// cover u, j ascending.  Across the lanes of a wave the loads of w_j[(rot + u) mod M] and g[u - jD] are contiguous but
// for the wrap.  The first n_out sums are finished: converted and stored; the rest are the new held state.
// (F = 0, n_out = total = held: the flush.)
template <int FMT>
__global__ __launch_bounds__(kThreads) void synthesizer_ola_kernel(SynthOla a, typename SynthDst<FMT>::t *__restrict__ out) {
    const unsigned u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= a.total) return;
    float2 acc = u < a.held ? a.hold_in[u] : make_float2(0.f, 0.f);
    if (a.F) {
        const unsigned j_lo = u >= a.L ? (u - a.L) / a.D + 1 : 0, j_hi = min(a.F - 1, u / a.D);
        const unsigned n = j_hi - j_lo + 1;  // (at least one: D <= L leaves no gap)
        const size_t M = (size_t)a.mask + 1;
        const float2 *wp = a.w + (size_t)j_lo * M + ((a.rot + u) & a.mask);
        const float *gp = a.taps + (u - j_lo * a.D);
        unsigned k = 0;
#pragma unroll 1
        for (; k + 4 <= n; k += 4) {
            float2 ww[4];
            float gg[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                ww[i] = wp[(size_t)i * M];
                gg[i] = *(gp - (size_t)i * a.D);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) acc = synth_term(acc, gg[i], ww[i]);
            wp += 4 * M;
            gp -= (size_t)4 * a.D;
            // (the trip's eight loads in flight before the first use: channelizer_frames_kernel's note applies)
            __builtin_amdgcn_sched_group_barrier(0x020, 8, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 64, 0);
        }
#pragma unroll 1
        for (; k < n; k++) {
            acc = synth_term(acc, *gp, *wp);
            wp += M;
            gp -= a.D;
        }
    }
    if (u < a.n_out)
        out[u] = SynthDst<FMT>::cvt(acc);
    else
        a.hold_out[u - a.n_out] = acc;
}

template <int M>
static int synth_frames_m(hzsdr_synthesizer *s, const float2 *in, size_t stride, size_t F) {
    constexpr int XPB = fv::xpb(M);
    const dim3 grid((unsigned)((F + XPB - 1) / XPB)), block(fv::block(M));
    const size_t lds = (size_t)XPB * fv::lds_elems(M) * sizeof(cf);
    HZ_TRY(pp::with_layout(s->layout, [&](auto l) {
        return launch_fv(synthesizer_frames_kernel<M, decltype(l)::value>, grid, block, lds, s->ctx->stream, in, stride, F, s->tabs.bwd, s->w, (int)s->negative_first());
    }));
    HZ_HIP(s->ctx, hipGetLastError());
    return HZSDR_OK;
}

static int synth_frames(hzsdr_synthesizer *s, const float2 *in, size_t stride, size_t F) {
    return pp::with_fv_size(s->M, [&](auto m) { return synth_frames_m<decltype(m)::value>(s, in, stride, F); });
}

// one group's overlap-add (the flush: no frames): the counts of hz_polyphase_plan.h in the kernel's arguments
static int synth_ola(hzsdr_synthesizer *s, const ppp::Group &g, void *out) {
    const bool flush = g.F == 0;
    const SynthOla a{flush ? nullptr : s->w, s->taps, s->held.now(), flush ? nullptr : s->held.next(), g.F, s->D, s->L, s->M - 1,
                     flush ? 0u : s->st.rot, g.held, g.n_out, g.total};
    const dim3 grid((a.total + kThreads - 1) / kThreads), block(kThreads);
    with_format(s->fmt, [&](auto f) {
        constexpr int FMT = decltype(f)::value;
        hipLaunchKernelGGL(synthesizer_ola_kernel<FMT>, grid, block, 0, s->ctx->stream, a, (typename SynthDst<FMT>::t *)out);
    });
    HZ_HIP(s->ctx, hipGetLastError());
    return HZSDR_OK;
}

// room in the scratch for the largest group of a push of n frames (grow-only, before anything is launched)
static int synth_scratch(hzsdr_synthesizer *s, size_t n) {
    const size_t want = ppp::scratch_frames(n, s->M);
    if (want <= s->wcap) return HZSDR_OK;
    if (s->w) {
        HZ_HIP(s->ctx, hipStreamSynchronize(s->ctx->stream));  // (enqueued work may still read the old one)
        HZ_HIP(s->ctx, hipFree(s->w));
        s->w = nullptr;
        s->wcap = 0;
    }
    HZ_HIP(s->ctx, hipMalloc((void **)&s->w, want * s->M * sizeof(float2)));
    s->wcap = want;
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_synthesizer_create(hzsdr_ctx *ctx, int dst_format, size_t channels, const float *taps, size_t n_taps, size_t hop,
                             int order, int layout, hzsdr_synthesizer **out) {
    using namespace hz;
    // (plan-time: the transform's tables, not inside the first push)
    return pp::create(ctx, dst_format, channels, taps, n_taps, hop, order, layout, out,
                      [&](hzsdr_synthesizer *s, std::vector<Table> &) { return get_fv_tables(ctx, s->M, &s->tabs); });
}

int hzsdr_synthesizer_push(hzsdr_synthesizer *s, const void *frames, size_t n_frames, size_t in_stride, void *out, size_t out_cap,
                           size_t *samples_written) {
    using namespace hz;
    if (samples_written) *samples_written = 0;
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = s->ctx;
    const bool chmajor = s->channel_major();
    const size_t M = s->M, D = s->D, n_out = n_frames * D;
    if (n_frames && !frames) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "synthesizer: null input");
    if (chmajor && in_stride < n_frames) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "synthesizer: in_stride is below the frames of the push");
    HZ_TRY(check_rows_out(ctx, "synthesizer", 1, out, out_cap, 0, n_out, 0));
    HZ_TRY(enter(ctx));
    if (n_frames == 0) return HZSDR_OK;
    HZ_TRY(synth_scratch(s, n_frames));
    const size_t fs = (size_t)format_size(s->fmt);
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t dstride;
    // (M channels of n_frames frames, in_stride apart, or -- frame-major -- one run of n_frames * M values)
    HZ_TRY(st.in_rows(0, frames, chmajor ? M : 1, chmajor ? n_frames : n_frames * M, in_stride, sizeof(float2), &din, &dstride));
    HZ_TRY(st.out(1, out, n_out * fs, &dout));
    const size_t group = ppp::group_frames(M);
    for (size_t f0 = 0; f0 < n_frames; f0 += group) {
        const size_t F = std::min(group, n_frames - f0);
        HZ_TRY(synth_frames(s, (const float2 *)din + (chmajor ? f0 : f0 * M), dstride, F));
        HZ_TRY(synth_ola(s, ppp::group(s->st, s->L, s->D, F), (char *)dout + f0 * D * fs));
        s->held.flip();
        s->st = ppp::after_group(s->st, s->M, s->L, s->D, F);
    }
    HZ_TRY(st.finish());
    if (samples_written) *samples_written = n_out;
    return HZSDR_OK;
}

int hzsdr_synthesizer_flush(hzsdr_synthesizer *s, void *out, size_t out_cap, size_t *samples_written) {
    using namespace hz;
    if (samples_written) *samples_written = 0;
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = s->ctx;
    const size_t n = (size_t)s->st.held;
    HZ_TRY(check_rows_out(ctx, "synthesizer", 1, out, out_cap, 0, n, 0));
    HZ_TRY(enter(ctx));
    if (n) {
        Stage st(ctx);
        void *dout;
        HZ_TRY(st.out(1, out, n * (size_t)format_size(s->fmt), &dout));
        HZ_TRY(synth_ola(s, ppp::flush_group(s->st), dout));
        HZ_TRY(st.finish());
    }
    s->st = ppp::State{};
    if (samples_written) *samples_written = n;
    return HZSDR_OK;
}

int hzsdr_synthesizer_pending(const hzsdr_synthesizer *s, size_t *samples_held, uint64_t *frame_index) { return hz::pp::pending(s, samples_held, frame_index); }

int hzsdr_synthesizer_group_frames(const hzsdr_synthesizer *s, size_t *frames) {
    if (!s || !frames) return HZSDR_ERR_INVALID_ARGUMENT;
    *frames = hz::ppp::group_frames(s->M);
    return HZSDR_OK;
}

int hzsdr_synthesizer_reset(hzsdr_synthesizer *s) { return hz::pp::reset(s); }

int hzsdr_synthesizer_free(hzsdr_synthesizer *s) { return hz::pp::release(s, {s ? s->w : nullptr}); }

}  // extern "C"
