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
#include "hz_chain_host.h"
#include "../../include/hzsdr_channelizer.h"
#include "hz_polyphase.h"

struct hzsdr_channelizer {
    hzsdr_ctx *ctx;
    int fmt;
    size_t m, ntaps, hop;
    int order, layout;
    hz::fv::FvTabs tabs{};
    float *taps = nullptr;                 // the prototype, L values
    float2 *tail[2] = {nullptr, nullptr};  // the samples held for the next frame, converted: read one, write the other
    int tcur = 0;
    size_t held = 0;     // samples held (below L)
    size_t rot = 0;      // (stream position of the next frame's first sample) mod M
    uint64_t frame = 0;  // index of the next frame
};

namespace hz {

// what a push of n samples does, computed on the host before anything is launched
struct ChanStep {
    size_t V;  // samples of the virtual buffer: held ++ in
    size_t F;  // frames that complete in the push
    size_t new_held;
};

static ChanStep chan_step(const hzsdr_channelizer *c, size_t n) {
    ChanStep p{};
    p.V = c->held + n;
    p.F = p.V >= c->ntaps ? (p.V - c->ntaps) / c->hop + 1 : 0;
    p.new_held = p.V - p.F * c->hop;  // (hop <= M <= L: never a gap; below L)
    return p;
}

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
    const int neg = c->order == HZSDR_ORDER_NEGATIVE_FIRST;
    if (c->layout == HZSDR_CHANNELIZER_FRAME_MAJOR)
        HZ_TRY(launch_fv(channelizer_frames_kernel<M, FMT, HZSDR_CHANNELIZER_FRAME_MAJOR>, grid, block, lds, c->ctx->stream, a, out, stride, neg));
    else
        HZ_TRY(launch_fv(channelizer_frames_kernel<M, FMT, HZSDR_CHANNELIZER_CHANNEL_MAJOR>, grid, block, lds, c->ctx->stream, a, out, stride, neg));
    HZ_HIP(c->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int FMT>
static int chan_launch_fmt(hzsdr_channelizer *c, const ChanArgs &a, float2 *out, size_t stride) {
    switch (c->m) {
    case 256: return chan_launch_m<256, FMT>(c, a, out, stride);
    case 512: return chan_launch_m<512, FMT>(c, a, out, stride);
    case 1024: return chan_launch_m<1024, FMT>(c, a, out, stride);
    case 2048: return chan_launch_m<2048, FMT>(c, a, out, stride);
    case 4096: return chan_launch_m<4096, FMT>(c, a, out, stride);
    case 8192: return chan_launch_m<8192, FMT>(c, a, out, stride);
    default: return HZSDR_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace hz

extern "C" {

int hzsdr_channelizer_create(hzsdr_ctx *ctx, int src_format, size_t channels, const float *taps, size_t n_taps, size_t hop,
                             int order, int layout, hzsdr_channelizer **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    const size_t m = channels;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "channelizer: unknown source format");
    if (m < 256 || m > 8192 || (m & (m - 1)) != 0)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "channelizer: the channel count is a power of two, 256 ... 8192");
    if (!taps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "channelizer: null taps");
    HZ_TRY(check_polyphase_args(ctx, "channelizer", m, n_taps, hop, order, layout));
    HZ_TRY(enter(ctx));
    hzsdr_channelizer *c = new hzsdr_channelizer{ctx, src_format, m, n_taps, hop, order, layout};
    auto undo = [&](int rc) {
        hzsdr_channelizer_free(c);
        return rc;
    };
    int rc = get_fv_tables(ctx, m, &c->tabs);  // (plan-time: the transform's tables, not inside the first push)
    if (rc != HZSDR_OK) return undo(rc);
    hipError_t e = hipMalloc((void **)&c->taps, n_taps * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&c->tail[i], n_taps * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpyAsync(c->taps, taps, n_taps * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (taps is the caller's: free to go when create returns)
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "channelizer_create", __FILE__, __LINE__));
    *out = c;
    return HZSDR_OK;
}

int hzsdr_channelizer_frames_for(const hzsdr_channelizer *c, size_t n_in, size_t *frames) {
    if (!c || !frames) return HZSDR_ERR_INVALID_ARGUMENT;
    *frames = hz::chan_step(c, n_in).F;
    return HZSDR_OK;
}

int hzsdr_channelizer_push(hzsdr_channelizer *c, const void *in, size_t n_in, void *out, size_t out_frames_cap, size_t out_stride,
                           size_t *frames_written) {
    using namespace hz;
    if (frames_written) *frames_written = 0;
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = c->ctx;
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "channelizer: null input");
    const ChanStep p = chan_step(c, n_in);
    const bool chmajor = c->layout == HZSDR_CHANNELIZER_CHANNEL_MAJOR;
    const size_t M = c->m;
    // (the rows of a push: M channels of F frames, out_stride apart, or -- frame-major -- one run of F * M values)
    HZ_TRY(check_rows_out(ctx, "channelizer", chmajor ? M : 1, out, out_frames_cap, out_stride, p.F, 0));
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t dstride;
    HZ_TRY(st.in(0, in, n_in * (size_t)format_size(c->fmt), &din));
    HZ_TRY(st.out_rows(1, out, chmajor ? M : 1, chmajor ? p.F : p.F * M, out_stride, sizeof(float2), &dout, &dstride, true));
    const ChanArgs a{din, c->tail[c->tcur], c->held, c->hop, p.F, c->taps, c->tabs.fwd, (unsigned)c->rot, (unsigned)(c->ntaps / M)};
    if (p.F) HZ_TRY(with_format(c->fmt, [&](auto f) { return chan_launch_fmt<decltype(f)::value>(c, a, (float2 *)dout, dstride); }));
    if (p.new_held) {
        HZ_TRY(hold_samples(ctx, c->fmt, din, a.tail, a.held, p.V - p.new_held, p.new_held, c->tail[c->tcur ^ 1]));
        c->tcur ^= 1;
    }
    c->held = p.new_held;
    c->rot = (c->rot + (p.F & (M - 1)) * c->hop) & (M - 1);  // (running value mod M: no product of stream length)
    c->frame += p.F;
    HZ_TRY(st.finish());
    if (frames_written) *frames_written = p.F;
    return HZSDR_OK;
}

int hzsdr_channelizer_pending(const hzsdr_channelizer *c, size_t *samples_held, uint64_t *frame_index) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (samples_held) *samples_held = c->held;
    if (frame_index) *frame_index = c->frame;
    return HZSDR_OK;
}

int hzsdr_channelizer_reset(hzsdr_channelizer *c) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    // (the held samples are only read behind a later push's own writes: nothing to clear, nothing to wait for)
    c->held = c->rot = 0;
    c->frame = 0;
    return HZSDR_OK;
}

int hzsdr_channelizer_free(hzsdr_channelizer *c) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(c->ctx, {c->taps, c->tail[0], c->tail[1]});
    delete c;
    return HZSDR_OK;
}

}  // extern "C"
