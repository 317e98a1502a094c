// hz_polyphase.h -- what the frame-by-frame banks share.  On the device: the channelizer (hz_channelizer.hip) and the
// synthesis bank (hz_synthesizer.hip) place channel k at the same position and deal frames to workgroups alike; the
// channelizer, the spectrum (hz_spectrum.hip) and the channel bank (hz_chanbank.hip) keep the samples that the next
// frame still needs with ONE kernel (held_samples_kernel) and one launcher (hold_samples).  On the host (namespace pp):
// the side of the three polyphase objects around their kernels -- what they hold alike (Bank, Held) and the calls over
// it: the head of a create, the analysis push around a bank's launch, frames_for, pending, reset, release, and the
// dispatch over the layout and the transform size.  A bank's object derives from Bank and adds its own tables and, as
// statics, the noun that starts its messages, its rule for M and its words for a refusal of M or the format.  The
// arithmetic is hz_polyphase_plan.h; nothing in pp knows which bank it serves.
#pragma once
#include "hz_chain_host.h"
#include "../../include/hzsdr_channelizer.h"
#include "hz_polyphase_plan.h"

namespace hz {

// output position of ZeroFirst channel k (FrequencySlice.Shift, fft/result.go:82-97): ppp::pos for a power of two m,
// in the form the transform kernels were compiled with
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

// The refusals of ppp::check_args that do not depend on the bank, as messages behind the bank's noun: what the three
// ask of a prototype of n_taps taps over m channels, of the hop, the order and the layout.
// (out of line, and not hidden: the library's dynamic symbols list it)
__attribute__((noinline)) inline int check_polyphase_args(hzsdr_ctx *ctx, const char *who, size_t m, size_t n_taps, size_t hop, int order, int layout) {
    const std::string w = std::string(who) + ": ";
    switch (ppp::check_args(ppp::ChannelRule{m, m, false}, m, true, n_taps, hop, order, layout)) {
    case ppp::kBadTaps: return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "the prototype has P * channels taps, 1 <= P <= 32");
    case ppp::kBadHop: return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "the hop is 1 ... channels");
    case ppp::kBadOrder: return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "unknown fft order");
    case ppp::kBadLayout: return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "unknown layout");
    default: return HZSDR_OK;
    }
}

static_assert(ppp::kOrderZeroFirst == HZSDR_ORDER_ZERO_FIRST && ppp::kOrderNegativeFirst == HZSDR_ORDER_NEGATIVE_FIRST, "hz_polyphase_plan.h");
static_assert(ppp::kFrameMajor == HZSDR_CHANNELIZER_FRAME_MAJOR && ppp::kChannelMajor == HZSDR_CHANNELIZER_CHANNEL_MAJOR, "hz_polyphase_plan.h");

// (hidden: the instantiations below add nothing to the library's dynamic symbols)
namespace pp __attribute__((visibility("hidden"))) {

// a pair of device buffers of which a call reads one and writes the other
struct Held {
    float2 *buf[2] = {nullptr, nullptr};
    int cur = 0;
    const float2 *now() const { return buf[cur]; }
    float2 *next() const { return buf[cur ^ 1]; }
    void flip() { cur ^= 1; }
};

// V[start .. start + cnt) of the push's virtual buffer (`held` samples of h, then `din`) kept in h for the next push
inline int keep(hzsdr_ctx *ctx, int fmt, Held &h, const void *din, size_t held, size_t start, size_t cnt) {
    if (cnt == 0) return HZSDR_OK;
    HZ_TRY(hold_samples(ctx, fmt, din, h.now(), held, start, cnt, h.next()));
    h.flip();
    return HZSDR_OK;
}

struct Bank {
    hzsdr_ctx *ctx = nullptr;
    int fmt = 0;
    uint32_t M = 0, L = 0, D = 0;  // channels, taps, hop
    int order = 0, layout = 0;
    float *taps = nullptr;  // the prototype, L values
    Held held;              // the samples held for the next frame, converted; the synthesis bank: the L - D partial sums
    ppp::State st{};
    bool channel_major() const { return layout == HZSDR_CHANNELIZER_CHANNEL_MAJOR; }
    bool negative_first() const { return order == HZSDR_ORDER_NEGATIVE_FIRST; }
};

template <class F> std::string who(const char *msg) { return std::string(F::noun) + ": " + msg; }

// f(std::integral_constant<int, LAYOUT>{}) for the layout, as with_format
template <class Fn> inline auto with_layout(int layout, Fn &&f) {
    if (layout == HZSDR_CHANNELIZER_FRAME_MAJOR) return f(std::integral_constant<int, HZSDR_CHANNELIZER_FRAME_MAJOR>{});
    return f(std::integral_constant<int, HZSDR_CHANNELIZER_CHANNEL_MAJOR>{});
}
// f(std::integral_constant<int, M>{}) -> status for a size of the workgroup transform (hz_fftv.h)
template <class Fn> inline int with_fv_size(size_t m, Fn &&f) {
    switch (m) {
    case 256: return f(std::integral_constant<int, 256>{});
    case 512: return f(std::integral_constant<int, 512>{});
    case 1024: return f(std::integral_constant<int, 1024>{});
    case 2048: return f(std::integral_constant<int, 2048>{});
    case 4096: return f(std::integral_constant<int, 4096>{});
    case 8192: return f(std::integral_constant<int, 8192>{});
    default: return HZSDR_ERR_INVALID_ARGUMENT;
    }
}

// the object's device buffers go, then the object (the body of every *_free; `own`: the bank's own buffers)
template <class F> int release(F *c, std::initializer_list<void *> own = {}) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    bank_release(c->ctx, {c->taps, c->held.buf[0], c->held.buf[1]});
    for (void *p : own)
        if (p) (void)hipFree(p);
    delete c;
    return HZSDR_OK;
}

// A create: the checks in their order, the object with the shared fields filled in, own(c, tables) -> status for the
// bank's own (the transform's tables, its host tables, and its device tables added to `tables`), then all the device
// memory -- the prototype, the two held buffers of L values, the bank's own -- and its contents.  A failure behind the
// checks frees what there is.
template <class F, class Own>
int create(hzsdr_ctx *ctx, int fmt, size_t channels, const float *taps, size_t n_taps, size_t hop, int order, int layout, F **out, Own own) {
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(fmt) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, who<F>(F::format_why));
    const ppp::Refusal bad = ppp::check_args(F::rule, channels, taps != nullptr, n_taps, hop, order, layout);
    if (bad == ppp::kBadChannels) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>(F::channels_why));
    if (bad == ppp::kNullTaps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("null taps"));
    if (bad) return check_polyphase_args(ctx, F::noun, channels, n_taps, hop, order, layout);
    HZ_TRY(enter(ctx));
    F *c = new F;
    c->ctx = ctx, c->fmt = fmt, c->M = (uint32_t)channels, c->L = (uint32_t)n_taps, c->D = (uint32_t)hop, c->order = order, c->layout = layout;
    // (taps is the caller's: free to go when create returns)
    std::vector<Table> tables{{(void **)&c->taps, taps, n_taps * sizeof(float)},
                              {(void **)&c->held.buf[0], nullptr, n_taps * sizeof(float2)},
                              {(void **)&c->held.buf[1], nullptr, n_taps * sizeof(float2)}};
    int rc = own(c, tables);
    if (rc == HZSDR_OK) rc = upload(ctx, F::create_name, tables);
    if (rc != HZSDR_OK) return F::destroy(c), rc;
    *out = c;
    return HZSDR_OK;
}

// The analysis push around a bank's launch: the checks in their order, the rows staged, launch(din, dout, dstride, step)
// -> status for the frames that complete, the samples the next frame needs kept, the position committed.
template <class F, class Launch>
int push_frames(F *c, const void *in, size_t n_in, void *out, size_t out_frames_cap, size_t out_stride, size_t *frames_written, Launch launch) {
    if (frames_written) *frames_written = 0;
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = c->ctx;
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("null input"));
    const ppp::Step p = ppp::step(c->st, c->M, c->L, c->D, n_in);
    if (!p.ok) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("the push is too long"));
    const bool chmajor = c->channel_major();
    const size_t F_ = (size_t)p.F, M = c->M;
    // (the rows of a push: M channels of F frames, out_stride apart, or -- frame-major -- one run of F * M values)
    HZ_TRY(check_rows_out(ctx, F::noun, chmajor ? M : 1, out, out_frames_cap, out_stride, F_, 0));
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t dstride;
    HZ_TRY(st.in(0, in, n_in * (size_t)format_size(c->fmt), &din));
    HZ_TRY(st.out_rows(1, out, chmajor ? M : 1, chmajor ? F_ : F_ * M, out_stride, sizeof(float2), &dout, &dstride, true));
    if (F_) HZ_TRY(launch(din, (float2 *)dout, dstride, p));
    HZ_TRY(keep(ctx, c->fmt, c->held, din, (size_t)c->st.held, (size_t)(p.V - p.next.held), (size_t)p.next.held));
    c->st = p.next;
    HZ_TRY(st.finish());
    if (frames_written) *frames_written = F_;
    return HZSDR_OK;
}

template <class F> int frames_for(const F *c, size_t n_in, size_t *frames) {
    if (!c || !frames) return HZSDR_ERR_INVALID_ARGUMENT;
    const ppp::Step p = ppp::step(c->st, c->M, c->L, c->D, n_in);
    if (!p.ok) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("the push is too long"));
    *frames = (size_t)p.F;
    return HZSDR_OK;
}

template <class F> int pending(const F *c, size_t *samples_held, uint64_t *frame_index) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (samples_held) *samples_held = (size_t)c->st.held;
    if (frame_index) *frame_index = c->st.frame;
    return HZSDR_OK;
}

template <class F> int reset(F *c) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    // (the held buffers are only read behind a later push's own writes: nothing to clear, nothing to wait for)
    c->st = ppp::State{};
    return HZSDR_OK;
}

}  // namespace pp
}  // namespace hz
