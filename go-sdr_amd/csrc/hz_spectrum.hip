// hz_spectrum.hip -- the fused power spectrum (include/hzsdr_spectrum.h): frames of a raw IQ stream converted and
// windowed in the loads, transformed by the workgroup core of hz_fftv.h, |X|^2 summed per bin over `avg` frames in
// frame order, scaled, written in the requested order and kind.  One pass over the raw samples; the frame that is not
// complete yet (converted complex64), the samples still to skip and the partial row's sums stay on the device.
//
// Two kernel forms, bit-identical by construction (the same staging, the same transform, the same bin_power, the same
// float32 sums in the same order):
//   * ROW WALK (spectrum_rows_kernel): a transform group owns one row and walks its frames in order, the next frame's
//     raw loads in flight under the current transform, the row's sums in registers (a lane keeps its sixteen bins);
//   * FRAME PARALLEL (spectrum_frames_kernel + spectrum_sum_kernel): every frame of a chunk on its own transform group,
//     p_j to scratch; then one thread per (row, bin) sums the chunk's frames in order into the row accumulators that
//     carry a partial row from chunk to chunk and from push to push.  For few rows of many frames.
#include "hz_chain_host.h"
#include "../../include/hzsdr_spectrum.h"
#include "hz_polyphase.h"

struct hzsdr_spectrum {
    hzsdr_ctx *ctx;
    int fmt;
    size_t n, hop, avg;
    float scale;
    int order, output;
    int form = HZSDR_SPECTRUM_FORM_AUTO, last_form = 0;
    hz::fv::FvTabs tabs{};
    float *win = nullptr;                 // n window values (ones for a rectangular window)
    hz::pp::Held tail;                    // the samples held for the next frame, converted: read one, write the other
    float *acc[2] = {nullptr, nullptr};   // the partial row's float32 sums per bin (ZeroFirst), likewise
    int acur = 0;
    size_t held = 0, skip = 0, frames = 0;  // samples held, samples still to skip, frames summed into the open row
    float *scratch = nullptr;             // frame-parallel p_j, grow-only
    size_t scratch_cap = 0;
};

namespace hz {

// what a push of m samples does, computed on the host before anything is launched
struct SpecStep {
    size_t s0;        // leading samples of the push that fall into a skip gap
    size_t L;         // samples of the virtual buffer: held ++ in[s0 ..)
    size_t F;         // frames that complete in the push
    size_t rows;      // rows that complete in the push
    size_t new_held, new_skip, new_frames;
};

static SpecStep spec_step(const hzsdr_spectrum *s, size_t m) {
    SpecStep p{};
    p.s0 = std::min(s->skip, m);
    p.L = s->held + (m - p.s0);
    p.F = p.L >= s->n ? (p.L - s->n) / s->hop + 1 : 0;
    const size_t next = p.F * s->hop;  // virtual index of the next frame's first sample
    if (s->skip > m) {
        p.new_held = 0;
        p.new_skip = s->skip - m;
    } else if (next <= p.L) {
        p.new_held = p.L - next;
        p.new_skip = 0;
    } else {
        p.new_held = 0;
        p.new_skip = next - p.L;
    }
    const size_t total = s->frames + p.F;
    p.rows = total / s->avg;
    p.new_frames = total % s->avg;
    return p;
}

// The frames of one launch.  Frame j (0-based within the push) starts at virtual index j*hop of
// V = tail[0 .. held) ++ convert(in[0 ..)), `in` already past the skipped samples.
struct SpecArgs {
    const void *in;
    const float2 *tail;
    size_t held, hop, F;
    const float *win;
    const cf4 *tab;
};

// |X|^2 of one bin: THE expression every kernel form evaluates (no contraction: two rounded products, one rounded sum)
__device__ __forceinline__ float bin_power(cf x) { return __fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y)); }

// a row's value of one bin: scale * sum, as power or as dB (float64 log10, rounded once)
__device__ __forceinline__ float spec_value(float acc, float scale, bool db) {
    const float p = __fmul_rn(scale, acc);
    return db ? (float)(10.0 * log10((double)p)) : p;
}

// output position of ZeroFirst bin k (FrequencySlice.Shift, fft/result.go:82-97)
__device__ __forceinline__ unsigned spec_pos(unsigned k, unsigned n, bool neg_first) { return neg_first ? (k + n / 2) & (n - 1) : k; }

// converted, windowed sample `i` of V
template <int FMT> __device__ __forceinline__ cf spec_sample(const SpecArgs &a, size_t i, float w) {
    using R = typename Raw<FMT>::t;
    const float2 x = i < a.held ? a.tail[i] : Raw<FMT>::cvt(((const R *)a.in)[i - a.held]);
    return fv::from2(x) * w;
}

// frame j into the first pass's edge layout (any frame: from the tail and / or the input)
template <int N, int FMT> __device__ __forceinline__ void spec_load(cf *v, const SpecArgs &a, const float *w, size_t j, int lane) {
    constexpr int R0 = fv::first_radix(N);
    const size_t base = j * a.hop + lane;
#pragma unroll
    for (int q = 0; q < 16; q++) v[q] = spec_sample<FMT>(a, base + fv::edge_off<N, R0>(q), w[q]);
}

template <int N> __device__ __forceinline__ void spec_window(float *w, const float *win, int lane) {
    constexpr int R0 = fv::first_radix(N);
#pragma unroll
    for (int q = 0; q < 16; q++) w[q] = win[fv::edge_off<N, R0>(q) + lane];
}

// the transform: one wave per transform up to N = 1024 (the wave orders its own LDS operations), a workgroup beyond
template <int N> __device__ __forceinline__ void spec_forward(cf *v, cf *lds, const cf4 *tab, int lane) {
    fv::forward<N, false, (fv::tpt(N) <= 64)>(v, lds, tab, lane);
}

// ROW WALK: row r (0-based within the push) sums frames j = r*K - f0 + t, t in [0, K), that lie in [0, F).
// The rows' trip ranges are made uniform per workgroup (several rows share a wave below N = 1024).
template <int N, int FMT>
__global__ __launch_bounds__(fv::block(N)) void spectrum_rows_kernel(SpecArgs a, size_t nrows, size_t f0, size_t K,
                                                                     const float *__restrict__ acc_in, float *__restrict__ acc_out,
                                                                     float *__restrict__ out, float scale, int neg_first, int db) {
    constexpr int TPT = fv::tpt(N), XPB = fv::xpb(N), R0 = fv::first_radix(N);
    using RT = typename Raw<FMT>::t;
    const int sub = XPB == 1 ? 0 : threadIdx.x / TPT, lane = XPB == 1 ? (int)threadIdx.x : threadIdx.x % TPT;
    cf *lds = fv_lds() + sub * fv::lds_elems(N);
    const size_t r0 = (size_t)blockIdx.x * XPB, r = r0 + sub;
    const bool live_row = r < nrows;
    const size_t r_last = std::min(r0 + XPB, nrows) - 1;
    // t in [t_begin, t_end): the union of the block's rows' ranges (only row 0 starts late, only the last row ends early)
    const size_t t_begin = f0 > r_last * K ? f0 - r_last * K : 0;
    const size_t t_end = std::min(K, f0 + a.F - r0 * K);
    float w[16], acc[16];
    spec_window<N>(w, a.win, lane);
#pragma unroll
    for (int q = 0; q < 16; q++) acc[q] = (live_row && r == 0 && f0 > 0) ? acc_in[lane + q * TPT] : 0.f;
    auto frame_of = [&](size_t t) -> int64_t { return (int64_t)(r * K + t) - (int64_t)f0; };
    auto from_input = [&](int64_t j) { return live_row && j >= 0 && (size_t)j < a.F && (size_t)j * a.hop >= a.held; };
    // raw loads of a frame that lies wholly in the input, one trip ahead (loads return in order: the table reads of the
    // transform queue behind them, as in conv_blocks_kernel16; the frame's own conversion waits for nothing else)
    RT nx[16];
    auto prefetch = [&](int64_t j) {
        const RT *p = (const RT *)a.in + ((size_t)j * a.hop - a.held) + lane;
#pragma unroll
        for (int q = 0; q < 16; q++) nx[q] = p[fv::edge_off<N, R0>(q)];
    };
    if (t_begin < t_end && from_input(frame_of(t_begin))) prefetch(frame_of(t_begin));
    cf v[16];
#pragma unroll 1
    for (size_t t = t_begin; t < t_end; t++) {
        const int64_t j = frame_of(t);
        const bool live = live_row && j >= 0 && (size_t)j < a.F;
        if (from_input(j)) {
#pragma unroll
            for (int q = 0; q < 16; q++) v[q] = fv::from2(Raw<FMT>::cvt(nx[q])) * w[q];
        } else {
            spec_load<N, FMT>(v, a, w, live ? (size_t)j : 0, lane);  // (dead rows transform frame 0 and drop it)
        }
        if (t + 1 < t_end && from_input(j + 1)) prefetch(j + 1);
        // the last pass of the previous frame read the LDS with no barrier behind it (several waves per transform)
        if constexpr (fv::block(N) > 64) __syncthreads();
        spec_forward<N>(v, lds, a.tab, lane);
        if (live) {
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = acc[q] + bin_power(v[q]);
        }
    }
    if (!live_row) return;
    if ((r + 1) * K <= f0 + a.F) {
        float *o = out + r * N;
#pragma unroll
        for (int q = 0; q < 16; q++) o[spec_pos(lane + q * TPT, N, neg_first)] = spec_value(acc[q], scale, db);
    } else {
#pragma unroll
        for (int q = 0; q < 16; q++) acc_out[lane + q * TPT] = acc[q];
    }
}

// FRAME PARALLEL, first half: p_j for frames c0 .. c0 + nfr - 1 into scratch (frame-major, ZeroFirst bins)
template <int N, int FMT>
__global__ __launch_bounds__(fv::block(N)) void spectrum_frames_kernel(SpecArgs a, size_t c0, size_t nfr, float *__restrict__ scratch) {
    constexpr int TPT = fv::tpt(N), XPB = fv::xpb(N);
    const int sub = XPB == 1 ? 0 : threadIdx.x / TPT, lane = XPB == 1 ? (int)threadIdx.x : threadIdx.x % TPT;
    cf *lds = fv_lds() + sub * fv::lds_elems(N);
    const size_t f = (size_t)blockIdx.x * XPB + sub;
    const bool live = f < nfr;
    float w[16];
    spec_window<N>(w, a.win, lane);
    cf v[16];
    spec_load<N, FMT>(v, a, w, c0 + (live ? f : 0), lane);
    spec_forward<N>(v, lds, a.tab, lane);
    if (live) {
        float *o = scratch + f * N + lane;
#pragma unroll
        for (int q = 0; q < 16; q++) o[q * TPT] = bin_power(v[q]);
    }
}

// FRAME PARALLEL, second half: one thread per (row, bin) of the chunk; frames j = r*K - f0 + t of the chunk in order
__global__ __launch_bounds__(kThreads) void spectrum_sum_kernel(const float *__restrict__ scratch, size_t nfr, size_t n, size_t nrows,
                                                                size_t f0, size_t K, const float *__restrict__ acc_in,
                                                                float *__restrict__ acc_out, float *__restrict__ out, float scale,
                                                                int neg_first, int db) {
    const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= nrows * n) return;
    const size_t r = idx / n, k = idx % n;
    const size_t j0 = r * K > f0 ? r * K - f0 : 0, j1 = std::min(nfr, (r + 1) * K - f0);
    float acc = (r == 0 && f0 > 0) ? acc_in[k] : 0.f;
    const float *p = scratch + k;
#pragma unroll 8
    for (size_t j = j0; j < j1; j++) acc = acc + p[j * n];
    if ((r + 1) * K <= f0 + nfr) out[r * n + spec_pos((unsigned)k, (unsigned)n, neg_first)] = spec_value(acc, scale, db);
    else acc_out[k] = acc;
}

// frame-parallel chunk: p_j of at most this many float32 values in scratch at once
constexpr size_t kSpecChunkFloats = (size_t)1 << 23;

template <int N, int FMT>
static int spec_launch_n(hzsdr_spectrum *s, const SpecArgs &a, float *out, int form) {
    hzsdr_ctx *ctx = s->ctx;
    constexpr int XPB = fv::xpb(N);
    const dim3 block(fv::block(N));
    const size_t lds = (size_t)XPB * fv::lds_elems(N) * sizeof(cf);
    const size_t K = s->avg, f0 = s->frames;
    const int neg = s->order == HZSDR_ORDER_NEGATIVE_FIRST, db = s->output == HZSDR_SPECTRUM_DB;
    if (form == HZSDR_SPECTRUM_FORM_ROW_WALK) {
        const size_t nrows = (f0 + a.F - 1) / K + 1;  // rows the push touches
        HZ_TRY(launch_fv(spectrum_rows_kernel<N, FMT>, dim3((unsigned)((nrows + XPB - 1) / XPB)), block, lds, ctx->stream, a, nrows, f0,
                         K, (const float *)s->acc[s->acur], s->acc[s->acur ^ 1], out, s->scale, neg, db));
        HZ_HIP(ctx, hipGetLastError());
        s->acur ^= 1;
        return HZSDR_OK;
    }
    const size_t chunk = std::max<size_t>(1, kSpecChunkFloats / N);
    const size_t want = std::min(chunk, a.F) * N * sizeof(float);
    if (s->scratch_cap < want) {
        if (s->scratch) {
            HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
            HZ_HIP(ctx, hipFree(s->scratch));
            s->scratch = nullptr;
            s->scratch_cap = 0;
        }
        HZ_HIP(ctx, hipMalloc((void **)&s->scratch, want));
        s->scratch_cap = want;
    }
    size_t fc = f0;  // frames of the open row before the chunk
    float *o = out;
    for (size_t c0 = 0; c0 < a.F; c0 += chunk) {
        const size_t nfr = std::min(chunk, a.F - c0);
        HZ_TRY(launch_fv(spectrum_frames_kernel<N, FMT>, dim3((unsigned)((nfr + XPB - 1) / XPB)), block, lds, ctx->stream, a, c0, nfr,
                         s->scratch));
        const size_t nrows = (fc + nfr - 1) / K + 1, done = (fc + nfr) / K;
        const size_t items = nrows * N;
        hipLaunchKernelGGL(spectrum_sum_kernel, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                           (const float *)s->scratch, nfr, (size_t)N, nrows, fc, K, (const float *)s->acc[s->acur], s->acc[s->acur ^ 1], o,
                           s->scale, neg, db);
        HZ_HIP(ctx, hipGetLastError());
        s->acur ^= 1;
        o += done * N;
        fc = (fc + nfr) % K;
    }
    return HZSDR_OK;
}

// Auto: the row walk as long as the rows give every SIMD of the chip a wave of their own (a row is TPT lanes), the
// frames dealt across the grid otherwise (few rows of many frames: the row walk would leave the chip idle).
static int spec_pick_form(const hzsdr_spectrum *s, size_t F) {
    if (s->form != HZSDR_SPECTRUM_FORM_AUTO) return s->form;
    const size_t nrows = (s->frames + F - 1) / s->avg + 1;
    const size_t lanes = nrows * (s->n / 16), chip = (size_t)s->ctx->num_cus * 4 * 64;
    return lanes >= chip ? HZSDR_SPECTRUM_FORM_ROW_WALK : HZSDR_SPECTRUM_FORM_FRAME_PARALLEL;
}

}  // namespace hz

extern "C" {

int hzsdr_spectrum_create(hzsdr_ctx *ctx, int src_format, size_t n, size_t hop, size_t avg, const float *window, float scale,
                          int order, int output, hzsdr_spectrum **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "spectrum: unknown source format");
    if (n < 256 || n > 8192 || (n & (n - 1)) != 0)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: the transform length is a power of two, 256 ... 8192");
    if (hop == 0 || avg == 0) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: hop and avg are at least 1");
    if (order != HZSDR_ORDER_ZERO_FIRST && order != HZSDR_ORDER_NEGATIVE_FIRST)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: unknown fft order");
    if (output != HZSDR_SPECTRUM_POWER && output != HZSDR_SPECTRUM_DB)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: unknown output kind");
    HZ_TRY(enter(ctx));
    hzsdr_spectrum *s = new hzsdr_spectrum{ctx, src_format, n, hop, avg, scale, order, output};
    auto undo = [&](int rc) {
        hzsdr_spectrum_free(s);
        return rc;
    };
    int rc = get_fv_tables(ctx, n, &s->tabs);  // (plan-time: the transform's tables, not inside the first push)
    if (rc != HZSDR_OK) return undo(rc);
    std::vector<float> w(n, 1.f);
    if (window) std::copy(window, window + n, w.begin());
    hipError_t e = hipMalloc((void **)&s->win, n * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&s->tail.buf[i], n * sizeof(float2));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&s->acc[i], n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(s->win, w.data(), n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (w is a host vector of this frame)
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "spectrum_create", __FILE__, __LINE__));
    *out = s;
    return HZSDR_OK;
}

int hzsdr_spectrum_rows_for(const hzsdr_spectrum *s, size_t n_in, size_t *rows) {
    if (!s || !rows) return HZSDR_ERR_INVALID_ARGUMENT;
    *rows = hz::spec_step(s, n_in).rows;
    return HZSDR_OK;
}

int hzsdr_spectrum_push(hzsdr_spectrum *s, const void *in, size_t n_in, float *out, size_t out_rows_cap, size_t *rows_written) {
    using namespace hz;
    if (rows_written) *rows_written = 0;
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = s->ctx;
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: null input");
    const SpecStep p = spec_step(s, n_in);
    if (out_rows_cap < p.rows) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "spectrum: output buffer too small for the rows of the push");
    if (p.rows && !out) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: null output");
    HZ_TRY(enter(ctx));
    const size_t fs = (size_t)format_size(s->fmt), mp = n_in - p.s0;
    if (mp == 0) {  // (nothing but a skip gap, or nothing at all)
        s->skip = p.new_skip;
        return HZSDR_OK;
    }
    Stage st(ctx);
    const void *din;
    void *dout = nullptr;
    HZ_TRY(st.in(0, (const char *)in + p.s0 * fs, mp * fs, &din));
    if (p.rows) HZ_TRY(st.out(1, out, p.rows * s->n * sizeof(float), &dout));
    const SpecArgs a{din, s->tail.now(), s->held, s->hop, p.F, s->win, s->tabs.fwd};
    if (p.F) {
        const int form = spec_pick_form(s, p.F);
        HZ_TRY(with_format(s->fmt, [&](auto f) {
            return pp::with_fv_size(s->n, [&](auto n) { return spec_launch_n<decltype(n)::value, decltype(f)::value>(s, a, (float *)dout, form); });
        }));
        s->last_form = form;
    }
    HZ_TRY(pp::keep(ctx, s->fmt, s->tail, din, a.held, p.L - p.new_held, p.new_held));
    s->held = p.new_held;
    s->skip = p.new_skip;
    s->frames = p.new_frames;
    HZ_TRY(st.finish());
    if (rows_written) *rows_written = p.rows;
    return HZSDR_OK;
}

int hzsdr_spectrum_pending(const hzsdr_spectrum *s, size_t *frames_in_row, size_t *samples_held) {
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    if (frames_in_row) *frames_in_row = s->frames;
    if (samples_held) *samples_held = s->held;
    return HZSDR_OK;
}

int hzsdr_spectrum_options(hzsdr_spectrum *s, int form) {
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    if (form != HZSDR_SPECTRUM_FORM_AUTO && form != HZSDR_SPECTRUM_FORM_ROW_WALK && form != HZSDR_SPECTRUM_FORM_FRAME_PARALLEL)
        return hz::fail(s->ctx, HZSDR_ERR_INVALID_ARGUMENT, "spectrum: unknown kernel form");
    s->form = form;
    return HZSDR_OK;
}

int hzsdr_spectrum_last_form(const hzsdr_spectrum *s, int *form) {
    if (!s || !form) return HZSDR_ERR_INVALID_ARGUMENT;
    *form = s->last_form;
    return HZSDR_OK;
}

int hzsdr_spectrum_reset(hzsdr_spectrum *s) {
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    // (the device buffers are only read behind a later push's own writes: nothing to clear, nothing to wait for)
    s->held = s->skip = s->frames = 0;
    return HZSDR_OK;
}

int hzsdr_spectrum_free(hzsdr_spectrum *s) {
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(s->ctx, {s->win, s->tail.buf[0], s->tail.buf[1], s->acc[0], s->acc[1], s->scratch});
    delete s;
    return HZSDR_OK;
}

}  // extern "C"
