// hz_tuner.hip -- the tuner bank (include/hzsdr_tuner.h): y_k[m] = rot(w_k m D) * sum_q G_k[q] c(x[m D - q]) for K
// tuners in one pass over the input.  The sum is a float32 matrix product on v_mfma_f32_16x16x4_f32 -- A (2K x 2Qp, the
// modulated taps in MFMA operand order, device memory, made at create and on retune) times B (2Qp x outputs, the
// windows behind every D-th sample) -- the rotator is hz_tuner_math.h (shared with tests/host/tuner_ref.cpp), the host
// arithmetic (counts, phase words, tiles, chunks, both layouts) is hz_tuner_plan.h.
//
// One kernel.  A workgroup of four waves takes T outputs times tile_rows rows of A.  It stages the tile's window of
// (T - 1) D + cq samples, converted in the loads -- from the held samples below the push's first one, +0 at and past
// its last -- into LDS as two planes, each transposed by D (transposed_slot), so that the 16 lanes of one k of a
// B-operand read, samples D apart, are 16 consecutive floats, and the re and im halves of a 32-lane group fall on
// disjoint banks (plane pitch 16 mod 32).  A wave holds 2 x 2 accumulators (32 rows x 32 outputs): per k-step two
// coalesced loads of A, two LDS reads of B and four MFMAs.  Where the window of the whole filter is past the LDS budget
// the inner dimension is staged in chunks of cq taps and the accumulators carry through them: the order of the terms,
// and so the bits, are the same.  The epilogue forms the phase word of every output in wrapping uint32 arithmetic,
// rotates and stores one complex64 per (k, m).
// make NO_PK_F32=1 (csrc/Makefile): no packed float32 instruction in this unit's device code, as in hz_firmm.hip
#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_tuner.h"
#include "hz_tuner_math.h"
#include "hz_tuner_plan.h"

struct hzsdr_tuner {
    hzsdr_ctx *ctx;
    int fmt;
    uint32_t K, D, Q;
    hz::tp::Geom g{};
    uint64_t magic = 0;
    std::vector<float> h;            // the Qp taps, +0 behind Q
    std::vector<uint32_t> words, step, phase;  // per tuner: w, (w D) mod 2^32, the running word of the next output
    std::vector<hz::tn::c32> G;      // K rows of Qp modulated taps
    std::vector<hz::tn::c32> tab;    // T2, T1, T0
    std::vector<float> a_host;       // A in operand order
    float *a_dev = nullptr;
    hz::tn::c32 *tab_dev = nullptr;
    uint32_t *step_dev = nullptr, *phase_dev = nullptr;
    float2 *tail[2] = {nullptr, nullptr};  // the Q - 1 converted samples before the next push: read one, write the other
    int tcur = 0;
    hz::tp::State st{};
};

namespace hz {

struct TunArgs {
    const void *in;
    const float2 *tail;  // the H samples before the push's first
    const float *A;
    const uint32_t *phase, *step;
    const tn::c32 *tab;
    uint64_t n_in, count;  // samples in the push; outputs per row to write
    size_t out_stride;
    uint64_t magic;
    uint32_t D, H, K, rel, steps, cq, chunks, J, plane, window;
};

// The samples around a 64-bit scalar base: at(u) is the converted sample at relative index base + u: +0 below the held
// samples, the held samples below the push's first sample, +0 at and past its last.  Per lane: three compares.
template <int FMT> struct TunSrc {
    using RT = typename Raw<FMT>::t;
    const RT *x;        // the input, moved by base
    const float2 *old;  // the held samples, moved by H + base
    uint32_t z, lo, hi; // u < z: before the held samples; u < lo: held; u < hi: the push; hi <= u: behind the push
    __device__ __forceinline__ TunSrc(const TunArgs &a, int64_t base) {
        x = (const RT *)a.in + base;
        old = a.tail + ((int64_t)a.H + base);
        const int64_t cap = 0x7fffffff;
        auto clamp = [&](int64_t v) { return v <= 0 ? 0u : v > cap ? (uint32_t)cap : (uint32_t)v; };
        z = clamp(-(int64_t)a.H - base);
        lo = clamp(-base);
        hi = clamp((int64_t)a.n_in - base);
        if (hi < lo) hi = lo;  // (an empty push: nothing between the held samples and the end)
    }
    __device__ __forceinline__ float2 at(uint32_t u) const {
        if (u < z || u >= hi) return make_float2(0.0f, 0.0f);
        return u < lo ? old[u] : Raw<FMT>::cvt(x[u]);
    }
};

typedef float tun_f4 __attribute__((ext_vector_type(4)));

// WO: waves along the outputs (T = 32 WO); the other 4 / WO lie along the rows
template <int FMT, int WO>
__global__ __launch_bounds__(tp::kThreads) void tuner_tile_kernel(TunArgs a, float2 *__restrict__ out) {
    constexpr uint32_t T = WO * tp::kWaveOutputs;
    constexpr uint32_t kRowTilesPerGroup = (tp::kThreads / 64 / WO) * (tp::kWaveRows / 16);
    extern __shared__ __align__(16) unsigned char tun_lds[];
    float *win = (float *)tun_lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t wo = wave % WO, wr = wave / WO;
    const uint32_t n = lane & 15u, kk = lane >> 4;
    const uint32_t rt0 = blockIdx.y * kRowTilesPerGroup + wr * (tp::kWaveRows / 16);
    const bool active = rt0 * 8u < a.K;  // (a row tile holds 8 tuners; the tiles of A behind 2K are zero)
    const uint32_t ml = wo * tp::kWaveOutputs + n;  // the lane's output of column tile 0; + 16: of column tile 1

    tun_f4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = tun_f4{0.0f, 0.0f, 0.0f, 0.0f};

    // the lane's first B sample of a chunk: w = ml D + (cq - 1) - (kk >> 1), then two samples down per k-step
    const uint32_t w0 = ml * a.D + (a.cq - 1u) - (kk >> 1);
    [[maybe_unused]] const uint32_t col0 = div_by_magic(w0, a.magic), row0 = w0 - col0 * a.D;
    const uint32_t dec = 2u % a.D, cdec = 2u / a.D;
    [[maybe_unused]] const uint32_t down = dec * a.J + cdec, wrap = a.D * a.J - 1u;
    [[maybe_unused]] const float *bp = win + (kk & 1u) * a.plane;
    [[maybe_unused]] const float *ap = a.A + (size_t)rt0 * a.steps * 64 + lane;
    [[maybe_unused]] const size_t a_tile = (size_t)a.steps * 64;

    for (uint32_t c = 0; c < a.chunks; c++) {
        if (c) __syncthreads();
        {
            const TunSrc<FMT> src(a, tp::tuner_window_base(a.rel, a.D, T, a.cq, blockIdx.x, c));
            for (uint32_t w = tid; w < a.window; w += tp::kThreads) {
                const float2 v = src.at(w);
                const uint32_t j = div_by_magic(w, a.magic);
                const uint32_t s = (w - j * a.D) * a.J + j;
                win[s] = v.x;
                win[a.plane + s] = v.y;
            }
        }
        __syncthreads();
        if (!active) continue;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t s0 = c * (a.cq / 2u);
        const uint32_t s1 = s0 + a.cq / 2u < a.steps ? s0 + a.cq / 2u : a.steps;
        uint32_t row = row0, off = row0 * a.J + col0;
        for (uint32_t s = s0; s < s1; s++) {
            const float a0 = ap[(size_t)s * 64], a1 = ap[a_tile + (size_t)s * 64];
            const float b0 = bp[off], b1 = bp[off + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
            if (row < dec) {
                row += a.D;
                off += wrap;
            }
            row -= dec;
            off -= down;
        }
#endif
    }
    if (!active) return;

    // D layout: column lane & 15, row (lane >> 4) * 4 + reg: registers (0, 1) and (2, 3) are (re, im) of two tuners
    const uint64_t m0 = (uint64_t)blockIdx.x * T + wo * tp::kWaveOutputs;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int hh = 0; hh < 2; hh++) {
            const uint32_t k = (rt0 + i) * 8u + kk * 2u + hh;
            if (k >= a.K) continue;
            const uint32_t p0 = a.phase[k], st = a.step[k];
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const uint64_t mo = m0 + j * 16 + n;
                if (mo >= a.count) continue;
                const tn::c32 s{acc[i][j][2 * hh], acc[i][j][2 * hh + 1]};
                const tn::c32 y = tn::tuner_rotate(s, tp::phase_advance(p0, st, mo), a.tab);
                out[(size_t)k * a.out_stride + mo] = make_float2(y.re, y.im);
            }
        }
}

// Behind a push: the samples held for the next one, the last H of held ++ convert(in), and the running phase words
// advanced by the push's outputs.
template <int FMT>
__global__ __launch_bounds__(tp::kThreads) void tuner_tail_kernel(TunArgs a, float2 *__restrict__ tail_out, uint32_t *__restrict__ phase) {
    const uint32_t p = blockIdx.x * tp::kThreads + threadIdx.x;
    const TunSrc<FMT> src(a, (int64_t)a.n_in - (int64_t)a.H);
    if (p < a.H) tail_out[p] = src.at(p);
    if (blockIdx.x == 0 && threadIdx.x < a.K) phase[threadIdx.x] = tp::phase_advance(phase[threadIdx.x], a.step[threadIdx.x], a.count);
}

template <int FMT>
static int tun_launch_fmt(hzsdr_tuner *t, const TunArgs &a, float2 *out) {
    const dim3 grid((unsigned)((a.count + t->g.T - 1) / t->g.T), (2 * t->K + t->g.tile_rows - 1) / t->g.tile_rows), block(tp::kThreads);
    const size_t lds = t->g.lds_bytes;
    hipStream_t stream = t->ctx->stream;
    if (t->g.waves_out == 4)
        HZ_TRY(launch_fv(tuner_tile_kernel<FMT, 4>, grid, block, lds, stream, a, out));
    else if (t->g.waves_out == 2)
        HZ_TRY(launch_fv(tuner_tile_kernel<FMT, 2>, grid, block, lds, stream, a, out));
    else
        HZ_TRY(launch_fv(tuner_tile_kernel<FMT, 1>, grid, block, lds, stream, a, out));
    HZ_HIP(t->ctx, hipGetLastError());
    return HZSDR_OK;
}

static int tun_launch(hzsdr_tuner *t, const TunArgs &a, float2 *out) {
    return with_format(t->fmt, [&](auto f) { return tun_launch_fmt<decltype(f)::value>(t, a, out); });
}

static int tun_tail(hzsdr_tuner *t, const TunArgs &a) {
    const dim3 grid((a.H + tp::kThreads - 1) / tp::kThreads + (a.H == 0));
    with_format(t->fmt, [&](auto f) {
        hipLaunchKernelGGL(tuner_tail_kernel<decltype(f)::value>, grid, dim3(tp::kThreads), 0, t->ctx->stream, a, t->tail[t->tcur ^ 1], t->phase_dev);
    });
    HZ_HIP(t->ctx, hipGetLastError());
    return HZSDR_OK;
}

static size_t tun_tail_bytes(const hzsdr_tuner *t) { return (size_t)(t->Q > 1 ? t->Q - 1 : 1) * sizeof(float2); }

static TunArgs tun_args(const hzsdr_tuner *t, const void *in, uint64_t n_in, uint64_t count, size_t out_stride) {
    return TunArgs{in, t->tail[t->tcur], t->a_dev, t->phase_dev, t->step_dev, t->tab_dev, n_in, count, out_stride, t->magic,
                   t->D, tp::tuner_held(t->Q), t->K, t->st.rel, t->g.steps, t->g.cq, t->g.chunks, t->g.J, t->g.plane, t->g.window};
}

// step 1 for tuner k, and its two rows of A
static void tun_modulate(hzsdr_tuner *t, uint32_t k) {
    const uint32_t Qp = t->g.Qp, w = t->words[k];
    t->step[k] = tp::phase_step(w, t->D);
    for (uint32_t q = 0; q < Qp; q++) {
        const tn::c32 g = q < t->Q ? tn::tuner_tap(t->h[q], w, q) : tn::c32{0.0f, 0.0f};
        t->G[(size_t)k * Qp + q] = g;
        t->a_host[tp::tuner_a_index(2 * k, 2 * q, t->g.steps)] = g.re;
        t->a_host[tp::tuner_a_index(2 * k, 2 * q + 1, t->g.steps)] = -g.im;
        t->a_host[tp::tuner_a_index(2 * k + 1, 2 * q, t->g.steps)] = g.im;
        t->a_host[tp::tuner_a_index(2 * k + 1, 2 * q + 1, t->g.steps)] = g.re;
    }
}

// the words, steps and A of tuners [first, first + count) to the device, and every running phase word for output m
static int tun_upload(hzsdr_tuner *t, uint32_t first, uint32_t count) {
    hzsdr_ctx *ctx = t->ctx;
    for (uint32_t k = 0; k < t->K; k++) t->phase[k] = tp::phase_at(t->step[k], t->st.m);
    const size_t tile = (size_t)t->g.steps * 64, r0 = 2 * first / 16, r1 = (2 * (first + count) - 1) / 16 + 1;
    HZ_HIP(ctx, hipMemcpyAsync(t->a_dev + r0 * tile, t->a_host.data() + r0 * tile, (r1 - r0) * tile * sizeof(float), hipMemcpyHostToDevice,
                               ctx->stream));
    HZ_HIP(ctx, hipMemcpyAsync(t->step_dev, t->step.data(), t->K * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HZ_HIP(ctx, hipMemcpyAsync(t->phase_dev, t->phase.data(), t->K * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the host copies change with the next retune)
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_tuner_create(hzsdr_ctx *ctx, int src_format, const uint32_t *words, size_t tuners, size_t down, const float *taps,
                       size_t n_taps, hzsdr_tuner **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "tuner: unknown source format");
    if (tuners == 0 || tuners > tp::kMaxTuners) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: 1 ... 256 tuners");
    if (down == 0 || down > tp::kMaxDown) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: down is 1 ... 256");
    if (!words) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: null words");
    if (!taps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: null taps");
    if (n_taps == 0 || n_taps > tp::kMaxTaps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: 1 ... 1024 taps");
    HZ_TRY(check_taps_finite(ctx, "tuner", taps, n_taps));
    HZ_TRY(enter(ctx));
    hzsdr_tuner *t = new hzsdr_tuner{ctx, src_format, (uint32_t)tuners, (uint32_t)down, (uint32_t)n_taps};
    t->g = tp::tuner_geom(t->K, t->D, t->Q);
    t->magic = div_magic(t->D);
    t->h.assign(t->g.Qp, 0.0f);
    for (size_t q = 0; q < n_taps; q++) t->h[q] = taps[q];
    t->words.assign(words, words + tuners);
    t->step.assign(tuners, 0);
    t->phase.assign(tuners, 0);
    t->G.assign(tuners * t->g.Qp, tn::c32{0.0f, 0.0f});
    t->a_host.assign(t->g.a_floats, 0.0f);
    t->tab.resize(tn::kTables);
    for (uint32_t i = 0; i < tn::kT2; i++) t->tab[i] = tn::tuner_table(i, 21);
    for (uint32_t i = 0; i < tn::kT1; i++) t->tab[tn::kT2 + i] = tn::tuner_table(i, 10);
    for (uint32_t i = 0; i < tn::kT0; i++) t->tab[tn::kT2 + tn::kT1 + i] = tn::tuner_table(i, 0);
    for (uint32_t k = 0; k < t->K; k++) tun_modulate(t, k);
    auto undo = [&](int rc) {
        hzsdr_tuner_free(t);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&t->a_dev, t->g.a_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&t->tab_dev, tn::kTables * sizeof(tn::c32));
    if (e == hipSuccess) e = hipMalloc((void **)&t->step_dev, tuners * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&t->phase_dev, tuners * sizeof(uint32_t));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&t->tail[i], tun_tail_bytes(t));
    if (e == hipSuccess) e = hipMemcpyAsync(t->tab_dev, t->tab.data(), tn::kTables * sizeof(tn::c32), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->tail[0], 0, tun_tail_bytes(t), ctx->stream);
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "tuner_create", __FILE__, __LINE__));
    const int rc = tun_upload(t, 0, t->K);
    if (rc != HZSDR_OK) return undo(rc);
    *out = t;
    return HZSDR_OK;
}

int hzsdr_tuner_outputs_for(const hzsdr_tuner *t, size_t n_in, size_t *count) {
    if (!t || !count) return HZSDR_ERR_INVALID_ARGUMENT;
    const hz::tp::Step p = hz::dp::demod_step(t->st, t->D, t->Q, n_in);
    if (!p.ok) return hz::fail(t->ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: the push is too long");
    *count = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_tuner_push(hzsdr_tuner *t, const void *in, size_t n_in, void *out, size_t out_cap, size_t out_stride, size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = t->ctx;
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: null input");
    const tp::Step p = dp::demod_step(t->st, t->D, t->Q, n_in);
    if (!p.ok) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: the push is too long");
    HZ_TRY(check_rows_out(ctx, "tuner", t->K, out, out_cap, out_stride, p.count, t->g.T));
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t ostride;
    HZ_TRY(st.in(0, in, n_in * (size_t)format_size(t->fmt), &din));
    HZ_TRY(st.out_rows(1, out, t->K, (size_t)p.count, out_stride, sizeof(float2), &dout, &ostride));
    const TunArgs a = tun_args(t, din, n_in, p.count, ostride);
    if (p.count) HZ_TRY(tun_launch(t, a, (float2 *)dout));
    HZ_TRY(tun_tail(t, a));
    t->tcur ^= 1;
    t->st = p.next;
    for (uint32_t k = 0; k < t->K; k++) t->phase[k] = tp::phase_advance(t->phase[k], t->step[k], p.count);
    HZ_TRY(st.finish());
    if (written) *written = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_tuner_flush(hzsdr_tuner *t, void *out, size_t out_cap, size_t out_stride, size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = t->ctx;
    const uint64_t count = dp::demod_flush_count(t->st, t->D, t->Q);
    HZ_TRY(check_rows_out(ctx, "tuner", t->K, out, out_cap, out_stride, count, t->g.T));
    HZ_TRY(enter(ctx));
    if (count) {
        Stage st(ctx);
        void *dout;
        size_t ostride;
        HZ_TRY(st.out_rows(1, out, t->K, (size_t)count, out_stride, sizeof(float2), &dout, &ostride));
        // (a push of no samples: every sample at or past the push's first reads as zero)
        HZ_TRY(tun_launch(t, tun_args(t, nullptr, 0, count, ostride), (float2 *)dout));
        HZ_TRY(st.finish());
    }
    HZ_TRY(hzsdr_tuner_reset(t));
    if (written) *written = (size_t)count;
    return HZSDR_OK;
}

int hzsdr_tuner_pending(const hzsdr_tuner *t, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs) {
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    if (consumed) *consumed = t->st.n;
    if (next_output) *next_output = t->st.m;
    if (flush_outputs) *flush_outputs = (size_t)hz::dp::demod_flush_count(t->st, t->D, t->Q);
    return HZSDR_OK;
}

int hzsdr_tuner_plan(const hzsdr_tuner *t, size_t *tile_outputs, size_t *tile_rows, int *form) {
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    if (tile_outputs) *tile_outputs = t->g.T;
    if (tile_rows) *tile_rows = t->g.tile_rows;
    if (form) *form = (t->g.chunks > 1 ? HZSDR_TUNER_FORM_CHUNKED : 0) | (t->D > 1 ? HZSDR_TUNER_FORM_TRANSPOSED : 0);
    return HZSDR_OK;
}

int hzsdr_tuner_set_words(hzsdr_tuner *t, size_t first, size_t count, const uint32_t *words) {
    using namespace hz;
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    if (first > t->K || count > t->K - first) return fail(t->ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: the range is outside the bank");
    if (count && !words) return fail(t->ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: null words");
    HZ_TRY(enter(t->ctx));
    if (count == 0) return HZSDR_OK;
    // (the pushes in flight read A, the steps and the phase words: behind them)
    HZ_HIP(t->ctx, hipStreamSynchronize(t->ctx->stream));
    for (size_t i = 0; i < count; i++) {
        t->words[first + i] = words[i];
        tun_modulate(t, (uint32_t)(first + i));
    }
    return tun_upload(t, (uint32_t)first, (uint32_t)count);
}

int hzsdr_tuner_readout(const hzsdr_tuner *t, int what, size_t index, void *dst, size_t cap) {
    using namespace hz;
    if (!t || !dst) return HZSDR_ERR_INVALID_ARGUMENT;
    const tn::c32 *src;
    size_t n;
    switch (what) {
    case HZSDR_TUNER_READ_TAPS:
        if (index >= t->K) return fail(t->ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: no such tuner");
        src = t->G.data() + index * t->g.Qp, n = t->g.Qp;
        break;
    case HZSDR_TUNER_READ_T2: src = t->tab.data(), n = tn::kT2; break;
    case HZSDR_TUNER_READ_T1: src = t->tab.data() + tn::kT2, n = tn::kT1; break;
    case HZSDR_TUNER_READ_T0: src = t->tab.data() + tn::kT2 + tn::kT1, n = tn::kT0; break;
    default: return fail(t->ctx, HZSDR_ERR_INVALID_ARGUMENT, "tuner: unknown read-out");
    }
    if (cap < n) return fail(t->ctx, HZSDR_ERR_DST_TOO_SMALL, "tuner: the read-out buffer is too small");
    memcpy(dst, src, n * sizeof(tn::c32));
    return HZSDR_OK;
}

int hzsdr_tuner_reset(hzsdr_tuner *t) {
    using namespace hz;
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(t->ctx));
    // (the held samples the next push reads and the phase words, zeroed behind whatever still reads or writes them)
    HZ_HIP(t->ctx, hipMemsetAsync(t->tail[t->tcur], 0, tun_tail_bytes(t), t->ctx->stream));
    HZ_HIP(t->ctx, hipMemsetAsync(t->phase_dev, 0, t->K * sizeof(uint32_t), t->ctx->stream));
    std::fill(t->phase.begin(), t->phase.end(), 0u);
    t->st = tp::State{};
    return HZSDR_OK;
}

int hzsdr_tuner_free(hzsdr_tuner *t) {
    if (!t) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(t->ctx, {t->a_dev, t->tab_dev, t->step_dev, t->phase_dev, t->tail[0], t->tail[1]});
    delete t;
    return HZSDR_OK;
}

}  // extern "C"

#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
