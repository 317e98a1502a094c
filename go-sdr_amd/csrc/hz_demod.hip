// hz_demod.hip -- the demodulator bank (include/hzsdr_demod.h): d[n] = FM, phase, envelope or power of c(x[n]), then
// y[m] = sum_q h[q] * d[m D - q], over one or many rows.  The arithmetic of every output is hz_demod_math.h (shared with
// the host restatement of tests/host/demod_ref.cpp); the host arithmetic (counts, tiles, the window's layout, the
// kernel's shape) is hz_demod_plan.h.
//
// One kernel.  A workgroup of 256 lanes takes one tile of T consecutive outputs of one row (the row is the grid's second
// dimension).  It computes the tile's (T - 1) D + Q detector values ONCE, from (T - 1) D + Q + 1 raw samples converted
// in the loads -- from the held tail below the push's first sample, +0 at and past its last -- and stores each as one
// float in LDS, transposed (transposed_slot: value w in row w mod D), so that the lanes of a read, D values apart, sit
// on consecutive banks.  A lane then owns T / 256 outputs, 256 apart, as independent fma chains; from tap to tap the
// slot moves by a step that is the same for every lane (scalar work), and the chains of a lane are a constant 256
// floats apart (an immediate offset).  h[q] is read from a wave-uniform address: scalar registers, never lane by lane.
// The Q converted samples behind a push stay with the object (two buffers, read one, write the other), zero at create
// and reset; d itself is never kept.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_demod.h"
#include "hz_demod_math.h"
#include "hz_demod_plan.h"

struct hzsdr_demod {
    hzsdr_ctx *ctx;
    int fmt, mode;
    uint32_t D, Q, R;
    hz::dp::Geom g{};
    uint64_t magic = 0;
    float *h = nullptr;                    // the Q taps, padded with +0 to a multiple of 8
    float2 *tail[2] = {nullptr, nullptr};  // R rows of Q converted samples: read one, write the other
    int tcur = 0;
    hz::dp::State st{};
};

namespace hz {

struct DemArgs {
    const void *in;      // row s starts s * in_stride samples in
    size_t in_stride;
    const float2 *tail;  // row s: the Q samples before the push's first
    const float *h;
    uint64_t n_in, count;  // samples per row in the push; outputs per row to write
    size_t out_stride;
    uint64_t magic;
    uint32_t D, Q, J, rel, row0, slot0;
    int mode;
};

// The samples of one row around a 64-bit scalar base: at(u) is the converted sample at relative index jb + u, from the
// held tail below the push's first sample; indices at and past `hi` are behind the push's last.  Per lane: a 32-bit
// offset and two compares.
template <int FMT> struct DemSrc {
    using RT = typename Raw<FMT>::t;
    const RT *x;        // the row, moved by jb
    const float2 *old;  // the row's tail, moved by Q + jb
    uint32_t lo, hi;    // u < lo: the tail; lo <= u < hi: the push; hi <= u: behind the push
    __device__ __forceinline__ DemSrc(const DemArgs &a, size_t s, int64_t jb) {
        x = (const RT *)a.in + (int64_t)(s * a.in_stride) + jb;
        old = a.tail + (int64_t)(s * a.Q) + (int64_t)a.Q + jb;
        lo = jb < 0 ? (uint32_t)(-jb) : 0u;  // (jb >= -Q)
        const int64_t left = (int64_t)a.n_in - jb;
        hi = left <= 0 ? 0u : left > 0x7fffffff ? 0x7fffffffu : (uint32_t)left;
        if (hi < lo) hi = lo;  // (an empty push: nothing between the tail and the end)
    }
    // (u < hi)
    __device__ __forceinline__ dm::c32 at(uint32_t u) const {
        const float2 v = u < lo ? old[u] : Raw<FMT>::cvt(x[u]);
        return dm::c32{v.x, v.y};
    }
};

// HALF: T = 128, the upper two waves leave after the window is full
template <int FMT, int R, bool HALF>
__global__ __launch_bounds__(dp::kThreads) void demod_tile_kernel(DemArgs a, float *__restrict__ out) {
    constexpr uint32_t T = HALF ? dp::kThreads / 2 : R * dp::kThreads;
    extern __shared__ __align__(16) unsigned char dem_lds[];
    float *win = (float *)dem_lds;
    const uint32_t tid = threadIdx.x;
    const size_t s = blockIdx.y;
    const dp::Tile t = dp::demod_tile(a.rel, a.D, a.Q, T, blockIdx.x);
    // raw sample u = w + 1 is the own sample of window value w, u - 1 the one before it
    const DemSrc<FMT> src(a, s, (int64_t)t.i0 - (int64_t)a.Q);
    for (uint32_t w = tid; w < t.window; w += dp::kThreads) {
        float d = 0.0f;  // at and behind the push's last sample
        if (w + 1 < src.hi) {
            const dm::c32 x1 = src.at(w + 1);
            const dm::c32 x0 = a.mode == dm::kFm ? src.at(w) : dm::c32{0.0f, 0.0f};
            d = dm::demod_detect(a.mode, x1, x0);
        }
        const uint32_t j = div_by_magic(w, a.magic);
        win[(w - j * a.D) * a.J + j] = d;
    }
    __syncthreads();
    if (HALF && tid >= T) return;

    // chain r of the lane is output tid + r * 256 of the tile; its newest value is window index (tid + r * 256) D + Q - 1,
    // slot0 + tid + r * 256, and from tap to tap every chain moves by the same step
    const float *wl = win + tid;
    uint32_t row = a.row0, off = a.slot0;
    const uint32_t up = (a.D - 1) * a.J - 1;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0f;
    uint32_t q = 0;
#pragma unroll 1
    for (; q + 8 <= a.Q; q += 8) {
        const float4 h0 = *(const float4 *)(a.h + q), h1 = *(const float4 *)(a.h + q + 4);
        const float h[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
        float x[8][R];
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
            for (int r = 0; r < R; r++) x[k][r] = wl[off + r * dp::kThreads];
            if (row == 0) {
                row = a.D - 1;
                off += up;
            } else {
                row--;
                off -= a.J;
            }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
#pragma unroll
            for (int r = 0; r < R; r++) acc[r] = dm::demod_term(acc[r], h[k], x[k][r]);
        }
    }
#pragma unroll 1
    for (; q < a.Q; q++) {
        const float h = a.h[q];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = dm::demod_term(acc[r], h, wl[off + r * dp::kThreads]);
        if (row == 0) {
            row = a.D - 1;
            off += up;
        } else {
            row--;
            off -= a.J;
        }
    }
    // 4 bytes per lane, contiguous across the lanes
    const uint64_t k0 = (uint64_t)blockIdx.x * T, left = a.count - k0;
    const uint32_t n = left < T ? (uint32_t)left : T;
    float *o = out + s * a.out_stride + k0;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (tid + r * dp::kThreads < n) o[tid + r * dp::kThreads] = acc[r];
}

// the samples held for the next push: the last Q of tail ++ convert(in), row by row
template <int FMT>
__global__ __launch_bounds__(dp::kThreads) void demod_tail_kernel(DemArgs a, float2 *__restrict__ tail_out) {
    const uint32_t p = blockIdx.x * dp::kThreads + threadIdx.x;
    const size_t s = blockIdx.y;
    const DemSrc<FMT> src(a, s, (int64_t)a.n_in - (int64_t)a.Q);  // (n_in >= 1; every p < Q is below hi = Q)
    if (p < a.Q) {
        const dm::c32 v = src.at(p);
        tail_out[s * a.Q + p] = make_float2(v.re, v.im);
    }
}

template <int FMT>
static int dem_launch_fmt(hzsdr_demod *d, const DemArgs &a, float *out) {
    const dim3 grid((unsigned)((a.count + d->g.T - 1) / d->g.T), d->R), block(dp::kThreads);
    const size_t lds = d->g.lds_bytes;
    hipStream_t stream = d->ctx->stream;
    if (d->g.half)
        HZ_TRY(launch_fv(demod_tile_kernel<FMT, 1, true>, grid, block, lds, stream, a, out));
    else if (d->g.T == 4u * dp::kThreads)
        HZ_TRY(launch_fv(demod_tile_kernel<FMT, 4, false>, grid, block, lds, stream, a, out));
    else if (d->g.T == 2u * dp::kThreads)
        HZ_TRY(launch_fv(demod_tile_kernel<FMT, 2, false>, grid, block, lds, stream, a, out));
    else
        HZ_TRY(launch_fv(demod_tile_kernel<FMT, 1, false>, grid, block, lds, stream, a, out));
    HZ_HIP(d->ctx, hipGetLastError());
    return HZSDR_OK;
}

static int dem_launch(hzsdr_demod *d, const DemArgs &a, float *out) {
    return with_format(d->fmt, [&](auto f) { return dem_launch_fmt<decltype(f)::value>(d, a, out); });
}

static int dem_tail(hzsdr_demod *d, const DemArgs &a) {
    const dim3 grid((d->Q + dp::kThreads - 1) / dp::kThreads, d->R);
    with_format(d->fmt, [&](auto f) {
        hipLaunchKernelGGL(demod_tail_kernel<decltype(f)::value>, grid, dim3(dp::kThreads), 0, d->ctx->stream, a, d->tail[d->tcur ^ 1]);
    });
    HZ_HIP(d->ctx, hipGetLastError());
    return HZSDR_OK;
}

static size_t dem_tail_bytes(const hzsdr_demod *d) { return (size_t)d->R * d->Q * sizeof(float2); }

static DemArgs dem_args(const hzsdr_demod *d, const void *in, size_t in_stride, uint64_t n_in, uint64_t count, size_t out_stride) {
    return DemArgs{in, in_stride, d->tail[d->tcur], d->h, n_in, count, out_stride, d->magic, d->D, d->Q, d->g.J, d->st.rel, d->g.row0, d->g.slot0, d->mode};
}

}  // namespace hz

extern "C" {

int hzsdr_demod_create(hzsdr_ctx *ctx, int src_format, int mode, size_t down, const float *taps, size_t n_taps, size_t streams,
                       hzsdr_demod **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "demod: unknown source format");
    if (mode < HZSDR_DEMOD_FM || mode > HZSDR_DEMOD_POWER) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: unknown mode");
    if (down == 0 || down > dp::kMaxDown) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: down is 1 ... 64");
    if (!taps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: null taps");
    if (n_taps == 0 || n_taps > dp::kMaxTaps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: 1 ... 1024 taps");
    if (streams == 0 || streams > dp::kMaxStreams) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: 1 ... 8192 streams");
    HZ_TRY(check_taps_finite(ctx, "demod", taps, n_taps));
    HZ_TRY(enter(ctx));
    hzsdr_demod *d = new hzsdr_demod{ctx, src_format, mode, (uint32_t)down, (uint32_t)n_taps, (uint32_t)streams};
    d->g = dp::demod_geom(d->D, d->Q);
    d->magic = div_magic(d->D);
    auto undo = [&](int rc) {
        hzsdr_demod_free(d);
        return rc;
    };
    std::vector<float> h((n_taps + 7) / 8 * 8, 0.0f);  // (the padding is never read)
    for (size_t k = 0; k < n_taps; k++) h[k] = taps[k];
    hipError_t e = hipMalloc((void **)&d->h, h.size() * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&d->tail[i], dem_tail_bytes(d));
    if (e == hipSuccess) e = hipMemcpyAsync(d->h, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->tail[0], 0, dem_tail_bytes(d), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (h is a local: gone when create returns)
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "demod_create", __FILE__, __LINE__));
    *out = d;
    return HZSDR_OK;
}

int hzsdr_demod_outputs_for(const hzsdr_demod *d, size_t n_in, size_t *count) {
    if (!d || !count) return HZSDR_ERR_INVALID_ARGUMENT;
    const hz::dp::Step p = hz::dp::demod_step(d->st, d->D, d->Q, n_in);
    if (!p.ok) return hz::fail(d->ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: the push is too long");
    *count = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_demod_push(hzsdr_demod *d, const void *in, size_t n_in, size_t in_stride, float *out, size_t out_cap, size_t out_stride,
                     size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = d->ctx;
    const size_t R = d->R, fs = (size_t)format_size(d->fmt);
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: null input");
    if (R > 1 && in_stride < n_in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: in_stride is below the samples of the push");
    const dp::Step p = dp::demod_step(d->st, d->D, d->Q, n_in);
    if (!p.ok) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "demod: the push is too long");
    HZ_TRY(check_rows_out(ctx, "demod", R, out, out_cap, out_stride, p.count, d->g.T));
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t dstride, ostride;
    HZ_TRY(st.in_rows(0, in, R, n_in, in_stride, fs, &din, &dstride));
    HZ_TRY(st.out_rows(1, out, R, (size_t)p.count, out_stride, sizeof(float), &dout, &ostride));
    const DemArgs a = dem_args(d, din, dstride, n_in, p.count, ostride);
    if (p.count) HZ_TRY(dem_launch(d, a, (float *)dout));
    HZ_TRY(dem_tail(d, a));
    d->tcur ^= 1;
    d->st = p.next;
    HZ_TRY(st.finish());
    if (written) *written = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_demod_flush(hzsdr_demod *d, float *out, size_t out_cap, size_t out_stride, size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = d->ctx;
    const uint64_t count = dp::demod_flush_count(d->st, d->D, d->Q);
    HZ_TRY(check_rows_out(ctx, "demod", d->R, out, out_cap, out_stride, count, d->g.T));
    HZ_TRY(enter(ctx));
    if (count) {
        Stage st(ctx);
        void *dout;
        size_t ostride;
        HZ_TRY(st.out_rows(1, out, d->R, (size_t)count, out_stride, sizeof(float), &dout, &ostride));
        // (a push of no samples: every detector value at or past the push's first sample reads as zero)
        HZ_TRY(dem_launch(d, dem_args(d, nullptr, 0, 0, count, ostride), (float *)dout));
        HZ_TRY(st.finish());
    }
    HZ_TRY(hzsdr_demod_reset(d));
    if (written) *written = (size_t)count;
    return HZSDR_OK;
}

int hzsdr_demod_pending(const hzsdr_demod *d, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    if (consumed) *consumed = d->st.n;
    if (next_output) *next_output = d->st.m;
    if (flush_outputs) *flush_outputs = (size_t)hz::dp::demod_flush_count(d->st, d->D, d->Q);
    return HZSDR_OK;
}

int hzsdr_demod_plan(const hzsdr_demod *d, size_t *tile_outputs, int *form) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    if (tile_outputs) *tile_outputs = d->g.T;
    if (form) *form = (d->g.half ? HZSDR_DEMOD_FORM_HALF_TILE : 0) | (d->D > 1 ? HZSDR_DEMOD_FORM_TRANSPOSED : 0);
    return HZSDR_OK;
}

int hzsdr_demod_reset(hzsdr_demod *d) {
    using namespace hz;
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(d->ctx));
    // (the tail the next push reads, zeroed behind whatever still reads or writes it on the context's stream)
    HZ_HIP(d->ctx, hipMemsetAsync(d->tail[d->tcur], 0, dem_tail_bytes(d), d->ctx->stream));
    d->st = dp::State{};
    return HZSDR_OK;
}

int hzsdr_demod_free(hzsdr_demod *d) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(d->ctx, {d->h, d->tail[0], d->tail[1]});
    delete d;
    return HZSDR_OK;
}

}  // extern "C"
