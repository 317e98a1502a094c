// hz_resampler.hip -- the polyphase rational resampler (include/hzsdr_resampler.h): y[m] = sum_q h[phi_m + q U] *
// c(x[i_m - q]) over one or many rows, a time-domain polyphase FIR with a per-output phase.  The host arithmetic
// (counts, the running phase, tiles, the reciprocal of U, the kernel's shape) is hz_resampler_plan.h.
//
// One kernel, a handful of forms.  A workgroup of 256 lanes takes one tile of T consecutive outputs of one row (the row is
// the grid's second dimension).  It stages the tile's input window, floor((phi_tile + (T - 1) D) / U) + Q samples
// converted in the loads, in LDS -- or, in the DIRECT form (D/U so large that the window of 256 outputs is past the
// budget), every lane reads its samples from memory.  At D/U >= 2 the window is stored with one empty slot behind every
// 32 samples (rs::resampler_slot), which takes the lanes' 8-byte reads off each other's banks.  The polyphase table hp[phi][q] is copied to LDS beside the
// window -- or, past the budget, read from memory (TAPS_GLOBAL); where U divides D every output has phase 0 and the one
// row is read as wave-uniform scalars instead (TAPS_UNIFORM).  A lane owns T / 256 outputs, 256 apart, as
// independent chains; its (i, phi) comes from one multiplication with the reciprocal of U and is stepped by
// add-and-carry.  The Q - 1 converted samples behind a push stay with the object (two buffers, read one, write the
// other), zero at create and reset; samples behind the last one pushed read as zero, which is all a flush needs.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_resampler.h"
#include "hz_resampler_plan.h"

struct hzsdr_resampler {
    hzsdr_ctx *ctx;
    int fmt;
    uint32_t U, D, L, Q, R;
    hz::rs::Geom g{};
    uint64_t magic = 0;
    float *hp = nullptr;                   // the polyphase table, U rows of g.pitch floats
    float2 *tail[2] = {nullptr, nullptr};  // R rows of Q - 1 converted samples: read one, write the other
    int tcur = 0;
    hz::rs::State st{};
};

namespace hz {

// one term of the sum: THE expression every path evaluates (one fused multiply-add per component)
__device__ __forceinline__ float2 res_term(float2 acc, float h, float2 x) { return make_float2(__fmaf_rn(h, x.x, acc.x), __fmaf_rn(h, x.y, acc.y)); }

struct ResArgs {
    const void *in;      // row s starts s * in_stride samples in
    size_t in_stride;
    const float2 *tail;  // row s: the Q - 1 samples before the push's first
    const float *hp;
    uint64_t n_in, count;  // samples per row in the push; outputs per row to write
    size_t out_stride;
    uint64_t magic;
    uint32_t U, D, Q, pitch, rel, phi, step_i, step_phi;
};

// The samples of one row around a 64-bit scalar base: at(w) is the converted sample at relative index jb + w, from the
// held tail below the push's first sample, +0 at and past its last.  Per lane: a 32-bit offset and two compares.
template <int FMT> struct ResSrc {
    using RT = typename Raw<FMT>::t;
    const RT *x;        // the row, moved by jb
    const float2 *old;  // the row's tail, moved by Q - 1 + jb
    uint32_t lo, hi;    // w < lo: the tail; lo <= w < hi: the push; hi <= w: zero
    __device__ __forceinline__ ResSrc(const ResArgs &a, size_t s, int64_t jb) {
        x = (const RT *)a.in + (int64_t)(s * a.in_stride) + jb;
        old = a.tail + (int64_t)(s * (a.Q - 1)) + (int64_t)(a.Q - 1) + jb;
        lo = jb < 0 ? (uint32_t)(-jb) : 0u;  // (jb >= -(Q - 1))
        const int64_t left = (int64_t)a.n_in - jb;
        hi = left <= 0 ? 0u : left > 0x7fffffff ? 0x7fffffffu : (uint32_t)left;
        if (hi < lo) hi = lo;  // (an empty push: nothing between the tail and the zeros)
    }
    __device__ __forceinline__ float2 at(uint32_t w) const {
        if (w < lo) return old[w];
        if (w < hi) return Raw<FMT>::cvt(x[w]);
        return make_float2(0.f, 0.f);
    }
};

// UNI (U divides D: every output has phase 0): TGLOBAL with the row offset a constant 0, so that the taps are loads from a
// wave-uniform address, scalar registers, and the LDS carries the samples alone.
template <int FMT, int R, bool DIRECT, bool TGLOBAL, bool PAD, bool UNI = false>
__global__ __launch_bounds__(rs::kThreads) void resampler_tile_kernel(ResArgs a, float2 *__restrict__ out) {
    constexpr uint32_t T = R * rs::kThreads;
    extern __shared__ __align__(16) unsigned char res_lds[];
    const uint32_t tid = threadIdx.x;
    const size_t s = blockIdx.y;
    const rs::Tile t = rs::resampler_tile(a.rel, a.phi, a.U, a.D, a.Q, T, blockIdx.x);
    const ResSrc<FMT> src(a, s, (int64_t)t.i0 - (int64_t)(a.Q - 1));
    // LDS: the table (U * pitch floats, a multiple of 16 bytes), then the window
    float *tab_lds = (float *)res_lds;
    float2 *win = (float2 *)(res_lds + (TGLOBAL ? 0 : (size_t)a.U * a.pitch * sizeof(float)));
    if constexpr (!TGLOBAL) {
        const uint32_t n4 = a.U * a.pitch / 4;
        for (uint32_t i = tid; i < n4; i += rs::kThreads) ((float4 *)tab_lds)[i] = ((const float4 *)a.hp)[i];
    }
    if constexpr (!DIRECT)
        for (uint32_t w = tid; w < t.window; w += rs::kThreads) win[rs::resampler_slot(w, PAD)] = src.at(w);
    if constexpr (!TGLOBAL || !DIRECT) __syncthreads();
    const float *tab = TGLOBAL ? a.hp : tab_lds;

    // chain r of the lane is output tid + r * 256 of the tile: its newest sample is window index ci + Q - 1
    uint32_t ci[R], cphi[R];
    {
        const uint32_t u = t.phi + tid * a.D;
        uint32_t i = div_by_magic(u, a.magic), phi = u - i * a.U;
#pragma unroll
        for (int r = 0; r < R; r++) {
            ci[r] = i + (a.Q - 1);
            cphi[r] = UNI ? 0u : phi * a.pitch;
            i += a.step_i;
            phi += a.step_phi;
            if (phi >= a.U) {
                phi -= a.U;
                i++;
            }
        }
    }
    auto sample = [&](uint32_t w) -> float2 {
        if constexpr (DIRECT)
            return src.at(w);
        else
            return win[rs::resampler_slot(w, PAD)];
    };
    float2 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = make_float2(0.f, 0.f);
    uint32_t q = 0;
#pragma unroll 1
    for (; q + 4 <= a.Q; q += 4) {
        float4 h[R];
        float2 x[R][4];
#pragma unroll
        for (int r = 0; r < R; r++) {
            h[r] = *(const float4 *)(tab + cphi[r] + q);
#pragma unroll
            for (int k = 0; k < 4; k++) x[r][k] = sample(ci[r] - q - k);
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            acc[r] = res_term(acc[r], h[r].x, x[r][0]);
            acc[r] = res_term(acc[r], h[r].y, x[r][1]);
            acc[r] = res_term(acc[r], h[r].z, x[r][2]);
            acc[r] = res_term(acc[r], h[r].w, x[r][3]);
        }
        if constexpr (!DIRECT && !TGLOBAL) {
            // (the trip's LDS reads in flight before the first use: channelizer_frames_kernel's note applies)
            __builtin_amdgcn_sched_group_barrier(0x100, 5 * R, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 8 * R, 0);
        }
    }
#pragma unroll 1
    for (; q < a.Q; q++) {
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = res_term(acc[r], tab[cphi[r] + q], sample(ci[r] - q));
    }
    // 8 bytes per lane, contiguous across the lanes
    const uint64_t k0 = (uint64_t)blockIdx.x * T, left = a.count - k0;
    const uint32_t n = left < T ? (uint32_t)left : T;
    float2 *o = out + s * a.out_stride + k0;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (tid + r * rs::kThreads < n) o[tid + r * rs::kThreads] = acc[r];
}

// the samples held for the next push: the last Q - 1 of tail ++ convert(in), row by row
template <int FMT>
__global__ __launch_bounds__(rs::kThreads) void resampler_tail_kernel(ResArgs a, float2 *__restrict__ tail_out) {
    const uint32_t p = blockIdx.x * rs::kThreads + threadIdx.x;
    const size_t s = blockIdx.y;
    const ResSrc<FMT> src(a, s, (int64_t)a.n_in - (int64_t)(a.Q - 1));  // (n_in >= 1: below it, the tail stays)
    if (p < a.Q - 1) tail_out[s * (a.Q - 1) + p] = src.at(p);
}

template <int FMT, int R, bool DIRECT, bool PAD>
static int res_launch_form(hzsdr_resampler *r, const ResArgs &a, float2 *out, dim3 grid) {
    const dim3 block(rs::kThreads);
    if (r->g.taps_global)
        HZ_TRY(launch_fv(resampler_tile_kernel<FMT, R, DIRECT, true, PAD>, grid, block, r->g.lds_bytes, r->ctx->stream, a, out));
    else if (!DIRECT && r->g.taps_uniform)
        HZ_TRY(launch_fv(resampler_tile_kernel<FMT, R, false, true, PAD, true>, grid, block, r->g.lds_bytes, r->ctx->stream, a, out));
    else
        HZ_TRY(launch_fv(resampler_tile_kernel<FMT, R, DIRECT, false, PAD>, grid, block, r->g.lds_bytes, r->ctx->stream, a, out));
    HZ_HIP(r->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int FMT>
static int res_launch_fmt(hzsdr_resampler *r, const ResArgs &a, float2 *out) {
    const dim3 grid((unsigned)((a.count + r->g.T - 1) / r->g.T), r->R);
    if (r->g.direct) return res_launch_form<FMT, 1, true, false>(r, a, out, grid);
    if (r->g.T == (uint32_t)rs::kThreads)
        return r->g.pad ? res_launch_form<FMT, 1, false, true>(r, a, out, grid) : res_launch_form<FMT, 1, false, false>(r, a, out, grid);
    return r->g.pad ? res_launch_form<FMT, 4, false, true>(r, a, out, grid) : res_launch_form<FMT, 4, false, false>(r, a, out, grid);
}

static int res_launch(hzsdr_resampler *r, const ResArgs &a, float2 *out) {
    return with_format(r->fmt, [&](auto f) { return res_launch_fmt<decltype(f)::value>(r, a, out); });
}

static int res_tail(hzsdr_resampler *r, const ResArgs &a) {
    const dim3 grid((r->Q - 1 + rs::kThreads - 1) / rs::kThreads, r->R);
    with_format(r->fmt, [&](auto f) {
        hipLaunchKernelGGL(resampler_tail_kernel<decltype(f)::value>, grid, dim3(rs::kThreads), 0, r->ctx->stream, a, r->tail[r->tcur ^ 1]);
    });
    HZ_HIP(r->ctx, hipGetLastError());
    return HZSDR_OK;
}

static size_t res_tail_bytes(const hzsdr_resampler *r) { return (size_t)r->R * std::max<size_t>(r->Q - 1, 1) * sizeof(float2); }

static ResArgs res_args(const hzsdr_resampler *r, const void *in, size_t in_stride, uint64_t n_in, uint64_t count, size_t out_stride) {
    return ResArgs{in, in_stride, r->tail[r->tcur], r->hp, n_in, count, out_stride, r->magic, r->U, r->D, r->Q, r->g.pitch,
                   r->st.rel, r->st.phi, r->g.step_i, r->g.step_phi};
}

}  // namespace hz

extern "C" {

int hzsdr_resampler_create(hzsdr_ctx *ctx, int src_format, size_t up, size_t down, const float *taps, size_t n_taps, size_t streams,
                           hzsdr_resampler **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "resampler: unknown source format");
    if (up == 0 || up > rs::kMaxRate || down == 0 || down > rs::kMaxRate)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: up and down are 1 ... 1024");
    if (!taps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: null taps");
    if (n_taps == 0 || n_taps > rs::kMaxTaps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: 1 ... 65536 taps");
    const size_t q = (n_taps + up - 1) / up;
    if (q > rs::kMaxPhaseTaps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: at most 256 taps per phase (ceil(n_taps / up))");
    if (streams == 0 || streams > rs::kMaxStreams) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: 1 ... 8192 streams");
    HZ_TRY(check_taps_finite(ctx, "resampler", taps, n_taps));
    HZ_TRY(enter(ctx));
    hzsdr_resampler *r = new hzsdr_resampler{ctx, src_format, (uint32_t)up, (uint32_t)down, (uint32_t)n_taps, (uint32_t)q, (uint32_t)streams};
    r->g = rs::resampler_geom(r->U, r->D, r->Q);
    r->magic = div_magic(r->U);
    auto undo = [&](int rc) {
        hzsdr_resampler_free(r);
        return rc;
    };
    // hp[phi][q] = h[phi + q U], +0 past L and in the pitch's padding (never read)
    std::vector<float> hp((size_t)r->U * r->g.pitch, 0.0f);
    for (size_t k = 0; k < n_taps; k++) hp[(k % up) * r->g.pitch + k / up] = taps[k];
    hipError_t e = hipMalloc((void **)&r->hp, hp.size() * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&r->tail[i], res_tail_bytes(r));
    if (e == hipSuccess) e = hipMemcpyAsync(r->hp, hp.data(), hp.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(r->tail[0], 0, res_tail_bytes(r), ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (hp is a local: gone when create returns)
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "resampler_create", __FILE__, __LINE__));
    *out = r;
    return HZSDR_OK;
}

int hzsdr_resampler_outputs_for(const hzsdr_resampler *r, size_t n_in, size_t *count) {
    if (!r || !count) return HZSDR_ERR_INVALID_ARGUMENT;
    const hz::rs::Step p = hz::rs::resampler_step(r->st, r->U, r->D, r->Q, n_in);
    if (!p.ok) return hz::fail(r->ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: the push is too long");
    *count = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_resampler_push(hzsdr_resampler *r, const void *in, size_t n_in, size_t in_stride, void *out, size_t out_cap, size_t out_stride,
                         size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = r->ctx;
    const size_t R = r->R, fs = (size_t)format_size(r->fmt);
    if (n_in && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: null input");
    if (R > 1 && in_stride < n_in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: in_stride is below the samples of the push");
    const rs::Step p = rs::resampler_step(r->st, r->U, r->D, r->Q, n_in);
    if (!p.ok) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "resampler: the push is too long");
    HZ_TRY(check_rows_out(ctx, "resampler", R, out, out_cap, out_stride, p.count, r->g.T));
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout;
    size_t dstride, ostride;
    HZ_TRY(st.in_rows(0, in, R, n_in, in_stride, fs, &din, &dstride));
    HZ_TRY(st.out_rows(1, out, R, (size_t)p.count, out_stride, sizeof(float2), &dout, &ostride));
    const ResArgs a = res_args(r, din, dstride, n_in, p.count, ostride);
    if (p.count) HZ_TRY(res_launch(r, a, (float2 *)dout));
    if (r->Q > 1) {
        HZ_TRY(res_tail(r, a));
        r->tcur ^= 1;
    }
    r->st = p.next;
    HZ_TRY(st.finish());
    if (written) *written = (size_t)p.count;
    return HZSDR_OK;
}

int hzsdr_resampler_flush(hzsdr_resampler *r, void *out, size_t out_cap, size_t out_stride, size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = r->ctx;
    const uint64_t count = rs::resampler_flush_count(r->st, r->U, r->D, r->L);
    HZ_TRY(check_rows_out(ctx, "resampler", r->R, out, out_cap, out_stride, count, r->g.T));
    HZ_TRY(enter(ctx));
    if (count) {
        Stage st(ctx);
        void *dout;
        size_t ostride;
        HZ_TRY(st.out_rows(1, out, r->R, (size_t)count, out_stride, sizeof(float2), &dout, &ostride));
        // (a push of no samples: every index at or past the push's first reads as zero)
        HZ_TRY(res_launch(r, res_args(r, nullptr, 0, 0, count, ostride), (float2 *)dout));
        HZ_TRY(st.finish());
    }
    HZ_TRY(hzsdr_resampler_reset(r));
    if (written) *written = (size_t)count;
    return HZSDR_OK;
}

int hzsdr_resampler_pending(const hzsdr_resampler *r, uint64_t *consumed, uint64_t *next_output, size_t *flush_outputs) {
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    if (consumed) *consumed = r->st.n;
    if (next_output) *next_output = r->st.m;
    if (flush_outputs) *flush_outputs = (size_t)hz::rs::resampler_flush_count(r->st, r->U, r->D, r->L);
    return HZSDR_OK;
}

int hzsdr_resampler_plan(const hzsdr_resampler *r, size_t *tile_outputs, int *form) {
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    if (tile_outputs) *tile_outputs = r->g.T;
    if (form)
        *form = (r->g.direct ? HZSDR_RESAMPLER_FORM_DIRECT : 0) | (r->g.taps_global ? HZSDR_RESAMPLER_FORM_TAPS_GLOBAL : 0) |
                (r->g.taps_uniform ? HZSDR_RESAMPLER_FORM_TAPS_UNIFORM : 0) | (r->g.pad ? HZSDR_RESAMPLER_FORM_WINDOW_PADDED : 0);
    return HZSDR_OK;
}

int hzsdr_resampler_reset(hzsdr_resampler *r) {
    using namespace hz;
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(r->ctx));
    // (the tail the next push reads, zeroed behind whatever still reads or writes it on the context's stream)
    HZ_HIP(r->ctx, hipMemsetAsync(r->tail[r->tcur], 0, res_tail_bytes(r), r->ctx->stream));
    r->st = rs::State{};
    return HZSDR_OK;
}

int hzsdr_resampler_free(hzsdr_resampler *r) {
    if (!r) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(r->ctx, {r->hp, r->tail[0], r->tail[1]});
    delete r;
    return HZSDR_OK;
}

}  // extern "C"
