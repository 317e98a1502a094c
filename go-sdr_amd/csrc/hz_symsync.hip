// hz_symsync.hip -- the symbol-timing recovery bank (include/hzsdr_symsync.h): a Gardner loop around a cubic interpolator
// over R rows, real or complex, soft symbols out at the symbol rate.  The arithmetic of every symbol, count and state
// value is hz_symsync_math.h (shared with the host restatement of tests/host/symsync_ref.cpp); the host arithmetic (rows
// per wave, the two tiles, their address maps, the loop constants, the bound) is hz_symsync_plan.h.
//
// One kernel, a row-wave one: the wave, its sample tile and steps 1 and 2 of a tile are described in hz_rowwave.h,
// which holds the wave's sync, the wait before the loop and the fetch.  Lane l < G keeps its row's loop constants and
// its state in registers from the first tile to the last, reads them from the object's state array before and writes
// them back behind.  Its own:
//   3. the walk: lane = row steps t = 0 ... T - 1, eight samples read ahead of the loop, every step computed without a
//      divergent branch (the lanes' clocks differ: the interpolant and the loop update are predicated) and the symbol,
//      where the step emits one, written into the SYMBOL TILE at the lane's own count k: float k P + lane.  One
//      wave-uniform branch stays where a wave owns ONE row (R <= 1024): a sample without a strobe moves the counter
//      and the samples only;
//   4. the rows' counts and running totals are broadcast from their lanes, and the symbol tile is stored row by row,
//      lane = symbol, 64 at a step, every store guarded by the row's capacity.
// Shared parameters travel in the kernel's arguments: wave-uniform scalars, never lane by lane.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_symsync.h"
#include "hz_symsync_math.h"
#include "hz_symsync_plan.h"
#include "hz_loopbank.h"
#include "hz_rowwave.h"

struct hzsdr_symsync : hz::lb::LoopBank<hz::sm::Loop, float> {  // params: 4 to the set; the state: sp::state_floats, sp::state_index
    static constexpr const char *noun = "symsync";
    int kind = 0;
    hz::sp::Geom g{};
    double amin = 1.0;         // the smallest hmin - g_mu over the rows
    uint32_t *maxw = nullptr;  // the largest count of a push, for a caller who asks
};

namespace hz {

struct SymArgs {
    const void *in;  // row r starts r * in_stride samples in
    size_t in_stride;
    void *out;  // row r's symbols start r * out_stride symbols in
    size_t out_stride, out_cap;
    uint64_t n;  // samples per row in the push
    const sm::Loop *loop_rows;
    float *state;
    uint32_t *counts, *maxw;
    uint32_t R, G, P;
    sm::Loop loop;  // the shared constants
};

template <int PL> struct SymSrc {
    using T = float2;
    static __device__ __forceinline__ void split(float2 v, float (&x)[PL]) { x[0] = v.x, x[PL - 1] = v.y; }
    static __device__ __forceinline__ float2 pack(float re, float im) { return make_float2(re, im); }
};
template <> struct SymSrc<1> {
    using T = float;
    static __device__ __forceinline__ void split(float v, float (&x)[1]) { x[0] = v; }
    static __device__ __forceinline__ float pack(float re, float) { return re; }
};

// one sample into the lane's row; its symbol, where there is one, into the lane's next slot of the symbol tile.  The
// flag alternates whatever the data, so cnt stays below Y (sp::tile_symbols); the comparison costs one instruction and
// keeps the write inside the tile whatever a state array brought in.
template <int PL, bool IDLE>
__device__ __forceinline__ void sym_sample(const float (&x)[PL], float *sy, uint32_t P, uint32_t Y, const sm::Loop &k, sm::State<PL> &s, uint32_t &cnt) {
    // IDLE: no lane of the wave has a strobe in this sample (wave-uniform: the lanes stay together): only the counters
    // and the samples move.  With one row per wave that is sps - 2 samples of every sps; with eight rows whose clocks
    // differ it is next to none (0.6^8 of the samples at 5 per symbol), and the branch only cuts the walk into blocks
    // (what was measured of both, and what was not: DESIGN.md section 4).
    if (IDLE && __builtin_amdgcn_ballot_w64(s.c < 1.0f) == 0) {
        sm::sync_idle<PL>(s, x);
        return;
    }
    float y[PL];
    const bool emit = sm::sync_step<PL>(s, k, x, y);
    if (emit && cnt < Y) {
#pragma unroll
        for (int p = 0; p < PL; p++) sy[sp::emit_slot(0, cnt, p, P, Y)] = y[p];
        cnt++;
    }
}

// lane = row: samples [0, tn) of the tile through the loop -> the symbols emitted.  Eight samples are read before the
// steps that consume them, so that no LDS latency sits on the loop-carried path.
template <int PL, bool IDLE>
__device__ __forceinline__ uint32_t sym_walk(const float *tl, float *sy, uint32_t P, uint32_t T, uint32_t Y, uint32_t tn, const sm::Loop &k,
                                             sm::State<PL> &s) {
    uint32_t cnt = 0, t = 0;
#pragma unroll 1
    for (; t + 8 <= tn; t += 8) {
        float x[8][PL];
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int p = 0; p < PL; p++) x[j][p] = tl[sp::walk_slot(0, t + j, p, P, T)];
#pragma unroll
        for (int j = 0; j < 8; j++) sym_sample<PL, IDLE>(x[j], sy, P, Y, k, s, cnt);
    }
#pragma unroll 1
    for (; t < tn; t++) {
        float x[PL];
#pragma unroll
        for (int p = 0; p < PL; p++) x[p] = tl[sp::walk_slot(0, t, p, P, T)];
        sym_sample<PL, IDLE>(x, sy, P, Y, k, s, cnt);
    }
    return cnt;
}

template <int PL, int K, bool PER_ROW, bool IDLE>
__global__ __launch_bounds__(sp::kLanes) void symsync_rows_kernel(SymArgs a) {
    using Src = SymSrc<PL>;
    using ST = typename Src::T;
    constexpr uint32_t T = sp::kLanes * K, Y = sp::tile_symbols(T);
    extern __shared__ __align__(16) unsigned char symsync_lds[];
    float *tile = (float *)symsync_lds;
    float *syms = tile + PL * T * a.P;  // (Geom::sym_base)
    const auto [lane, row0, g, own, row] = rw::wave(a);

    sm::Loop k = a.loop;
    sm::State<PL> s{};
    if (own) {
        if (PER_ROW) k = a.loop_rows[row];
        const float *z = a.state + row * sp::state_row_floats(PL);
        s.c = z[sp::kStC];
        s.h = z[sp::kStH];
        s.flag = z[sp::kStFlag] != 0.0f ? 1u : 0u;
#pragma unroll
        for (int p = 0; p < PL; p++) {
            s.yp[p] = z[sp::state_index(0, sp::kStYp, p, PL)];
            s.ym[p] = z[sp::state_index(0, sp::kStYm, p, PL)];
            s.x1[p] = z[sp::state_index(0, sp::kStX1, p, PL)];
            s.x2[p] = z[sp::state_index(0, sp::kStX2, p, PL)];
            s.x3[p] = z[sp::state_index(0, sp::kStX3, p, PL)];
        }
    }

    const ST *in = (const ST *)a.in + (size_t)row0 * a.in_stride;
    ST *out = (ST *)a.out + (size_t)row0 * a.out_stride;
    ST raw[sp::kMaxGroup][K];
    rw::fetch<ST, K>(raw, in, a.in_stride, g, 0, a.n, lane);
    rw::settle(k.g_mu), rw::settle(k.g_omega), rw::settle(k.hmin), rw::settle(k.hmax);
    rw::settle(s.c), rw::settle(s.h), rw::settle(s.flag);
#pragma unroll
    for (int p = 0; p < PL; p++) rw::settle(s.yp[p]), rw::settle(s.ym[p]), rw::settle(s.x1[p]), rw::settle(s.x2[p]), rw::settle(s.x3[p]);

    uint32_t total = 0;  // the lane's row: symbols emitted by the push so far
#pragma unroll 1
    for (uint64_t t0 = 0; t0 < a.n; t0 += T) {
        const uint64_t left = a.n - t0;
        const uint32_t tn = left < T ? (uint32_t)left : T;
        // 1. into the sample tile: row fixed, lane = sample
#pragma unroll
        for (uint32_t r = 0; r < sp::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    if (lane + sp::kLanes * kk < tn) {
                        float x[PL];
                        Src::split(raw[r][kk], x);
#pragma unroll
                        for (int p = 0; p < PL; p++) tile[sp::move_slot(lane, kk, r, p, a.P, T)] = x[p];
                    }
                }
            }
        }
        rw::wave_sync();
        // 2. the next tile's loads, in flight under the walk
        if (left > T) rw::fetch<ST, K>(raw, in, a.in_stride, g, t0 + T, a.n, lane);
        // 3. lane = row
        uint32_t cnt = 0;
        if (own) cnt = sym_walk<PL, IDLE>(tile + lane, syms + lane, a.P, T, Y, tn, k, s);
        rw::wave_sync();
        // 4. out of the symbol tile: row fixed, lane = symbol.  The row's count and total come from its lane; both are
        // wave-uniform, and so is the loop over the steps of 64.
#pragma unroll
        for (uint32_t r = 0; r < sp::kMaxGroup; r++) {
            if (r < g) {
                const uint32_t cr = (uint32_t)__builtin_amdgcn_readlane((int)cnt, (int)r);
                const uint32_t tr = (uint32_t)__builtin_amdgcn_readlane((int)total, (int)r);
                for (uint32_t j = 0; j * sp::kLanes < cr; j++) {
                    const uint32_t i = lane + sp::kLanes * j;
                    const size_t col = (size_t)tr + i;
                    if (i < cr && col < a.out_cap) {  // (the guard that keeps a garbage row inside its capacity)
                        const float re = syms[sp::store_slot(lane, j, r, 0, a.P, Y)];
                        const float im = PL == 2 ? syms[sp::store_slot(lane, j, r, PL - 1, a.P, Y)] : 0.0f;
                        out[r * a.out_stride + col] = Src::pack(re, im);
                    }
                }
            }
        }
        total += cnt;
        rw::wave_sync();  // (the next tile's symbols overwrite these)
    }

    if (own) {
        float *z = a.state + row * sp::state_row_floats(PL);
        z[sp::kStC] = s.c;
        z[sp::kStH] = s.h;
        z[sp::kStFlag] = s.flag ? 1.0f : 0.0f;
#pragma unroll
        for (int p = 0; p < PL; p++) {
            z[sp::state_index(0, sp::kStYp, p, PL)] = s.yp[p];
            z[sp::state_index(0, sp::kStYm, p, PL)] = s.ym[p];
            z[sp::state_index(0, sp::kStX1, p, PL)] = s.x1[p];
            z[sp::state_index(0, sp::kStX2, p, PL)] = s.x2[p];
            z[sp::state_index(0, sp::kStX3, p, PL)] = s.x3[p];
        }
        const uint32_t written = (size_t)total < a.out_cap ? total : (uint32_t)a.out_cap;
        a.counts[row] = written;
        if (a.maxw) atomicMax(a.maxw, written);
    }
}

static bool sym_complex(int kind) { return kind != HZSDR_SYMSYNC_REAL_F32; }
static size_t sym_size(int kind) { return sym_complex(kind) ? sizeof(float2) : sizeof(float); }

template <int PL>
static int sym_launch_kind(hzsdr_symsync *f, const SymArgs &a) {
    constexpr int K = sp::kSteps;  // (the plan's: f->g.K)
    const dim3 grid(f->g.waves), block(sp::kLanes);
    const bool idle = f->g.G == 1;  // one row per wave: the walk skips the samples without a strobe
    if (f->per_row && idle)
        HZ_TRY(launch_fv(symsync_rows_kernel<PL, K, true, true>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else if (f->per_row)
        HZ_TRY(launch_fv(symsync_rows_kernel<PL, K, true, false>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else if (idle)
        HZ_TRY(launch_fv(symsync_rows_kernel<PL, K, false, true>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else
        HZ_TRY(launch_fv(symsync_rows_kernel<PL, K, false, false>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    HZ_HIP(f->ctx, hipGetLastError());
    return HZSDR_OK;
}

// what the bank gives hz_loopbank.h
struct SymBank {
    using Obj = hzsdr_symsync;
    static constexpr size_t kParams = sp::kParams;
    static const char *check_params(const float *p) { return sp::check_params(p); }
    static sm::Loop derive(const float *p) { return sp::derive(p).loop; }
    static int check_kind(hzsdr_ctx *ctx, int kind) {
        if (kind != HZSDR_SYMSYNC_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "symsync: real float32 or complex64 rows");
        return HZSDR_OK;
    }
    static void shape(hzsdr_symsync *f, int kind) {
        f->kind = kind;
        f->g = sp::symsync_geom(f->R, sym_complex(kind));
        f->words = sp::state_floats(f->R, f->g.planes);
    }
    // the initial state: c = 0, h = h0 of the row, flag = 0, everything else +0
    static void initial(const hzsdr_symsync *f, size_t r, size_t set, float *z) {
        z[r * sp::state_row_floats(f->g.planes) + sp::kStH] = sp::derive(f->params.data() + set * kParams).h0;
    }
};

// the bank's own beside its parameters: the smallest advance over the sets the object holds
static void sym_least_advance(hzsdr_symsync *f) {
    double amin = 0.0;
    for (size_t r = 0; r < f->sets(); r++) {
        const double a = sp::least_advance(f->params.data() + r * sp::kParams);
        if (r == 0 || a < amin) amin = a;
    }
    f->amin = amin;
}

}  // namespace hz

extern "C" {

int hzsdr_symsync_create(hzsdr_ctx *ctx, int kind, const float *params, int per_row, size_t rows, hzsdr_symsync **out) {
    using namespace hz;
    HZ_TRY(lb::create<SymBank>(ctx, kind, params, per_row, rows, out));
    hzsdr_symsync *f = *out;
    sym_least_advance(f);
    const hipError_t e = hipMalloc((void **)&f->maxw, sizeof(uint32_t));
    if (e == hipSuccess) return HZSDR_OK;
    *out = nullptr;
    hzsdr_symsync_free(f);
    return hip_fail(ctx, e, "symsync_create", __FILE__, __LINE__);
}

int hzsdr_symsync_max_symbols(const hzsdr_symsync *f, size_t n, size_t *bound) {
    if (!f || !bound) return HZSDR_ERR_INVALID_ARGUMENT;
    *bound = (size_t)hz::sp::max_symbols(n, f->amin);
    return HZSDR_OK;
}

int hzsdr_symsync_push(hzsdr_symsync *f, const void *in, size_t n, size_t in_stride, void *out, size_t out_cap, size_t out_stride,
                       uint32_t *counts, size_t *max_written) {
    using namespace hz;
    if (max_written) *max_written = 0;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R;
    if (n && (!in || !counts)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "symsync: null input or counts");
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "symsync: in_stride is below the samples of the push");
    if (f->pos + n < f->pos || n > 0xfffffff0ull) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "symsync: the push is too long");
    const size_t bound = (size_t)sp::max_symbols(n, f->amin);
    HZ_TRY(check_rows_out(ctx, "symsync", R, out, out_cap, out_stride, bound, 0));
    HZ_TRY(enter(ctx));
    if (n == 0) {  // nothing written for any row
        if (counts && ctx->memspace == HZSDR_MEM_HOST) memset(counts, 0, R * sizeof(uint32_t));
        if (counts && ctx->memspace != HZSDR_MEM_HOST) HZ_HIP(ctx, hipMemsetAsync(counts, 0, R * sizeof(uint32_t), ctx->stream));
        return HZSDR_OK;
    }
    Stage st(ctx);
    const void *din;
    void *dout, *dcounts;
    size_t dstride, ostride = out_stride;
    const size_t size = sym_size(f->kind);
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, size, &din, &dstride));
    // the columns behind a row's count stay as they are: a HOST context's rows go up before they come back
    if (R == 1 || out_stride == bound) {
        HZ_TRY(st.out_preserve(1, out, R * bound * size, &dout));
    } else {
        const void *up;
        HZ_TRY(st.in_rows(1, out, R, bound, out_stride, size, &up, &ostride));
        HZ_TRY(st.out_rows(1, out, R, bound, out_stride, size, &dout, &ostride));
    }
    HZ_TRY(st.out(2, counts, R * sizeof(uint32_t), &dcounts));
    if (max_written) HZ_HIP(ctx, hipMemsetAsync(f->maxw, 0, sizeof(uint32_t), ctx->stream));
    SymArgs a{din, dstride, dout, ostride, bound, n, f->loop_rows, f->state, (uint32_t *)dcounts, max_written ? f->maxw : nullptr,
              f->R, f->g.G, f->g.P, f->loop[0]};
    HZ_TRY(f->g.planes == 2 ? sym_launch_kind<2>(f, a) : sym_launch_kind<1>(f, a));
    f->pos += n;
    HZ_TRY(st.finish());
    if (max_written) {
        uint32_t m = 0;
        HZ_HIP(ctx, hipMemcpyAsync(&m, f->maxw, sizeof m, hipMemcpyDeviceToHost, ctx->stream));
        HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *max_written = m;
    }
    return HZSDR_OK;
}

int hzsdr_symsync_set_params(hzsdr_symsync *f, const float *params) {
    HZ_TRY(hz::lb::set_params<hz::SymBank>(f, params));
    hz::sym_least_advance(f);
    return HZSDR_OK;
}

int hzsdr_symsync_get_state(hzsdr_symsync *f, float *state, size_t cap) { return hz::lb::get_state(f, state, cap); }

int hzsdr_symsync_set_state(hzsdr_symsync *f, const float *state, size_t count, uint64_t position) {
    return hz::lb::set_state(f, state, count, position, "the state has rows * 8 (complex rows: 13) floats");
}

int hzsdr_symsync_position(const hzsdr_symsync *f, uint64_t *position) { return hz::lb::position(f, position); }

int hzsdr_symsync_plan(const hzsdr_symsync *f, size_t *rows_per_wave, size_t *tile_samples, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    return hz::lb::plan(f, rows_per_wave, tile_samples, form,
                        (f->per_row ? HZSDR_SYMSYNC_FORM_PER_ROW : 0) | (f->g.planes == 2 ? HZSDR_SYMSYNC_FORM_COMPLEX : 0));
}

int hzsdr_symsync_reset(hzsdr_symsync *f) { return hz::lb::reset<hz::SymBank>(f); }

int hzsdr_symsync_free(hzsdr_symsync *f) { return f ? hz::lb::destroy(f, {f->loop_rows, f->maxw}) : HZSDR_ERR_INVALID_ARGUMENT; }

}  // extern "C"
