// hz_equalizer.hip -- the adaptive equalizer bank (include/hzsdr_equalizer.h): an N-tap linear equalizer at the symbol
// rate over R rows of soft symbols, real or complex, adapted blind (CMA) or on its own decisions (DD_BPSK, DD_QPSK), one
// output per symbol consumed.  The arithmetic of every output, track value and state word is hz_equalizer_math.h
// (shared with the host restatement of tests/host/equalizer_ref.cpp); the host arithmetic (lanes per row, rows per
// wave, the LDS and its address maps, the state's layout, the bounds) is hz_equalizer_plan.h.
//
// One kernel, and a shape of its own in the family: LANE = TAP.  A workgroup is one wave and owns G consecutive rows
// for the whole push, as the row-wave banks' does (hz_rowwave.h: the wave's sync, the wait before the loop), but a row
// takes Np consecutive lanes and lane i of them keeps tap w[i] in registers from the first tile to the last.  Time goes
// by in tiles of T = 256 symbols:
//   1. the tile's symbols, fetched a tile ahead into registers with lane = symbol, go into the row's segment of the
//      LDS behind the N - 1 symbols of history that the tile before left there (the state's, before the first);
//   2. the loads of the next tile are issued and stay in flight under
//   3. the walk, t = 0 ... the largest count of the wave's rows: lane i reads X[i] at slot N - 1 + t - i (eight symbols
//      ahead of the steps that consume them), multiplies, the Np products are summed by a butterfly of lane exchanges
//      (eq_exchange: the form is HZ_EQ_EXCHANGE, below), every lane forms the error and the step from the sum and
//      updates its own tap; the row's first lane writes y, and the track value where asked for, into the output tile.
//      A row past its count goes through the same instructions with its taps held and nothing written: the lanes of
//      the wave stay together, and the exchanges always run with every lane live;
//   4. the last N - 1 symbols a row consumed move to the front of its segment, and the output tile is stored with
//      lane = symbol, every store guarded by the row's count.
// Behind the last tile the taps and the history go back to the state.  A row's count comes from in_counts and never
// from a float: no NaN reaches a trip count, an address or another row's lanes (the exchanges stay inside Np lanes).
//
// HZ_EQ_EXCHANGE, the form of p[i ^ s] (the builds that tools/equalizer_time.py compares):
//   0  __shfl_xor: a ds_bpermute per component and stage;
//   1  lane moves in the VALU where the chip has one: quad permutes for s = 1 and 2, the half-row and row mirrors for
//      s = 4 and 8 (lane 7 - i and lane 15 - i hold the bits of lane i ^ 4 and i ^ 8, since the stages before left
//      their groups of 4 and 8 lanes equal), the 16- and 32-lane swaps of gfx950 for s = 16 and 32;
//   2  a round trip through 64 floats of the wave's LDS per component.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_equalizer.h"
#include "hz_equalizer_math.h"
#include "hz_equalizer_plan.h"
#include "hz_loopbank.h"
#include "hz_rowwave.h"

#ifndef HZ_EQ_EXCHANGE
#define HZ_EQ_EXCHANGE 1
#endif

struct hzsdr_equalizer : hz::lb::LoopBank<hz::em::Loop, float> {  // params: 2 to the set; the state: ep::state_floats
    static constexpr const char *noun = "equalizer";
    int kind = 0, mode = 0;
    hz::ep::Geom g{};
};

namespace hz {

static bool eq_complex(int kind) { return kind == HZSDR_FMT_C64; }
static size_t eq_size(int kind) { return eq_complex(kind) ? sizeof(float2) : sizeof(float); }

struct EqArgs {
    const void *in;  // row r starts r * in_stride symbols in
    size_t in_stride;
    void *out;
    size_t out_stride;
    float *track;  // (TRACK forms only)
    size_t track_stride;
    const uint32_t *in_counts;  // null: every row has n
    const em::Loop *loop_rows;
    float *state;
    uint32_t n;  // symbols per row in the push at most
    uint32_t R, G, N, S, out_base, xchg_base;
    int mode;
    em::Loop loop;  // the shared parameters
};

template <int PL> struct EqSrc {
    using T = float2;
    static __device__ __forceinline__ void split(float2 v, float (&x)[PL]) { x[0] = v.x, x[PL - 1] = v.y; }
    static __device__ __forceinline__ float2 pack(float re, float im) { return make_float2(re, im); }
};
template <> struct EqSrc<1> {
    using T = float;
    static __device__ __forceinline__ void split(float v, float (&x)[1]) { x[0] = v; }
    static __device__ __forceinline__ float pack(float re, float) { return re; }
};

// one stage of the sum: v + the value of lane l ^ S (its bits, where the stages before left the lanes of a group equal:
// see above)
template <int S> __device__ __forceinline__ float eq_stage(float v, float *xchg, uint32_t lane) {
#if HZ_EQ_EXCHANGE == 1
    const int b = __float_as_int(v);
    if constexpr (S == 1) return v + __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0xB1, 0xF, 0xF, false));  // quad_perm [1, 0, 3, 2]
    if constexpr (S == 2) return v + __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x4E, 0xF, 0xF, false));  // quad_perm [2, 3, 0, 1]
    if constexpr (S == 4) return v + __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x141, 0xF, 0xF, false));  // row_half_mirror
    if constexpr (S == 8) return v + __int_as_float(__builtin_amdgcn_update_dpp(0, b, 0x140, 0xF, 0xF, false));  // row_mirror
#if __has_builtin(__builtin_amdgcn_permlane16_swap) && __has_builtin(__builtin_amdgcn_permlane32_swap)
    // both operands hold v: behind the swap one of them has the even halves (of 16, of 32 lanes) twice and the other
    // the odd ones, so in every lane one is the lane's own value and the other its partner's, and addition commutes
    if constexpr (S == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)b, (unsigned)b, false, false);
        return __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
    }
    if constexpr (S == 32) {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)b, (unsigned)b, false, false);
        return __int_as_float((int)r[0]) + __int_as_float((int)r[1]);
    }
#endif
    return v + __shfl_xor(v, S, 64);
#elif HZ_EQ_EXCHANGE == 2
    xchg[lane] = v;
    rw::wave_sync();
    const float o = xchg[lane ^ S];
    rw::wave_sync();
    return v + o;
#else
    return v + __shfl_xor(v, S, 64);
#endif
}

// p[i] += p[i ^ s] for s = 1, 2, 4 ... < NP, over the row's NP lanes at once
template <int PL, int NP> __device__ __forceinline__ void eq_butterfly(float (&p)[PL], float *xchg, uint32_t lane) {
#pragma unroll
    for (int q = 0; q < PL; q++) {
        float v = p[q];
        float *x = xchg + q * ep::kLanes;
        if constexpr (NP > 1) v = eq_stage<1>(v, x, lane);
        if constexpr (NP > 2) v = eq_stage<2>(v, x, lane);
        if constexpr (NP > 4) v = eq_stage<4>(v, x, lane);
        if constexpr (NP > 8) v = eq_stage<8>(v, x, lane);
        if constexpr (NP > 16) v = eq_stage<16>(v, x, lane);
        if constexpr (NP > 32) v = eq_stage<32>(v, x, lane);
        p[q] = v;
    }
}

// what a lane carries through the walk
template <int PL> struct EqLane {
    float w[PL];    // the tap
    em::Loop k;     // the row's parameters
    float *lds;     // the wave's LDS
    uint32_t x0;    // the lane's X[tap] of symbol 0 of a tile, plane 0
    uint32_t xp;    // floats from plane to plane of the segments
    uint32_t y0;    // the row's output of symbol 0, plane 0
    uint32_t yp;    // floats from plane to plane of the outputs (the track is plane PL)
    uint32_t lane;
    float *xchg;
    bool fill;      // a lane from tap N up: its product is +0
    bool first;     // tap 0: it writes the row's outputs
};

// one symbol: x is X[tap]; t the symbol's place in the tile, tn the symbols of the tile that the lane's row consumes
template <int PL, int NP, int MODE, bool TRACK>
__device__ __forceinline__ void eq_symbol(EqLane<PL> &s, const float (&x)[PL], uint32_t t, uint32_t tn) {
    float p[PL], e[PL], g[PL], wn[PL];
    em::eq_product<PL>(s.w, x, p);
#pragma unroll
    for (int q = 0; q < PL; q++) p[q] = s.fill ? 0.0f : p[q];
    eq_butterfly<PL, NP>(p, s.xchg, s.lane);
    em::eq_error<PL>(MODE, p, s.k.level, e);
    em::eq_gain<PL>(s.k.mu, e, g);
#pragma unroll
    for (int q = 0; q < PL; q++) wn[q] = s.w[q];
    em::eq_update<PL>(wn, g, x);
    const bool act = t < tn;
#pragma unroll
    for (int q = 0; q < PL; q++) s.w[q] = act ? wn[q] : s.w[q];
    if (act && s.first) {
#pragma unroll
        for (int q = 0; q < PL; q++) s.lds[s.y0 + q * s.yp + t] = p[q];
        if (TRACK) s.lds[s.y0 + PL * s.yp + t] = em::eq_track<PL>(e);
    }
}

// symbols [0, tmax) of the tile (tmax: the largest count of the wave's rows; wave-uniform).  Eight symbols are read
// before the steps that consume them, so that no LDS latency sits on the loop-carried path.
template <int PL, int NP, int MODE, bool TRACK>
__device__ __forceinline__ void eq_walk(EqLane<PL> &s, uint32_t tmax, uint32_t tn) {
    uint32_t t = 0;
#pragma unroll 1
    for (; t + 8 <= tmax; t += 8) {
        float x[8][PL];
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int q = 0; q < PL; q++) x[j][q] = s.lds[s.x0 + q * s.xp + t + j];
#pragma unroll
        for (int j = 0; j < 8; j++) eq_symbol<PL, NP, MODE, TRACK>(s, x[j], t + j, tn);
    }
#pragma unroll 1
    for (; t < tmax; t++) {
        float x[PL];
#pragma unroll
        for (int q = 0; q < PL; q++) x[q] = s.lds[s.x0 + q * s.xp + t];
        eq_symbol<PL, NP, MODE, TRACK>(s, x, t, tn);
    }
}

template <int PL, int NP, bool PER_ROW, bool TRACK>
__global__ __launch_bounds__(ep::kLanes) void equalizer_rows_kernel(EqArgs a) {
    using Src = EqSrc<PL>;
    using ST = typename Src::T;
    constexpr uint32_t T = ep::kTile;
    constexpr int K = ep::kSteps;
    extern __shared__ __align__(16) unsigned char equalizer_lds[];
    float *lds = (float *)equalizer_lds;
    const uint32_t lane = threadIdx.x, row0 = rw::wave_first_row(blockIdx.x, a.G), g = rw::wave_row_count(blockIdx.x, a.G, a.R);
    const uint32_t N = a.N, tap = ep::lane_tap(lane, NP);
    const bool own = ep::lane_row(lane, NP) < g;       // the lane's row is one of the bank's
    const uint32_t mr = own ? ep::lane_row(lane, NP) : 0;  // the row whose addresses the lane uses
    const bool live = own && tap < N, past = own && tap + 1 < N;  // a tap of the row; an entry of its history
    const size_t row = (size_t)row0 + mr;

    // the rows' counts: wave-uniform, from integers alone
    uint32_t cnt[ep::kMaxGroup], cmax = 0, mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < ep::kMaxGroup; r++) {
        cnt[r] = 0;
        if (r < g) {
            const uint32_t c = a.in_counts ? a.in_counts[row0 + r] : a.n;
            cnt[r] = c < a.n ? c : a.n;
            cmax = cnt[r] > cmax ? cnt[r] : cmax;
            if (own && mr == r) mine = cnt[r];
        }
    }

    EqLane<PL> s{};
    s.k = a.loop;
    s.lds = lds, s.lane = lane, s.xchg = lds + a.xchg_base;
    s.x0 = ep::seg_slot(mr, 0, ep::walk_slot(tap, 0, N), a.G, a.S), s.xp = a.G * a.S;
    s.y0 = ep::out_slot(mr, 0, 0, a.G, a.out_base), s.yp = a.G * ep::kOutPitch;
    s.fill = tap >= N, s.first = tap == 0;
    float *z = a.state + row * ep::state_row_floats(N, PL);
    if (own && PER_ROW) s.k = a.loop_rows[row];
    if (live) {
#pragma unroll
        for (int q = 0; q < PL; q++) s.w[q] = z[ep::state_tap(tap, q, PL)];
    }
    if (past) {
#pragma unroll
        for (int q = 0; q < PL; q++) lds[ep::seg_slot(mr, q, ep::history_slot(tap, N), a.G, a.S)] = z[ep::state_history(tap, q, N, PL)];
    }

    const ST *in = (const ST *)a.in + (size_t)row0 * a.in_stride;
    ST *out = (ST *)a.out + (size_t)row0 * a.out_stride;
    float *track = TRACK ? a.track + (size_t)row0 * a.track_stride : nullptr;
    ST raw[ep::kMaxGroup][K];
    // the tile's symbols of the wave's rows into registers: lane = symbol, every row up to its own count
    auto fetch = [&](uint32_t t0) {
#pragma unroll
        for (uint32_t r = 0; r < ep::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    const uint32_t t = lane + ep::kLanes * kk;
                    if (t < cnt[r] - (t0 < cnt[r] ? t0 : cnt[r])) raw[r][kk] = in[r * a.in_stride + t0 + t];
                }
            }
        }
    };
    fetch(0);
    rw::settle(s.k.mu), rw::settle(s.k.level);
#pragma unroll
    for (int q = 0; q < PL; q++) rw::settle(s.w[q]);

#pragma unroll 1
    for (uint32_t t0 = 0; t0 < cmax; t0 += T) {
        const uint32_t left = cmax - t0, tmax = left < T ? left : T;
        // 1. into the segments: row fixed, lane = symbol
#pragma unroll
        for (uint32_t r = 0; r < ep::kMaxGroup; r++) {
            if (r < g) {
                const uint32_t tr = cnt[r] > t0 ? cnt[r] - t0 : 0;
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    if (lane + ep::kLanes * kk < tr) {
                        float x[PL];
                        Src::split(raw[r][kk], x);
#pragma unroll
                        for (int q = 0; q < PL; q++) lds[ep::seg_slot(r, q, ep::load_slot(lane, kk, N), a.G, a.S)] = x[q];
                    }
                }
            }
        }
        rw::wave_sync();
        // 2. the next tile's loads, in flight under the walk
        if (left > T) fetch(t0 + T);
        // 3. lane = tap
        const uint32_t ahead = mine > t0 ? mine - t0 : 0, tn = ahead < T ? ahead : T;
        switch (a.mode) {
        case em::kCma: eq_walk<PL, NP, em::kCma, TRACK>(s, tmax, tn); break;
        case em::kDdBpsk: eq_walk<PL, NP, em::kDdBpsk, TRACK>(s, tmax, tn); break;
        default: eq_walk<PL, NP, em::kDdQpsk, TRACK>(s, tmax, tn); break;
        }
        rw::wave_sync();
        // 4. the history to the front of the segment (read by all lanes before any writes), and the outputs out of
        // their tile: row fixed, lane = symbol
        float h[PL];
        if (past) {
#pragma unroll
            for (int q = 0; q < PL; q++) h[q] = lds[ep::seg_slot(mr, q, tap + tn, a.G, a.S)];
        }
        rw::wave_sync();
        if (past) {
#pragma unroll
            for (int q = 0; q < PL; q++) lds[ep::seg_slot(mr, q, tap, a.G, a.S)] = h[q];
        }
#pragma unroll
        for (uint32_t r = 0; r < ep::kMaxGroup; r++) {
            if (r < g) {
                const uint32_t tr = cnt[r] > t0 ? cnt[r] - t0 : 0;
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    const uint32_t t = lane + ep::kLanes * kk;
                    if (t < tr) {  // (t < T: tr is at most the tile where it matters, and t is below T)
                        const float re = lds[ep::out_slot(r, 0, t, a.G, a.out_base)];
                        const float im = PL == 2 ? lds[ep::out_slot(r, PL - 1, t, a.G, a.out_base)] : 0.0f;
                        out[r * a.out_stride + t0 + t] = Src::pack(re, im);
                        if (TRACK) track[r * a.track_stride + t0 + t] = lds[ep::out_slot(r, PL, t, a.G, a.out_base)];
                    }
                }
            }
        }
        rw::wave_sync();  // (the next tile's symbols and outputs overwrite these)
    }

    if (live) {
#pragma unroll
        for (int q = 0; q < PL; q++) z[ep::state_tap(tap, q, PL)] = s.w[q];
    }
    if (past) {
#pragma unroll
        for (int q = 0; q < PL; q++) z[ep::state_history(tap, q, N, PL)] = lds[ep::seg_slot(mr, q, ep::history_slot(tap, N), a.G, a.S)];
    }
}

template <int PL, int NP, bool PER_ROW>
static int eq_launch_track(hzsdr_equalizer *f, const EqArgs &a) {
    const dim3 grid(f->g.waves), block(ep::kLanes);
    if (a.track)
        HZ_TRY(launch_fv(equalizer_rows_kernel<PL, NP, PER_ROW, true>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else
        HZ_TRY(launch_fv(equalizer_rows_kernel<PL, NP, PER_ROW, false>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    HZ_HIP(f->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int PL, int NP>
static int eq_launch_sets(hzsdr_equalizer *f, const EqArgs &a) {
    return f->per_row ? eq_launch_track<PL, NP, true>(f, a) : eq_launch_track<PL, NP, false>(f, a);
}

template <int PL>
static int eq_launch_lanes(hzsdr_equalizer *f, const EqArgs &a) {
    switch (f->g.Np) {
    case 1: return eq_launch_sets<PL, 1>(f, a);
    case 2: return eq_launch_sets<PL, 2>(f, a);
    case 4: return eq_launch_sets<PL, 4>(f, a);
    case 8: return eq_launch_sets<PL, 8>(f, a);
    case 16: return eq_launch_sets<PL, 16>(f, a);
    case 32: return eq_launch_sets<PL, 32>(f, a);
    default: return eq_launch_sets<PL, 64>(f, a);
    }
}

// what the bank gives hz_loopbank.h (stage_params, commit_params, initial_state, set_params, reset); create is its own
struct EqBank {
    using Obj = hzsdr_equalizer;
    static constexpr size_t kParams = ep::kParams;
    static const char *check_params(const float *p) { return ep::check_params(p); }
    static em::Loop derive(const float *p) { return ep::derive(p); }
    // the initial state: w[c] = 1, everything else +0
    static void initial(const hzsdr_equalizer *f, size_t r, size_t, float *z) {
        z[r * ep::state_row_floats(f->g.N, f->g.planes) + ep::state_tap(f->g.c, 0, f->g.planes)] = 1.0f;
    }
};

}  // namespace hz

extern "C" {

int hzsdr_equalizer_create(hzsdr_ctx *ctx, int kind, int mode, size_t taps, size_t centre, const float *params, int per_row, size_t rows,
                           hzsdr_equalizer **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != HZSDR_EQUALIZER_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "equalizer: real float32 or complex64 rows");
    if (rows == 0 || rows > rw::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "equalizer: 1 ... 8192 rows");
    const bool big = taps > ep::kMaxTaps || centre > ep::kMaxTaps;
    if (const char *why = ep::check_geom(big ? -1 : (long long)taps, big ? -1 : (long long)centre, mode, eq_complex(kind)))
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("equalizer: ") + why);
    hzsdr_equalizer *f = new hzsdr_equalizer{};
    f->ctx = ctx, f->R = (uint32_t)rows, f->per_row = per_row != 0;
    lb::ParamSets<em::Loop> next;
    int rc = lb::stage_params<EqBank>(f, params, next);
    if (rc == HZSDR_OK) rc = enter(ctx);
    if (rc != HZSDR_OK) {
        delete f;
        return rc;
    }
    auto undo = [&](int status) {
        lb::destroy(f, {f->loop_rows});
        return status;
    };
    f->kind = kind, f->mode = mode;
    f->g = ep::equalizer_geom(f->R, (uint32_t)taps, (uint32_t)centre, eq_complex(kind));
    f->words = ep::state_floats(f->R, f->g.N, f->g.planes);
    hipError_t e = hipMalloc((void **)&f->state, f->words * sizeof(uint32_t));
    if (e == hipSuccess && f->per_row) e = hipMalloc((void **)&f->loop_rows, (size_t)f->R * sizeof(em::Loop));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "equalizer_create", __FILE__, __LINE__));
    rc = lb::commit_params(f, next);
    if (rc == HZSDR_OK) rc = lb::initial_state<EqBank>(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_equalizer_push(hzsdr_equalizer *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, void *out, size_t out_stride,
                         float *track, size_t track_stride) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R, size = eq_size(f->kind);
    if (n && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "equalizer: null input");
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "equalizer: in_stride is below the symbols of the push");
    if (n > 0xfffffff0ull) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "equalizer: the push is too long");
    HZ_TRY(check_rows_out(ctx, "equalizer", R, out, n, out_stride, n, 0));
    if (track) HZ_TRY(check_rows_out(ctx, "equalizer track", R, track, n, track_stride, n, 0));
    if (n && in == out && R > 1 && in_stride != out_stride) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "equalizer: in place needs equal strides");
    HZ_TRY(enter(ctx));
    if (n == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din, *dic = nullptr;
    void *dout, *dtrack = nullptr;
    size_t dstride, ostride = out_stride, tstride = track_stride;
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, size, &din, &dstride));
    if (in_counts) HZ_TRY(st.in(3, in_counts, R * sizeof(uint32_t), &dic));
    // with counts the columns behind a row's count stay as they are: a HOST context's rows go up before they come back
    auto rows_out = [&](int slot, void *p, size_t stride, size_t bytes, void **dev, size_t *dev_stride) {
        if (!in_counts) return st.out_rows(slot, p, R, n, stride, bytes, dev, dev_stride);
        if (R == 1 || stride == n) return st.out_preserve(slot, p, R * n * bytes, dev);
        const void *up;
        HZ_TRY(st.in_rows(slot, p, R, n, stride, bytes, &up, dev_stride));
        return st.out_rows(slot, p, R, n, stride, bytes, dev, dev_stride);
    };
    HZ_TRY(rows_out(1, out, out_stride, size, &dout, &ostride));
    if (track) HZ_TRY(rows_out(2, track, track_stride, sizeof(float), &dtrack, &tstride));
    EqArgs a{din, dstride, dout, ostride, (float *)dtrack, tstride, (const uint32_t *)dic, f->loop_rows, f->state, (uint32_t)n,
             f->R, f->g.G, f->g.N, f->g.S, f->g.out_base, f->g.xchg_base, f->mode, f->loop[0]};
    HZ_TRY(f->g.planes == 2 ? eq_launch_lanes<2>(f, a) : eq_launch_lanes<1>(f, a));
    return st.finish();
}

int hzsdr_equalizer_set_params(hzsdr_equalizer *f, const float *params) { return hz::lb::set_params<hz::EqBank>(f, params); }

int hzsdr_equalizer_get_state(hzsdr_equalizer *f, float *state, size_t cap) { return hz::lb::get_state(f, state, cap); }

int hzsdr_equalizer_set_state(hzsdr_equalizer *f, const float *state, size_t count) {
    return hz::lb::set_state(f, state, count, 0, "the state has rows * (2 * taps - 1) floats (complex rows: twice that)");
}

int hzsdr_equalizer_plan(const hzsdr_equalizer *f, size_t *rows_per_wave, size_t *tile_symbols, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    return hz::lb::plan(f, rows_per_wave, tile_symbols, form,
                        (f->per_row ? HZSDR_EQUALIZER_FORM_PER_ROW : 0) | (hz::eq_complex(f->kind) ? HZSDR_EQUALIZER_FORM_COMPLEX : 0));
}

int hzsdr_equalizer_reset(hzsdr_equalizer *f) { return hz::lb::reset<hz::EqBank>(f); }

int hzsdr_equalizer_free(hzsdr_equalizer *f) { return f ? hz::lb::destroy(f, {f->loop_rows}) : HZSDR_ERR_INVALID_ARGUMENT; }

}  // extern "C"
