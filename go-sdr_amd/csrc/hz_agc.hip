// hz_agc.hip -- the AGC bank (include/hzsdr_agc.h): a multiplicative gain loop over R real float32 or complex64 rows,
// one output per input of the input's type and, where asked for, the gain applied to every sample.  The arithmetic of
// every output, track value and state word is hz_agc_math.h (shared with the host restatement of
// tests/host/agc_ref.cpp); the host arithmetic (rows per wave, the tile's planes, the parameters' bounds and why no
// step overflows) is hz_agc_plan.h.
//
// One kernel, a row-wave one: the wave, its tile and the four steps of a tile are described in hz_rowwave.h, which
// holds the wave's sync, the wait before the loop and the fetch.  Only the gain is carried from sample to sample, so
// only the gain's chain is walked: with lane = sample the loader writes the samples into their planes and, beside
// them, the walk's input b = |x| / ref (a NaN under the gate) into the gain plane -- the square root, the product and
// the gate's comparison at 64 lanes a step; lane l < G then reads b and writes the gain it applied, eight samples read
// ahead of the steps that consume them, one function for both kinds since it never touches x; with lane = sample again
// the storer forms y = x g and sends the gain plane to the track.  No divergent branch in the walk (clip, rate, gate and
// clamps are selections).  Shared parameters travel in the kernel's arguments: wave-uniform scalars; per-row ones are
// loaded by the row's lane, and the two that the loader needs are read out of that lane (a readlane per row).
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_agc.h"
#include "hz_agc_math.h"
#include "hz_agc_plan.h"
#include "hz_loopbank.h"
#include "hz_rowwave.h"

struct hzsdr_agc : hz::lb::LoopBank<hz::am::Loop, float> {  // params: 7 to the set; the state: R gains
    static constexpr const char *noun = "agc";
    int kind = 0;
    hz::ap::Geom g{};
};

namespace hz {

static bool agc_complex(int kind) { return kind == HZSDR_FMT_C64; }
static size_t agc_size(int kind) { return agc_complex(kind) ? sizeof(float2) : sizeof(float); }

struct AgcArgs {
    const void *in;  // row r starts r * in_stride samples in
    size_t in_stride;
    void *out;
    size_t out_stride;
    float *track;  // (TRACK forms only)
    size_t track_stride;
    uint64_t n;  // samples per row in the push
    const am::Loop *loop_rows;
    float *state;
    uint32_t R, G, P;
    am::Loop loop;  // the shared constants
};

__device__ __forceinline__ float agc_sample(float v) { return v; }
__device__ __forceinline__ dm::c32 agc_sample(float2 v) { return dm::c32{v.x, v.y}; }

// lane = row: samples [0, tn) of the gain plane through the loop, the gain applied to a sample over its b.  Eight
// values are read before the steps that consume them, so that no LDS latency sits on the loop-carried path.
__device__ __forceinline__ void agc_walk(float *tl, uint32_t P, uint32_t T, uint32_t tn, const am::Loop &k, float &g) {
    uint32_t t = 0;
#pragma unroll 1
    for (; t + 8 <= tn; t += 8) {
        float b[8];
#pragma unroll
        for (int j = 0; j < 8; j++) b[j] = tl[ap::walk_slot(0, t + j, ap::kGainPlane, P, T)];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float applied = g;
            g = am::agc_step(applied, b[j], k);
            b[j] = applied;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) tl[ap::walk_slot(0, t + j, ap::kGainPlane, P, T)] = b[j];
    }
#pragma unroll 1
    for (; t < tn; t++) {
        const float b = tl[ap::walk_slot(0, t, ap::kGainPlane, P, T)];
        tl[ap::walk_slot(0, t, ap::kGainPlane, P, T)] = g;
        g = am::agc_step(g, b, k);
    }
}

// RT: float (real rows) or float2 (complex rows)
template <typename RT, int K, bool PER_ROW, bool TRACK>
__global__ __launch_bounds__(ap::kLanes) void agc_rows_kernel(AgcArgs a) {
    constexpr uint32_t T = ap::kLanes * K;
    constexpr bool CPLX = sizeof(RT) == sizeof(float2);
    extern __shared__ __align__(16) unsigned char agc_lds[];
    float *tile = (float *)agc_lds;
    const auto [lane, row0, g, own, row] = rw::wave(a);

    am::Loop k = a.loop;
    float gain = 0.0f;
    if (own) {
        if (PER_ROW) k = a.loop_rows[row];
        gain = a.state[row];
    }

    const RT *in = (const RT *)a.in + (size_t)row0 * a.in_stride;
    RT *out = (RT *)a.out + (size_t)row0 * a.out_stride;
    float *track = TRACK ? a.track + (size_t)row0 * a.track_stride : nullptr;
    RT raw[ap::kMaxGroup][K];
    rw::fetch<RT, K>(raw, in, a.in_stride, g, 0, a.n, lane);
    rw::settle(k.iref), rw::settle(k.attack), rw::settle(k.decay), rw::settle(k.floor), rw::settle(k.gmin), rw::settle(k.gmax);
    rw::settle(gain);
    // what the loader needs of row r's constants: wave-uniform, out of the row's lane where the rows have their own
    float iref[ap::kMaxGroup], floor[ap::kMaxGroup];
#pragma unroll
    for (uint32_t r = 0; r < ap::kMaxGroup; r++) {
        iref[r] = PER_ROW ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k.iref), r)) : a.loop.iref;
        floor[r] = PER_ROW ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(k.floor), r)) : a.loop.floor;
    }

#pragma unroll 1
    for (uint64_t t0 = 0; t0 < a.n; t0 += T) {
        const uint64_t left = a.n - t0;
        const uint32_t tn = left < T ? (uint32_t)left : T;
        // 1. into the tile: row fixed, lane = sample; the sample's plane(s) and its b
#pragma unroll
        for (uint32_t r = 0; r < ap::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    if (lane + ap::kLanes * kk < tn) {
                        const RT x = raw[r][kk];
                        if constexpr (CPLX) {
                            tile[ap::move_slot(lane, kk, r, ap::kSamplePlane, a.P, T)] = x.x;
                            tile[ap::move_slot(lane, kk, r, ap::kSamplePlane + 1, a.P, T)] = x.y;
                        } else {
                            tile[ap::move_slot(lane, kk, r, ap::kSamplePlane, a.P, T)] = x;
                        }
                        tile[ap::move_slot(lane, kk, r, ap::kGainPlane, a.P, T)] = am::agc_drive(am::agc_level(agc_sample(x)), iref[r], floor[r]);
                    }
                }
            }
        }
        rw::wave_sync();
        // 2. the next tile's loads, in flight under the walk
        if (left > T) rw::fetch<RT, K>(raw, in, a.in_stride, g, t0 + T, a.n, lane);
        // 3. lane = row
        if (own) agc_walk(tile + lane, a.P, T, tn, k, gain);
        rw::wave_sync();
        // 4. out of the tile: row fixed, lane = sample; y = x g
#pragma unroll
        for (uint32_t r = 0; r < ap::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    const uint32_t t = lane + ap::kLanes * kk;
                    if (t < tn) {
                        const float applied = tile[ap::move_slot(lane, kk, r, ap::kGainPlane, a.P, T)];
                        if constexpr (CPLX) {
                            const dm::c32 x{tile[ap::move_slot(lane, kk, r, ap::kSamplePlane, a.P, T)],
                                            tile[ap::move_slot(lane, kk, r, ap::kSamplePlane + 1, a.P, T)]};
                            const dm::c32 y = am::agc_apply(x, applied);
                            out[r * a.out_stride + t0 + t] = make_float2(y.re, y.im);
                        } else {
                            out[r * a.out_stride + t0 + t] = am::agc_apply(tile[ap::move_slot(lane, kk, r, ap::kSamplePlane, a.P, T)], applied);
                        }
                        if (TRACK) track[r * a.track_stride + t0 + t] = applied;
                    }
                }
            }
        }
        rw::wave_sync();  // (the next tile's samples overwrite these)
    }

    if (own) a.state[row] = gain;
}

template <typename RT, bool PER_ROW>
static int agc_launch_track(hzsdr_agc *f, const AgcArgs &a) {
    constexpr int K = ap::kSteps;  // (the plan's: f->g.K)
    const dim3 grid(f->g.waves), block(ap::kLanes);
    if (a.track)
        HZ_TRY(launch_fv(agc_rows_kernel<RT, K, PER_ROW, true>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else
        HZ_TRY(launch_fv(agc_rows_kernel<RT, K, PER_ROW, false>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    HZ_HIP(f->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <typename RT>
static int agc_launch_kind(hzsdr_agc *f, const AgcArgs &a) {
    return f->per_row ? agc_launch_track<RT, true>(f, a) : agc_launch_track<RT, false>(f, a);
}

static int agc_launch(hzsdr_agc *f, const AgcArgs &a) {
    return agc_complex(f->kind) ? agc_launch_kind<float2>(f, a) : agc_launch_kind<float>(f, a);
}

// what the bank gives hz_loopbank.h
struct AgcBank {
    using Obj = hzsdr_agc;
    static constexpr size_t kParams = ap::kParams;
    static const char *check_params(const float *p) { return ap::check_params(p); }
    static am::Loop derive(const float *p) { return ap::derive(p); }
    static int check_kind(hzsdr_ctx *ctx, int kind) {
        if (kind != HZSDR_AGC_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "agc: real float32 or complex64 rows");
        return HZSDR_OK;
    }
    static void shape(hzsdr_agc *f, int kind) {
        f->kind = kind;
        f->g = ap::agc_geom(f->R, agc_complex(kind));
        f->words = f->R;
    }
    // the initial state: g = g0 of the row
    static void initial(const hzsdr_agc *f, size_t r, size_t set, float *z) { z[r] = ap::initial_gain(f->params.data() + set * kParams); }
};

}  // namespace hz

extern "C" {

int hzsdr_agc_create(hzsdr_ctx *ctx, int kind, const float *params, int per_row, size_t rows, hzsdr_agc **out) {
    return hz::lb::create<hz::AgcBank>(ctx, kind, params, per_row, rows, out);
}

int hzsdr_agc_push(hzsdr_agc *f, const void *in, size_t n, size_t in_stride, void *out, size_t out_stride, float *track, size_t track_stride) {
    using namespace hz;
    const size_t size = f ? agc_size(f->kind) : 0;
    return lb::push_rows(f, n, {in, in_stride, size}, {out, n, out_stride, size}, {track, n, track_stride, sizeof(float)}, [&](const lb::DevRows &d) {
        AgcArgs a{d.in, d.in_stride, d.out, d.out_stride, d.track, d.track_stride, n, f->loop_rows, f->state, f->R, f->g.G, f->g.P, f->loop[0]};
        return agc_launch(f, a);
    });
}

int hzsdr_agc_set_params(hzsdr_agc *f, const float *params) { return hz::lb::set_params<hz::AgcBank>(f, params); }

int hzsdr_agc_get_state(hzsdr_agc *f, float *state, size_t cap) { return hz::lb::get_state(f, state, cap); }

int hzsdr_agc_set_state(hzsdr_agc *f, const float *state, size_t count, uint64_t position) {
    return hz::lb::set_state(f, state, count, position, "the state has one float per row");
}

int hzsdr_agc_position(const hzsdr_agc *f, uint64_t *position) { return hz::lb::position(f, position); }

int hzsdr_agc_plan(const hzsdr_agc *f, size_t *rows_per_wave, size_t *tile_samples, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    return hz::lb::plan(f, rows_per_wave, tile_samples, form,
                        (f->per_row ? HZSDR_AGC_FORM_PER_ROW : 0) | (hz::agc_complex(f->kind) ? HZSDR_AGC_FORM_COMPLEX : 0));
}

int hzsdr_agc_reset(hzsdr_agc *f) { return hz::lb::reset<hz::AgcBank>(f); }

int hzsdr_agc_free(hzsdr_agc *f) { return f ? hz::lb::destroy(f, {f->loop_rows}) : HZSDR_ERR_INVALID_ARGUMENT; }

}  // extern "C"
