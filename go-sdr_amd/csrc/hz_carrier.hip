// hz_carrier.hip -- the carrier recovery bank (include/hzsdr_carrier.h): a second-order loop around a numerically
// controlled oscillator over R complex64 rows, three phase detectors, one derotated output per input and, where asked
// for, the frequency estimate behind every sample.  The arithmetic of every output, track value and state word is
// hz_carrier_math.h (shared with the host restatement of tests/host/carrier_ref.cpp); the host arithmetic (rows per
// wave, the tile and its third plane, the loop constants and their bounds) is hz_carrier_plan.h.
//
// One kernel, a row-wave one: the wave, its tile and the four steps of a tile are described in hz_rowwave.h, which
// holds the wave's sync, the wait before the loop and the fetch.  Lane l < G keeps theta, F and its row's constants in
// registers from the first tile to the last, reads the two state words from the object's state array before and
// writes them back behind.  The walk is the loop: eight samples read ahead of the steps that consume them, each y
// written over its x, the track into a third plane of the tile; no divergent branch (the detector is a template
// parameter, clip and clamp are selections).  The tile is read back as it was written, and the track plane likewise.
// Shared parameters travel in the kernel's arguments: wave-uniform scalars, never lane by lane.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_carrier.h"
#include "hz_carrier_math.h"
#include "hz_carrier_plan.h"
#include "hz_loopbank.h"
#include "hz_rowwave.h"

struct hzsdr_carrier : hz::lb::LoopBank<hz::cm::Loop, uint32_t> {  // params: 5 to the set; the state: cp::state_words, cp::state_index
    static constexpr const char *noun = "carrier";
    int mode = 0;
    hz::cp::Geom g{};
};

namespace hz {

struct CarArgs {
    const float2 *in;  // row r starts r * in_stride samples in
    size_t in_stride;
    float2 *out;
    size_t out_stride;
    float *track;  // (TRACK forms only)
    size_t track_stride;
    uint64_t n;  // samples per row in the push
    const cm::Loop *loop_rows;
    uint32_t *state;
    uint32_t R, G, P;
    cm::Loop loop;  // the shared constants
};

// lane = row: samples [0, tn) of the tile through the loop, y over x, the track into its plane.  Eight samples are read
// before the steps that consume them, so that no LDS latency sits on the loop-carried path.
template <int MODE, bool TRACK>
__device__ __forceinline__ void car_walk(float *tl, uint32_t P, uint32_t T, uint32_t tn, const cm::Loop &k, cm::State &s) {
    uint32_t t = 0;
#pragma unroll 1
    for (; t + 8 <= tn; t += 8) {
        tn::c32 x[8];
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = tn::c32{tl[cp::walk_slot(0, t + j, 0, P, T)], tl[cp::walk_slot(0, t + j, 1, P, T)]};
#pragma unroll
        for (int j = 0; j < 8; j++) f[j] = cm::car_step<MODE>(s, k, x[j], &x[j]);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            tl[cp::walk_slot(0, t + j, 0, P, T)] = x[j].re;
            tl[cp::walk_slot(0, t + j, 1, P, T)] = x[j].im;
            if (TRACK) tl[cp::walk_slot(0, t + j, cp::kTrackPlane, P, T)] = f[j];
        }
    }
#pragma unroll 1
    for (; t < tn; t++) {
        tn::c32 x{tl[cp::walk_slot(0, t, 0, P, T)], tl[cp::walk_slot(0, t, 1, P, T)]};
        const float f = cm::car_step<MODE>(s, k, x, &x);
        tl[cp::walk_slot(0, t, 0, P, T)] = x.re;
        tl[cp::walk_slot(0, t, 1, P, T)] = x.im;
        if (TRACK) tl[cp::walk_slot(0, t, cp::kTrackPlane, P, T)] = f;
    }
}

template <int MODE, int K, bool PER_ROW, bool TRACK>
__global__ __launch_bounds__(cp::kLanes) void carrier_rows_kernel(CarArgs a) {
    constexpr uint32_t T = cp::kLanes * K;
    extern __shared__ __align__(16) unsigned char carrier_lds[];
    float *tile = (float *)carrier_lds;
    const auto [lane, row0, g, own, row] = rw::wave(a);

    cm::Loop k = a.loop;
    cm::State s{0u, 0};
    if (own) {
        if (PER_ROW) k = a.loop_rows[row];
        s.theta = a.state[cp::state_index(row, 0)];
        s.f = (int32_t)a.state[cp::state_index(row, 1)];
    }

    const float2 *in = a.in + (size_t)row0 * a.in_stride;
    float2 *out = a.out + (size_t)row0 * a.out_stride;
    float *track = TRACK ? a.track + (size_t)row0 * a.track_stride : nullptr;
    float2 raw[cp::kMaxGroup][K];
    rw::fetch<float2, K>(raw, in, a.in_stride, g, 0, a.n, lane);
    rw::settle(k.aw), rw::settle(k.bw), rw::settle((uint32_t)k.fmin), rw::settle((uint32_t)k.fmax);
    rw::settle(s.theta), rw::settle((uint32_t)s.f);

#pragma unroll 1
    for (uint64_t t0 = 0; t0 < a.n; t0 += T) {
        const uint64_t left = a.n - t0;
        const uint32_t tn = left < T ? (uint32_t)left : T;
        // 1. into the tile: row fixed, lane = sample
#pragma unroll
        for (uint32_t r = 0; r < cp::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    if (lane + cp::kLanes * kk < tn) {
                        tile[cp::move_slot(lane, kk, r, 0, a.P, T)] = raw[r][kk].x;
                        tile[cp::move_slot(lane, kk, r, 1, a.P, T)] = raw[r][kk].y;
                    }
                }
            }
        }
        rw::wave_sync();
        // 2. the next tile's loads, in flight under the walk
        if (left > T) rw::fetch<float2, K>(raw, in, a.in_stride, g, t0 + T, a.n, lane);
        // 3. lane = row
        if (own) car_walk<MODE, TRACK>(tile + lane, a.P, T, tn, k, s);
        rw::wave_sync();
        // 4. out of the tile: row fixed, lane = sample
#pragma unroll
        for (uint32_t r = 0; r < cp::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int kk = 0; kk < K; kk++) {
                    const uint32_t t = lane + cp::kLanes * kk;
                    if (t < tn) {
                        const float re = tile[cp::move_slot(lane, kk, r, 0, a.P, T)];
                        const float im = tile[cp::move_slot(lane, kk, r, 1, a.P, T)];
                        out[r * a.out_stride + t0 + t] = make_float2(re, im);
                        if (TRACK) track[r * a.track_stride + t0 + t] = tile[cp::move_slot(lane, kk, r, cp::kTrackPlane, a.P, T)];
                    }
                }
            }
        }
        rw::wave_sync();  // (the next tile's samples overwrite these)
    }

    if (own) {
        a.state[cp::state_index(row, 0)] = s.theta;
        a.state[cp::state_index(row, 1)] = (uint32_t)s.f;
    }
}

template <int MODE, bool PER_ROW>
static int car_launch_track(hzsdr_carrier *f, const CarArgs &a, size_t lds) {
    constexpr int K = cp::kSteps;  // (the plan's: f->g.K)
    const dim3 grid(f->g.waves), block(cp::kLanes);
    if (a.track)
        HZ_TRY(launch_fv(carrier_rows_kernel<MODE, K, PER_ROW, true>, grid, block, lds, f->ctx->stream, a));
    else
        HZ_TRY(launch_fv(carrier_rows_kernel<MODE, K, PER_ROW, false>, grid, block, lds, f->ctx->stream, a));
    HZ_HIP(f->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int MODE>
static int car_launch_mode(hzsdr_carrier *f, const CarArgs &a, size_t lds) {
    return f->per_row ? car_launch_track<MODE, true>(f, a, lds) : car_launch_track<MODE, false>(f, a, lds);
}

static int car_launch(hzsdr_carrier *f, const CarArgs &a) {
    const size_t lds = cp::carrier_geom(f->R, a.track != nullptr).lds_bytes;
    switch (f->mode) {
    case HZSDR_CARRIER_TONE: return car_launch_mode<cm::kTone>(f, a, lds);
    case HZSDR_CARRIER_BPSK: return car_launch_mode<cm::kBpsk>(f, a, lds);
    default: return car_launch_mode<cm::kQpsk>(f, a, lds);
    }
}

// what the bank gives hz_loopbank.h
struct CarBank {
    using Obj = hzsdr_carrier;
    static constexpr size_t kParams = cp::kParams;
    static const char *check_params(const float *p) { return cp::check_params(p); }
    static cm::Loop derive(const float *p) { return cp::derive(p); }
    static int check_kind(hzsdr_ctx *ctx, int mode) {
        if (mode != HZSDR_CARRIER_TONE && mode != HZSDR_CARRIER_BPSK && mode != HZSDR_CARRIER_QPSK)
            return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: the mode is HZSDR_CARRIER_TONE, _BPSK or _QPSK");
        return HZSDR_OK;
    }
    static void shape(hzsdr_carrier *f, int mode) {
        f->mode = mode;
        f->g = cp::carrier_geom(f->R, true);
        f->words = cp::state_words(f->R);
    }
    // the initial state: theta = 0, F = F0 of the row
    static void initial(const hzsdr_carrier *f, size_t r, size_t set, uint32_t *z) { z[cp::state_index(r, 1)] = (uint32_t)f->loop[set].f0; }
};

}  // namespace hz

extern "C" {

int hzsdr_carrier_create(hzsdr_ctx *ctx, int mode, const float *params, int per_row, size_t rows, hzsdr_carrier **out) {
    return hz::lb::create<hz::CarBank>(ctx, mode, params, per_row, rows, out);
}

int hzsdr_carrier_push(hzsdr_carrier *f, const void *in, size_t n, size_t in_stride, void *out, size_t out_stride, float *track,
                       size_t track_stride) {
    using namespace hz;
    return lb::push_rows(f, n, {in, in_stride, sizeof(float2)}, {out, n, out_stride, sizeof(float2)}, {track, n, track_stride, sizeof(float)},
                         [&](const lb::DevRows &d) {
                             CarArgs a{(const float2 *)d.in, d.in_stride, (float2 *)d.out, d.out_stride, d.track, d.track_stride, n, f->loop_rows,
                                       f->state, f->R, f->g.G, f->g.P, f->loop[0]};
                             return car_launch(f, a);
                         });
}

int hzsdr_carrier_set_params(hzsdr_carrier *f, const float *params) { return hz::lb::set_params<hz::CarBank>(f, params); }

int hzsdr_carrier_get_state(hzsdr_carrier *f, uint32_t *state, size_t cap) { return hz::lb::get_state(f, state, cap); }

int hzsdr_carrier_set_state(hzsdr_carrier *f, const uint32_t *state, size_t count, uint64_t position) {
    return hz::lb::set_state(f, state, count, position, "the state has rows * 2 words");
}

int hzsdr_carrier_position(const hzsdr_carrier *f, uint64_t *position) { return hz::lb::position(f, position); }

int hzsdr_carrier_plan(const hzsdr_carrier *f, size_t *rows_per_wave, size_t *tile_samples, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    return hz::lb::plan(f, rows_per_wave, tile_samples, form, (f->per_row ? HZSDR_CARRIER_FORM_PER_ROW : 0) + f->mode * HZSDR_CARRIER_FORM_MODE);
}

int hzsdr_carrier_reset(hzsdr_carrier *f) { return hz::lb::reset<hz::CarBank>(f); }

int hzsdr_carrier_free(hzsdr_carrier *f) { return f ? hz::lb::destroy(f, {f->loop_rows}) : HZSDR_ERR_INVALID_ARGUMENT; }

}  // extern "C"
