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
#include "hz_rowwave.h"

struct hzsdr_carrier {
    hzsdr_ctx *ctx;
    int mode;
    uint32_t R;
    bool per_row;
    hz::cp::Geom g{};
    std::vector<float> params;       // the caller's: 5, or R * 5
    std::vector<hz::cm::Loop> loop;  // derived from them: 1, or R
    hz::cm::Loop *loop_rows = nullptr;  // per_row: `loop` on the device
    uint32_t *state = nullptr;       // cp::state_words, cp::state_index
    uint64_t pos = 0;
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

static size_t car_param_sets(const hzsdr_carrier *f) { return f->per_row ? f->R : 1; }
static size_t car_state_bytes(const hzsdr_carrier *f) { return cp::state_words(f->R) * sizeof(uint32_t); }

static int car_check_params(hzsdr_ctx *ctx, const float *params, size_t sets) {
    if (!params) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: null params");
    for (size_t r = 0; r < sets; r++)
        if (const char *why = cp::check_params(params + r * cp::kParams)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("carrier: ") + why);
    return HZSDR_OK;
}

// validated parameters into the object: the host's copy, the derived constants, and the device's rows of constants
// (per-row parameters; shared ones travel with each launch).  The device's rows go first: a copy that fails leaves the
// object as it was.
static int car_take_params(hzsdr_carrier *f, const float *params) {
    const size_t sets = car_param_sets(f);
    std::vector<cm::Loop> loop(sets);
    for (size_t r = 0; r < sets; r++) loop[r] = cp::derive(params + r * cp::kParams);
    if (f->per_row) HZ_TRY(bank_upload(f->ctx, f->loop_rows, loop.data(), sets * sizeof(cm::Loop)));
    f->params.assign(params, params + sets * cp::kParams);
    f->loop.swap(loop);
    return HZSDR_OK;
}

// the initial state: theta = 0, F = F0 of the row
static int car_initial_state(hzsdr_carrier *f) {
    std::vector<uint32_t> z(cp::state_words(f->R), 0u);
    for (size_t r = 0; r < f->R; r++) z[cp::state_index(r, 1)] = (uint32_t)f->loop[f->per_row ? r : 0].f0;
    HZ_TRY(bank_upload(f->ctx, f->state, z.data(), car_state_bytes(f)));
    f->pos = 0;
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_carrier_create(hzsdr_ctx *ctx, int mode, const float *params, int per_row, size_t rows, hzsdr_carrier **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (mode != HZSDR_CARRIER_TONE && mode != HZSDR_CARRIER_BPSK && mode != HZSDR_CARRIER_QPSK)
        return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: the mode is HZSDR_CARRIER_TONE, _BPSK or _QPSK");
    if (rows == 0 || rows > cp::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: 1 ... 8192 rows");
    hzsdr_carrier *f = new hzsdr_carrier{ctx, mode, (uint32_t)rows, per_row != 0};
    auto undo = [&](int rc) {
        hzsdr_carrier_free(f);
        return rc;
    };
    int rc = car_check_params(ctx, params, car_param_sets(f));
    if (rc == HZSDR_OK) rc = enter(ctx);
    if (rc != HZSDR_OK) {
        delete f;
        return rc;
    }
    f->g = cp::carrier_geom(f->R, true);
    hipError_t e = hipMalloc((void **)&f->state, car_state_bytes(f));
    if (e == hipSuccess && f->per_row) e = hipMalloc((void **)&f->loop_rows, (size_t)f->R * sizeof(cm::Loop));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "carrier_create", __FILE__, __LINE__));
    rc = car_take_params(f, params);
    if (rc == HZSDR_OK) rc = car_initial_state(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_carrier_push(hzsdr_carrier *f, const void *in, size_t n, size_t in_stride, void *out, size_t out_stride, float *track,
                       size_t track_stride) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R;
    if (n && !in) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: null input");
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: in_stride is below the samples of the push");
    if (f->pos + n < f->pos) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: the push is too long");
    HZ_TRY(check_rows_out(ctx, "carrier", R, out, n, out_stride, n, 0));
    if (track) HZ_TRY(check_rows_out(ctx, "carrier track", R, track, n, track_stride, n, 0));
    if (n && in == out && R > 1 && in_stride != out_stride) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "carrier: in place needs equal strides");
    HZ_TRY(enter(ctx));
    if (n == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din;
    void *dout, *dtrack = nullptr;
    size_t dstride, ostride, tstride = 0;
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, sizeof(float2), &din, &dstride));
    HZ_TRY(st.out_rows(1, out, R, n, out_stride, sizeof(float2), &dout, &ostride));
    if (track) HZ_TRY(st.out_rows(2, track, R, n, track_stride, sizeof(float), &dtrack, &tstride));
    CarArgs a{(const float2 *)din, dstride, (float2 *)dout, ostride, (float *)dtrack, tstride, n, f->loop_rows, f->state, f->R, f->g.G, f->g.P,
              f->loop[0]};
    HZ_TRY(car_launch(f, a));
    f->pos += n;
    return st.finish();
}

int hzsdr_carrier_set_params(hzsdr_carrier *f, const float *params) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(car_check_params(f->ctx, params, car_param_sets(f)));
    HZ_TRY(enter(f->ctx));
    return car_take_params(f, params);  // (behind the pushes so far on the context's stream)
}

int hzsdr_carrier_get_state(hzsdr_carrier *f, uint32_t *state, size_t cap) {
    if (!f || !state) return HZSDR_ERR_INVALID_ARGUMENT;
    static_assert(sizeof(uint32_t) == sizeof(float), "the state's words move as the sibling banks' floats do");
    return hz::bank_state_get(f->ctx, "carrier", (float *)state, cap, (const float *)f->state, hz::cp::state_words(f->R));
}

int hzsdr_carrier_set_state(hzsdr_carrier *f, const uint32_t *state, size_t count, uint64_t position) {
    if (!f || !state) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(hz::bank_state_set(f->ctx, "carrier", (float *)f->state, (const float *)state, count, hz::cp::state_words(f->R),
                              "the state has rows * 2 words"));
    f->pos = position;
    return HZSDR_OK;
}

int hzsdr_carrier_position(const hzsdr_carrier *f, uint64_t *position) {
    if (!f || !position) return HZSDR_ERR_INVALID_ARGUMENT;
    *position = f->pos;
    return HZSDR_OK;
}

int hzsdr_carrier_plan(const hzsdr_carrier *f, size_t *rows_per_wave, size_t *tile_samples, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_per_wave) *rows_per_wave = f->g.G;
    if (tile_samples) *tile_samples = f->g.T;
    if (form) *form = (f->per_row ? HZSDR_CARRIER_FORM_PER_ROW : 0) + f->mode * HZSDR_CARRIER_FORM_MODE;
    return HZSDR_OK;
}

int hzsdr_carrier_reset(hzsdr_carrier *f) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return car_initial_state(f);
}

int hzsdr_carrier_free(hzsdr_carrier *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->loop_rows, f->state});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"
