// hz_iir.hip -- the IIR bank (include/hzsdr_iir.h): a cascade of S biquads in transposed direct form II over R rows, real
// or complex.  The arithmetic of every output is hz_iir_math.h (shared with the host restatement of
// tests/host/iir_ref.cpp); the host arithmetic is hz_iir_plan.h.
//
// One kernel, a row-wave one: the wave, its tile and the four steps of a tile are described in hz_rowwave.h, which
// holds the wave's sync, the wait before the loop and the fetch.  Lane l < G keeps its row's coefficients and its 2 S
// (4 S for complex rows) state values in registers from the first tile to the last, reads them from the object's state
// array before and writes them back behind.  The walk is the recursion: eight samples read ahead of the chain, each y
// written over its x; the loop-carried path is two dependent fused steps per section (y -> z1 -> y).  The tile is read
// back as it was written.
// A shared cascade travels in the kernel's arguments: wave-uniform scalars, never lane by lane.
#include <cmath>

#include "hz_chain_host.h"
#include "../../include/hzsdr_iir.h"
#include "hz_iir_math.h"
#include "hz_iir_plan.h"
#include "hz_loopbank.h"
#include "hz_rowwave.h"

struct hzsdr_iir : hz::lb::Bank<float> {  // the state: ip::state_floats, ip::state_index
    static constexpr const char *noun = "iir";
    int kind = 0;
    uint32_t S = 0;
    hz::ip::Geom g{};
    std::vector<float> coef;     // the host's copy: S * 5, or R * S * 5
    float *coef_rows = nullptr;  // per_row: the same on the device
};

namespace hz {

struct IirArgs {
    const void *in;  // row r starts r * in_stride samples in
    size_t in_stride;
    void *out;
    size_t out_stride;
    uint64_t n;  // samples per row in the push
    const float *coef_rows;
    float *state;
    uint32_t R, S, G, P;
    float coef[ip::kMaxSections * im::kCoefs];  // the shared cascade, +0 behind its S sections
};

template <int KIND> struct IirSrc {
    using RT = typename Raw<KIND>::t;
    using OT = float2;
    static constexpr int PL = 2;
    static __device__ __forceinline__ float2 cvt(RT r) { return Raw<KIND>::cvt(r); }
    static __device__ __forceinline__ float2 pack(float re, float im) { return make_float2(re, im); }
};
template <> struct IirSrc<HZSDR_IIR_REAL_F32> {
    using RT = float;
    using OT = float;
    static constexpr int PL = 1;
    static __device__ __forceinline__ float2 cvt(float r) { return make_float2(r, 0.0f); }
    static __device__ __forceinline__ float pack(float re, float) { return re; }
};

// lane = row: samples [0, tn) of the tile through the S sections, y over x.  Eight samples are read before the chain
// that consumes them, so that no LDS latency sits on the loop-carried path.
template <int S, int PL>
__device__ __forceinline__ void iir_walk(float *tl, uint32_t P, uint32_t T, uint32_t tn, const float (&c)[ip::kMaxSections][im::kCoefs],
                                         float (&z)[ip::kMaxSections][2][PL]) {
    uint32_t t = 0;
#pragma unroll 1
    for (; t + 8 <= tn; t += 8) {
        float x[8][PL];
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int p = 0; p < PL; p++) x[j][p] = tl[ip::walk_slot(0, t + j, p, P, T)];
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int p = 0; p < PL; p++) {
                float v = x[j][p];
#pragma unroll
                for (int s = 0; s < S; s++) v = im::iir_step(c[s], v, z[s][0][p], z[s][1][p]);
                x[j][p] = v;
            }
#pragma unroll
        for (int j = 0; j < 8; j++)
#pragma unroll
            for (int p = 0; p < PL; p++) tl[ip::walk_slot(0, t + j, p, P, T)] = x[j][p];
    }
#pragma unroll 1
    for (; t < tn; t++) {
#pragma unroll
        for (int p = 0; p < PL; p++) {
            float v = tl[ip::walk_slot(0, t, p, P, T)];
#pragma unroll
            for (int s = 0; s < S; s++) v = im::iir_step(c[s], v, z[s][0][p], z[s][1][p]);
            tl[ip::walk_slot(0, t, p, P, T)] = v;
        }
    }
}

template <int KIND, int K, bool PER_ROW>
__global__ __launch_bounds__(ip::kLanes) void iir_rows_kernel(IirArgs a) {
    using Src = IirSrc<KIND>;
    using RT = typename Src::RT;
    using OT = typename Src::OT;
    constexpr int PL = Src::PL;
    constexpr uint32_t T = ip::kLanes * K;
    extern __shared__ __align__(16) unsigned char iir_lds[];
    float *tile = (float *)iir_lds;
    const auto [lane, row0, g, own, row] = rw::wave(a);

    float c[ip::kMaxSections][im::kCoefs];
    float z[ip::kMaxSections][2][PL];
#pragma unroll
    for (uint32_t s = 0; s < ip::kMaxSections; s++) {
#pragma unroll
        for (int k = 0; k < im::kCoefs; k++) c[s][k] = PER_ROW ? 0.0f : a.coef[s * im::kCoefs + k];
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int p = 0; p < PL; p++) z[s][q][p] = 0.0f;
        if (own && s < a.S) {
            if (PER_ROW) {
#pragma unroll
                for (int k = 0; k < im::kCoefs; k++) c[s][k] = a.coef_rows[(row * a.S + s) * im::kCoefs + k];
            }
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int p = 0; p < PL; p++) z[s][q][p] = a.state[ip::state_index(row, s, q, p, a.S, PL)];
        }
    }

    const RT *in = (const RT *)a.in + (size_t)row0 * a.in_stride;
    OT *out = (OT *)a.out + (size_t)row0 * a.out_stride;
    RT raw[ip::kMaxGroup][K];
    rw::fetch<RT, K>(raw, in, a.in_stride, g, 0, a.n, lane);
#pragma unroll
    for (uint32_t s = 0; s < ip::kMaxSections; s++) {
#pragma unroll
        for (int k = 0; k < im::kCoefs; k++) rw::settle(c[s][k]);
#pragma unroll
        for (int q = 0; q < 2; q++)
#pragma unroll
            for (int p = 0; p < PL; p++) rw::settle(z[s][q][p]);
    }
#pragma unroll 1
    for (uint64_t t0 = 0; t0 < a.n; t0 += T) {
        const uint64_t left = a.n - t0;
        const uint32_t tn = left < T ? (uint32_t)left : T;
        // 1. converted, into the tile: row fixed, lane = sample
#pragma unroll
        for (uint32_t r = 0; r < ip::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if (lane + ip::kLanes * k < tn) {
                        const float2 v = Src::cvt(raw[r][k]);
                        tile[ip::move_slot(lane, k, r, 0, a.P, T)] = v.x;
                        if (PL == 2) tile[ip::move_slot(lane, k, r, 1, a.P, T)] = v.y;
                    }
                }
            }
        }
        rw::wave_sync();
        // 2. the next tile's loads, in flight under the recursion
        if (left > T) rw::fetch<RT, K>(raw, in, a.in_stride, g, t0 + T, a.n, lane);
        // 3. lane = row
        if (own) {
            float *tl = tile + lane;
            switch (a.S) {
            case 1: iir_walk<1, PL>(tl, a.P, T, tn, c, z); break;
            case 2: iir_walk<2, PL>(tl, a.P, T, tn, c, z); break;
            case 3: iir_walk<3, PL>(tl, a.P, T, tn, c, z); break;
            case 4: iir_walk<4, PL>(tl, a.P, T, tn, c, z); break;
            case 5: iir_walk<5, PL>(tl, a.P, T, tn, c, z); break;
            case 6: iir_walk<6, PL>(tl, a.P, T, tn, c, z); break;
            case 7: iir_walk<7, PL>(tl, a.P, T, tn, c, z); break;
            default: iir_walk<8, PL>(tl, a.P, T, tn, c, z); break;
            }
        }
        rw::wave_sync();
        // 4. out of the tile: row fixed, lane = sample
#pragma unroll
        for (uint32_t r = 0; r < ip::kMaxGroup; r++) {
            if (r < g) {
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const uint32_t t = lane + ip::kLanes * k;
                    if (t < tn) {
                        const float re = tile[ip::move_slot(lane, k, r, 0, a.P, T)];
                        const float im = PL == 2 ? tile[ip::move_slot(lane, k, r, 1, a.P, T)] : 0.0f;
                        out[r * a.out_stride + t0 + t] = Src::pack(re, im);
                    }
                }
            }
        }
        rw::wave_sync();  // (the next tile's samples overwrite these)
    }

    if (own) {
#pragma unroll
        for (uint32_t s = 0; s < ip::kMaxSections; s++) {
            if (s < a.S) {
#pragma unroll
                for (int q = 0; q < 2; q++)
#pragma unroll
                    for (int p = 0; p < PL; p++) a.state[ip::state_index(row, s, q, p, a.S, PL)] = z[s][q][p];
            }
        }
    }
}

static bool iir_complex(int kind) { return kind != HZSDR_IIR_REAL_F32; }
static size_t iir_in_size(int kind) { return kind == HZSDR_IIR_REAL_F32 ? sizeof(float) : (size_t)format_size(kind); }
static size_t iir_out_size(int kind) { return iir_complex(kind) ? sizeof(float2) : sizeof(float); }

template <int KIND, int K>
static int iir_launch_kind(hzsdr_iir *f, const IirArgs &a) {
    const dim3 grid(f->g.waves), block(ip::kLanes);
    if (f->per_row)
        HZ_TRY(launch_fv(iir_rows_kernel<KIND, K, true>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    else
        HZ_TRY(launch_fv(iir_rows_kernel<KIND, K, false>, grid, block, f->g.lds_bytes, f->ctx->stream, a));
    HZ_HIP(f->ctx, hipGetLastError());
    return HZSDR_OK;
}

static int iir_launch(hzsdr_iir *f, const IirArgs &a) {
    constexpr int K = ip::kSteps;  // (the plan's: f->g.K)
    switch (f->kind) {
    case HZSDR_IIR_REAL_F32: return iir_launch_kind<HZSDR_IIR_REAL_F32, K>(f, a);
    case HZSDR_FMT_C64: return iir_launch_kind<HZSDR_FMT_C64, K>(f, a);
    case HZSDR_FMT_I16: return iir_launch_kind<HZSDR_FMT_I16, K>(f, a);
    case HZSDR_FMT_U8: return iir_launch_kind<HZSDR_FMT_U8, K>(f, a);
    default: return iir_launch_kind<HZSDR_FMT_I8, K>(f, a);
    }
}

static size_t iir_coefs(const hzsdr_iir *f) { return (size_t)(f->per_row ? f->R : 1) * f->S * im::kCoefs; }
static size_t iir_state_bytes(const hzsdr_iir *f) { return f->words * sizeof(float); }

static int iir_check_sections(hzsdr_ctx *ctx, const float *sections, size_t count) {
    if (!sections) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "iir: null sections");
    for (size_t k = 0; k < count; k++)
        if (!std::isfinite(sections[k])) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "iir: a coefficient is not finite");
    return HZSDR_OK;
}

// the object's host copy of the coefficients onto the device (per-row cascades; a shared one travels with each launch)
static int iir_upload(hzsdr_iir *f) {
    return f->per_row ? bank_upload(f->ctx, f->coef_rows, f->coef.data(), f->coef.size() * sizeof(float)) : HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_iir_create(hzsdr_ctx *ctx, int kind_or_format, const float *sections, size_t n_sections, int per_row, size_t rows,
                     hzsdr_iir **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind_or_format != HZSDR_IIR_REAL_F32 && format_size(kind_or_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "iir: unknown input kind");
    if (n_sections == 0 || n_sections > ip::kMaxSections) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "iir: 1 ... 8 sections");
    if (rows == 0 || rows > ip::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "iir: 1 ... 8192 rows");
    hzsdr_iir *f = new hzsdr_iir{};
    f->ctx = ctx, f->R = (uint32_t)rows, f->per_row = per_row != 0, f->kind = kind_or_format, f->S = (uint32_t)n_sections;
    auto undo = [&](int rc) {
        hzsdr_iir_free(f);
        return rc;
    };
    int rc = iir_check_sections(ctx, sections, iir_coefs(f));
    if (rc == HZSDR_OK) rc = enter(ctx);
    if (rc != HZSDR_OK) {
        delete f;
        return rc;
    }
    f->g = ip::iir_geom(f->R, (uint32_t)iir_in_size(f->kind), iir_complex(f->kind));
    f->words = ip::state_floats(f->R, f->S, f->g.planes);
    f->coef.assign(sections, sections + iir_coefs(f));
    hipError_t e = hipMalloc((void **)&f->state, iir_state_bytes(f));
    if (e == hipSuccess && f->per_row) e = hipMalloc((void **)&f->coef_rows, f->coef.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemsetAsync(f->state, 0, iir_state_bytes(f), ctx->stream);
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "iir_create", __FILE__, __LINE__));
    rc = iir_upload(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_iir_push(hzsdr_iir *f, const void *in, size_t n, size_t in_stride, void *out, size_t out_cap, size_t out_stride,
                   size_t *written) {
    using namespace hz;
    if (written) *written = 0;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(lb::push_rows(f, n, {in, in_stride, iir_in_size(f->kind)}, {out, out_cap, out_stride, iir_out_size(f->kind)}, {}, [&](const lb::DevRows &d) {
        IirArgs a{d.in, d.in_stride, d.out, d.out_stride, n, f->coef_rows, f->state, f->R, f->S, f->g.G, f->g.P, {}};
        if (!f->per_row)
            for (size_t k = 0; k < f->coef.size(); k++) a.coef[k] = f->coef[k];
        return iir_launch(f, a);
    }));
    if (written) *written = n;
    return HZSDR_OK;
}

int hzsdr_iir_set_sections(hzsdr_iir *f, const float *sections, size_t n_sections) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    if (n_sections != f->S) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "iir: the section count cannot change");
    HZ_TRY(iir_check_sections(f->ctx, sections, iir_coefs(f)));
    HZ_TRY(enter(f->ctx));
    f->coef.assign(sections, sections + iir_coefs(f));
    return iir_upload(f);  // (behind the pushes so far on the context's stream)
}

int hzsdr_iir_get_state(hzsdr_iir *f, float *state, size_t cap) { return hz::lb::get_state(f, state, cap); }

int hzsdr_iir_set_state(hzsdr_iir *f, const float *state, size_t count, uint64_t position) {
    return hz::lb::set_state(f, state, count, position, "the state has rows * sections * 2 (* 2) floats");
}

int hzsdr_iir_position(const hzsdr_iir *f, uint64_t *position) { return hz::lb::position(f, position); }

int hzsdr_iir_plan(const hzsdr_iir *f, size_t *rows_per_wave, size_t *tile_samples, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    return hz::lb::plan(f, rows_per_wave, tile_samples, form, (f->per_row ? HZSDR_IIR_FORM_PER_ROW : 0) | (f->g.planes == 2 ? HZSDR_IIR_FORM_COMPLEX : 0));
}

int hzsdr_iir_reset(hzsdr_iir *f) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    HZ_HIP(f->ctx, hipMemsetAsync(f->state, 0, iir_state_bytes(f), f->ctx->stream));
    f->pos = 0;
    return HZSDR_OK;
}

int hzsdr_iir_free(hzsdr_iir *f) { return f ? hz::lb::destroy(f, {f->coef_rows}) : HZSDR_ERR_INVALID_ARGUMENT; }

}  // extern "C"
