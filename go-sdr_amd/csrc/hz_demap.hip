// hz_demap.hip -- the demapper bank (include/hzsdr_demap.h): frames of received symbols to per-bit soft values in the
// decoder's order and sign, over R rows of `cap` frame slots with a count per row.  The arithmetic of a symbol is
// hz_demap_math.h (shared with the host restatement of tests/host/demap_ref.cpp); the host arithmetic (the validation,
// the dealing of frames to workgroups and threads, the LDS request) is hz_demap_plan.h; the call around the kernel is the
// decoder banks' (hz_decodebank.h).
//
// One kernel, instantiated per kind and per m, so that a point's label bits select its accumulators at compile time.  A
// workgroup takes G frames side by side, frame g on the threads [g T, (g + 1) T), T a multiple of 64, and walks on from
// one group of slots to the next.  Per frame:
//   1. lane = symbol: a thread reads its symbol (coalesced over the wave), takes the 2 m minima over the M points -- the
//      points come from the constant address space under compile-time offsets, so they are wave-uniform scalar loads --
//      and writes its m values L[s m ... s m + m - 1] into the frame's LDS, as one vector where m allows;
//   2. behind a barrier, lane = output: out[k] = L[perm[k]] (or L[k]), the flip bit applied on the bit pattern, any NaN
//      canonical: consecutive lanes store consecutive floats whatever the permutation.
// Nothing data-dependent indexes memory: every perm entry was checked at create.  No inline assembly, vector stores only.
#include <string>
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_demap.h"
#include "hz_decodebank.h"
#include "hz_demap_math.h"
#include "hz_demap_plan.h"
#include "hz_received.h"

struct hzsdr_demap : hz::db::Bank {
    static constexpr const char *noun = "demap";
    hz::dmp::Config q;
    hz::dmp::Geom g{};
    float *points = nullptr, *gains = nullptr;
    uint32_t *perm = nullptr;
    uint8_t *flip = nullptr;
};

namespace hz {

struct DmArgs : dbp::FrameArgs {  // (in and out are floats, the strides count floats, info is null)
    const float *points, *gains;
    const uint32_t *perm;
    const uint8_t *flip;
    uint32_t cap, slots;  // slots: R * cap
    uint32_t S, W, N, T, G, frame_floats, per_row_gain;
};

typedef const float __attribute__((address_space(4))) *ConstFloats;

// m consecutive floats at a multiple of m floats (the frame's base is 16-byte aligned)
template <int m> __device__ __forceinline__ void store_values(float *dst, const float *v) {
    if constexpr (m % 4 == 0) {
#pragma unroll
        for (int j = 0; j < m; j += 4) *(float4 *)(dst + j) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
    } else if constexpr (m % 2 == 0) {
#pragma unroll
        for (int j = 0; j < m; j += 2) *(float2 *)(dst + j) = make_float2(v[j], v[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < m; j++) dst[j] = v[j];
    }
}

template <int KIND, int m, bool TREE>
__global__ __launch_bounds__(dmp::kMaxThreads) void demap_frames_kernel(DmArgs a) {
    extern __shared__ __align__(16) unsigned char dm_lds[];
    const uint32_t tid = threadIdx.x, g = tid / a.T, t = tid - g * a.T;
    float *L = (float *)dm_lds + (size_t)g * a.frame_floats;
    const ConstFloats pts = (ConstFloats)a.points;

#pragma unroll 1
    for (uint32_t base = blockIdx.x * a.G; base < a.slots; base += gridDim.x * a.G) {
        // the group's slots: which hold a frame (the same answer on every thread)
        bool any = false, act = false;
        uint32_t row = 0, f = 0;
        for (uint32_t k = 0; k < a.G; k++) {
            const uint32_t slot = base + k;
            if (slot >= a.slots) break;
            uint32_t rr, ff;
            const bool live = dbp::slot_frame(slot, a.cap, a.in_counts, &rr, &ff);
            any |= live;
            if (k == g) act = live, row = rr, f = ff;
        }
        if (!any) continue;  // workgroup-uniform

        // 1. lane = symbol
        if (act) {
            const float *src = (const float *)a.in + (size_t)row * a.in_stride + (size_t)f * a.W;
            const float gain = a.gains[a.per_row_gain ? row : 0];
#pragma unroll 1
            for (uint32_t s = t; s < a.S; s += a.T) {
                if constexpr (KIND == dmp::kLlrF32) {
                    L[s] = src[s] * gain;
                } else {
                    constexpr bool cplx = KIND == dmp::kC64;
                    const float xr = cplx ? src[2 * s] : src[s], xi = cplx ? src[2 * s + 1] : 0.0f;
                    float d0[m], d1[m], v[m];
                    // (s is below 2^13: the offset is 0, wave-uniform, and renewed per symbol, so that the 2 M scalar
                    // loads stay inside the loop beside their uses; hoisted, they spill into vector lanes)
                    const ConstFloats p = pts + __builtin_amdgcn_readfirstlane((int)(s >> 13));
                    if constexpr (TREE)
                        dm::symbol_tree<m, cplx>(xr, xi, p, d0, d1);
                    else
                        dm::symbol_naive<m, cplx>(xr, xi, p, d0, d1);
                    const bool erased = xr != xr || xi != xi;
#pragma unroll
                    for (int j = 0; j < m; j++) v[j] = erased ? dm::float_of(dm::kNanBits) : dm::llr(d0[j], d1[j], gain);
                    store_values<m>(L + (size_t)s * m, v);
                }
            }
        }
        __syncthreads();

        // 2. lane = output
        if (act) {
            uint32_t *dst = (uint32_t *)a.out + (size_t)row * a.out_stride + (size_t)f * a.N;
#pragma unroll 1
            for (uint32_t k = t; k < a.N; k += a.T) {
                const uint32_t at = a.perm ? a.perm[k] : k;
                const float v = at == dm::kErased ? dm::float_of(dm::kNanBits) : L[at];
                dst[k] = dm::stored(v, a.flip ? rx::packed_bit(a.flip, k) : 0u);
            }
        }
        __syncthreads();  // (the next group's values overwrite these)
    }
}

template <int KIND, int m> static int launch_m(const dmp::Geom &g, const DmArgs &a, uint32_t slots, hipStream_t s) {
    const dim3 grid(dmp::groups_for(g, slots)), block(g.G * g.T);
    constexpr bool tree = KIND != dmp::kLlrF32 && m >= (int)dmp::kTreeFrom;
    return launch_fv(demap_frames_kernel<KIND, m, tree>, grid, block, g.lds_bytes, s, a);
}
template <int KIND> static int launch_kind(const dmp::Geom &g, const DmArgs &a, uint32_t slots, hipStream_t s) {
    switch (g.m) {
        case 1: return launch_m<KIND, 1>(g, a, slots, s);
        case 2: return launch_m<KIND, 2>(g, a, slots, s);
        case 3: return launch_m<KIND, 3>(g, a, slots, s);
        case 4: return launch_m<KIND, 4>(g, a, slots, s);
        case 5: return launch_m<KIND, 5>(g, a, slots, s);
        case 6: return launch_m<KIND, 6>(g, a, slots, s);
        case 7: return launch_m<KIND, 7>(g, a, slots, s);
        default: return launch_m<KIND, 8>(g, a, slots, s);
    }
}

}  // namespace hz

extern "C" {

int hzsdr_demap_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, const float *points, size_t symbols, const uint32_t *perm,
                       size_t received, const uint8_t *flip, const float *gains, size_t n_gains, size_t rows, hzsdr_demap **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!dmp::known(kind)) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "demap: complex symbols, real symbols or per-bit values");
    const dmp::Config q{kind, bits_per_symbol, symbols, received, points != nullptr, perm != nullptr, n_gains, rows};
    if (const char *why = dmp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("demap: ") + why);
    if (const char *why = dmp::check_arrays(q, points, perm, gains)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("demap: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_demap *d = new hzsdr_demap{{ctx, (uint32_t)rows}, q};
    d->g = dmp::geom(q);
    const size_t npoints = kind == dmp::kLlrF32 ? 0 : ((size_t)(kind == dmp::kC64 ? 2 : 1) << q.m);
    const int rc = db::upload(ctx, "demap_create",
                              {{(void **)&d->points, points, npoints * sizeof(float)},
                               {(void **)&d->gains, gains, n_gains * sizeof(float)},
                               {(void **)&d->perm, perm, perm ? received * sizeof(uint32_t) : 0},
                               {(void **)&d->flip, flip, flip ? dbp::packed_bytes((uint32_t)received) : 0}});
    if (rc != HZSDR_OK) {
        hzsdr_demap_free(d);
        return rc;
    }
    *out = d;
    return HZSDR_OK;
}

int hzsdr_demap_run(hzsdr_demap *d, const float *in, size_t in_stride, const uint32_t *in_counts, size_t cap, float *out, size_t out_stride) {
    using namespace hz;
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    const dmp::Geom &g = d->g;
    const dbp::Call c{(uintptr_t)in, (uintptr_t)out, in_stride, g.W, out_stride, g.N, cap, d->R, true};
    return db::run(
        d, dmp::slots_of(g), sizeof(float), sizeof(float), c, in_counts, nullptr, [&](const char **why) { return dmp::check_run(g, c, why); },
        [&](const dbp::FrameArgs &fa, uint32_t cap, uint32_t slots) {
            DmArgs a{};
            static_cast<dbp::FrameArgs &>(a) = fa;
            a.points = d->points, a.gains = d->gains, a.perm = d->perm, a.flip = d->flip;
            a.cap = cap, a.slots = slots;
            a.S = g.S, a.W = g.W, a.N = g.N, a.T = g.T, a.G = g.G, a.frame_floats = g.frame_floats, a.per_row_gain = d->q.n_gains > 1;
            hipStream_t s = d->ctx->stream;
            if (d->q.kind == dmp::kC64) return launch_kind<dmp::kC64>(g, a, slots, s);
            if (d->q.kind == dmp::kRealF32) return launch_kind<dmp::kRealF32>(g, a, slots, s);
            return launch_m<dmp::kLlrF32, 1>(g, a, slots, s);
        });
}

int hzsdr_demap_sizes(const hzsdr_demap *d, size_t *S, size_t *W, size_t *m, size_t *N) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    if (S) *S = d->g.S;
    if (W) *W = d->g.W;
    if (m) *m = d->g.m;
    if (N) *N = d->g.N;
    return HZSDR_OK;
}

int hzsdr_demap_plan(const hzsdr_demap *d, size_t *frames_per_group, size_t *threads_per_frame, size_t *frame_lds_bytes, int *form) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    if (frames_per_group) *frames_per_group = d->g.G;
    if (threads_per_frame) *threads_per_frame = d->g.T;
    if (frame_lds_bytes) *frame_lds_bytes = (size_t)d->g.frame_floats * 4;
    if (form) *form = d->g.form;
    return HZSDR_OK;
}

int hzsdr_demap_free(hzsdr_demap *d) {
    if (!d) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(d->ctx, {d->points, d->gains, d->perm, d->flip});
    delete d;
    return HZSDR_OK;
}

}  // extern "C"
