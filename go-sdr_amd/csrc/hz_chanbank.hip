// hz_chanbank.hip -- the channel bank (include/hzsdr_chanbank.h): the polyphase channelizer for any M from 2 to 255.
// Frames of a raw IQ stream converted in the loads, folded with the prototype's taps into Mp values indexed by absolute
// time modulo M, then y = W u as a float32 matrix product on v_mfma_f32_16x16x4_f32 -- A (2M x 2Mp, the DFT table as a
// real matrix in MFMA operand order, made at create) times B (2Mp x T, the tile's folded frames) -- and stored as
// complex rows (frame-major) or as one stream per channel (channel-major).  The term of the fold is hz_chanbank_math.h
// (shared with tests/host/chanbank_ref.cpp), the host arithmetic (tile, both layouts, table) is hz_chanbank_plan.h, the
// stream's (counts, rotation, position map) hz_polyphase_plan.h; the object's host side (create, the push around the
// launch, frames_for, pending, reset, free) is hz_polyphase.h.
//
// One kernel.  A workgroup of four waves takes T consecutive frames of a push, tile after tile.  The fold gives
// 2^fold_shift lanes to a frame (a wave folds 64 >> fold_shift frames at once; consecutive lanes read consecutive
// samples but for the rotation's wrap point) and writes B into LDS, (re, im) of one r side by side at an odd pitch: its
// stores spread over the banks and every B-operand read is 32 consecutive floats per half wave.  The rotation jD mod M
// is applied to the load indices; the padding r and the frames behind the push's last one are +0.  Then the 16-row
// tiles of A are dealt to the waves in groups of two; a wave holds 2 x T/16 accumulators and per k-step loads
// two values of A (from LDS where A fits beside B, else coalesced from device memory: 256 bytes per wave and
// value) and T/16 of B.  Channel-major runs the MFMA as A B: a lane holds 16 consecutive frames' worth of one channel
// pair across its 16-lane group, stored as runs of 128 bytes per channel.  Frame-major runs it as (A B)^T = B^T A^T --
// the SAME operand registers exchanged, the same chain of fused steps per output since a product commutes -- so that a
// 16-lane group holds (re, im) of 8 consecutive channels of one frame and stores 64 consecutive bytes of its row.
// make NO_PK_F32=1 (csrc/Makefile): no packed float32 instruction in this unit's device code, as in hz_tuner.hip
#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "hz_chain_host.h"
#include "../../include/hzsdr_chanbank.h"
#include "hz_chanbank_math.h"
#include "hz_chanbank_plan.h"
#include "hz_polyphase.h"

struct hzsdr_chanbank : hz::pp::Bank {
    static constexpr const char *noun = "chanbank", *create_name = "chanbank_create";
    static constexpr const char *format_why = "unknown source format", *channels_why = "the channel count is 2 ... 255 (hzsdr_channelizer.h from 256 on)";
    static constexpr hz::ppp::ChannelRule rule = hz::ppp::kMatrixRule;
    static constexpr auto destroy = hzsdr_chanbank_free;
    hz::cp::Geom g{};
    uint64_t magic = 0;
    std::vector<float> taps_host;
    std::vector<hz::cb::c32> W;  // M rows of Mp
    float *a_dev = nullptr;      // A in operand order
};

namespace hz {

struct CbArgs {
    const void *in;
    const float2 *tail;
    const float *taps, *A;
    uint64_t held, F, tiles;  // samples held; frames of the push; its tiles
    size_t stride;            // channel-major row pitch
    uint64_t magic;
    uint32_t M, Mp, P, D, rot, steps, pitch, groups, fold_shift, b_floats, a_floats, neg_first;
};

typedef float cb_f4 __attribute__((ext_vector_type(4)));

// NC: 16-frame column tiles of the workgroup's tile (T = 16 NC); A_LDS: A is staged in LDS behind B
template <int FMT, int NC, bool A_LDS, int LAYOUT>
__global__ __launch_bounds__(cp::kThreads) void chanbank_tile_kernel(CbArgs a, float2 *__restrict__ out) {
    using RT = typename Raw<FMT>::t;
    constexpr uint32_t T = NC * 16;
    [[maybe_unused]] constexpr uint32_t NR = cp::kGroupTiles;
    extern __shared__ __align__(16) unsigned char cb_lds[];
    float *B = (float *)cb_lds;
    [[maybe_unused]] float *Al = B + a.b_floats;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    [[maybe_unused]] const uint32_t n = lane & 15u, kk = lane >> 4;

    if constexpr (A_LDS)
        for (uint32_t i = tid; i < a.a_floats; i += cp::kThreads) Al[i] = a.A[i];  // (visible behind the first tile's barrier)

    const uint32_t fold_lanes = 1u << a.fold_shift, fold_frames = 64u >> a.fold_shift;
    const uint32_t fsub = lane >> a.fold_shift, r0 = lane & (fold_lanes - 1u);

    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        if (tile != blockIdx.x) __syncthreads();  // (the last tile's B is read no more)
        const uint64_t f0 = tile * T;
        // ---- the fold: B[2r + c][fl] of the tile's frames f0 + fl ----
        {
            const uint32_t rot0 = cp::chanbank_rot(a.rot, f0, a.D, a.M);
            for (uint32_t fl = wave * fold_frames + fsub; fl < T; fl += cp::kWaves * fold_frames) {
                const uint64_t f = f0 + fl;
                const bool live = f < a.F;
                const uint32_t w = rot0 + fl * a.D, s = w - div_by_magic(w, a.magic) * a.M;
                const uint64_t base = f * a.D;  // the frame's first sample in held ++ in
                for (uint32_t r = r0; r < a.Mp; r += fold_lanes) {
                    cb::c32 acc{0.0f, 0.0f};
                    if (live && r < a.M) {
                        uint32_t o = cp::chanbank_offset(r, s, a.M);
                        for (uint32_t p = 0; p < a.P; p++, o += a.M) {
                            const uint64_t v = base + o;
                            const float2 x = v < a.held ? a.tail[v] : Raw<FMT>::cvt(((const RT *)a.in)[v - a.held]);
                            acc = cb::chanbank_fold(acc, a.taps[o], cb::c32{x.x, x.y});
                        }
                    }
                    *(float2 *)(B + cp::chanbank_b_index(2 * r, fl, a.pitch)) = make_float2(acc.re, acc.im);
                }
            }
        }
        __syncthreads();
        // ---- the product: the groups of row tiles, dealt to the waves ----
#if defined(__HIP_DEVICE_COMPILE__)
        for (uint32_t grp = wave; grp < a.groups; grp += cp::kWaves) {
            cb_f4 acc[NR][NC];
#pragma unroll
            for (uint32_t i = 0; i < NR; i++)
#pragma unroll
                for (uint32_t j = 0; j < NC; j++) acc[i][j] = cb_f4{0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t rt0 = grp * NR;
            const size_t a_tile = (size_t)a.steps * 64;
            const float *ap = (A_LDS ? (const float *)Al : a.A) + (size_t)rt0 * a_tile + lane;
            // lane (n, kk) of a B read: element (4 s + kk, 16 j + n)
            const float *bp = B + cp::chanbank_b_index(kk, n, a.pitch);
            const uint32_t b_step = 4u * a.pitch;  // two r down
            for (uint32_t s = 0; s < a.steps; s++) {
                float av[NR], bv[NC];
#pragma unroll
                for (uint32_t i = 0; i < NR; i++) av[i] = ap[i * a_tile + (size_t)s * 64];
#pragma unroll
                for (uint32_t j = 0; j < NC; j++) bv[j] = bp[s * b_step + j * 32u];
#pragma unroll
                for (uint32_t i = 0; i < NR; i++)
#pragma unroll
                    for (uint32_t j = 0; j < NC; j++) {
                        if constexpr (LAYOUT == HZSDR_CHANNELIZER_CHANNEL_MAJOR)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
                        else
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bv[j], av[i], acc[i][j], 0, 0, 0);
                    }
            }
            // D layout: column lane & 15, row (lane >> 4) * 4 + reg
#pragma unroll
            for (uint32_t i = 0; i < NR; i++) {
                if constexpr (LAYOUT == HZSDR_CHANNELIZER_CHANNEL_MAJOR) {
                    // rows are rows of A: registers (0, 1) and (2, 3) are (re, im) of two channels; columns are frames
#pragma unroll
                    for (uint32_t hh = 0; hh < 2; hh++) {
                        const uint32_t k = (rt0 + i) * 8u + kk * 2u + hh;
                        if (k >= a.M) continue;
                        float2 *o = out + (size_t)cp::chanbank_pos(k, a.M, a.neg_first) * a.stride;
#pragma unroll
                        for (uint32_t j = 0; j < NC; j++) {
                            const uint64_t f = f0 + j * 16u + n;
                            if (f < a.F) o[f] = make_float2(acc[i][j][2 * hh], acc[i][j][2 * hh + 1]);
                        }
                    }
                } else {
                    // columns are rows of A: the lane's n is (channel, component); rows are frames
                    const uint32_t k = (rt0 + i) * 8u + (n >> 1);
                    if (k >= a.M) continue;
                    float *o = (float *)out + (size_t)cp::chanbank_pos(k, a.M, a.neg_first) * 2u + (n & 1u);
#pragma unroll
                    for (uint32_t j = 0; j < NC; j++)
#pragma unroll
                        for (uint32_t q = 0; q < 4; q++) {
                            const uint64_t f = f0 + j * 16u + kk * 4u + q;
                            if (f < a.F) o[f * (2u * a.M)] = acc[i][j][q];
                        }
                }
            }
        }
#endif
    }
}

template <int FMT, int NC, bool A_LDS>
static int cb_launch_form(hzsdr_chanbank *c, const CbArgs &a, float2 *out) {
    // (tile after tile in a workgroup once the chip is full many times over: A is staged once per workgroup)
    const uint64_t cap = (uint64_t)c->ctx->num_cus * 16;
    const dim3 grid((unsigned)(a.tiles < cap ? a.tiles : cap)), block(cp::kThreads);
    HZ_TRY(pp::with_layout(c->layout, [&](auto l) {
        return launch_fv(chanbank_tile_kernel<FMT, NC, A_LDS, decltype(l)::value>, grid, block, c->g.lds_bytes, c->ctx->stream, a, out);
    }));
    HZ_HIP(c->ctx, hipGetLastError());
    return HZSDR_OK;
}

template <int FMT>
static int cb_launch_fmt(hzsdr_chanbank *c, const CbArgs &a, float2 *out) {
    const bool al = c->g.a_lds;
    if (c->g.col_tiles == 4) return al ? cb_launch_form<FMT, 4, true>(c, a, out) : cb_launch_form<FMT, 4, false>(c, a, out);
    return cb_launch_form<FMT, 2, false>(c, a, out);  // (M above 128: A is far past the budget)
}

static int cb_launch(hzsdr_chanbank *c, const CbArgs &a, float2 *out) {
    return with_format(c->fmt, [&](auto f) { return cb_launch_fmt<decltype(f)::value>(c, a, out); });
}

// what create makes on the host: the tile, the table and A in operand order
static void cb_host_tables(hzsdr_chanbank *c, const float *taps, std::vector<float> &A) {
    c->g = cp::chanbank_geom(c->M);
    c->magic = div_magic(c->M);
    c->taps_host.assign(taps, taps + c->L);
    c->W = cp::chanbank_tables(c->M);
    A = cp::chanbank_fill_a(c->g, c->W);
}

}  // namespace hz

// (the table's move into the object stays in the library's symbol table whatever was inlined above)
template std::vector<hz::cb::c32> &std::vector<hz::cb::c32>::operator=(std::vector<hz::cb::c32> &&);

extern "C" {

int hzsdr_chanbank_create(hzsdr_ctx *ctx, int src_format, size_t channels, const float *taps, size_t n_taps, size_t hop, int order,
                          int layout, hzsdr_chanbank **out) {
    using namespace hz;
    std::vector<float> A;  // (local: free to go when create returns)
    return pp::create(ctx, src_format, channels, taps, n_taps, hop, order, layout, out, [&](hzsdr_chanbank *c, std::vector<Table> &tables) {
        cb_host_tables(c, taps, A);
        tables.push_back({(void **)&c->a_dev, A.data(), A.size() * sizeof(float)});
        return HZSDR_OK;
    });
}

int hzsdr_chanbank_frames_for(const hzsdr_chanbank *c, size_t n_in, size_t *frames) { return hz::pp::frames_for(c, n_in, frames); }

int hzsdr_chanbank_push(hzsdr_chanbank *c, const void *in, size_t n_in, void *out, size_t out_frames_cap, size_t out_stride,
                        size_t *frames_written) {
    using namespace hz;
    return pp::push_frames(c, in, n_in, out, out_frames_cap, out_stride, frames_written, [&](const void *din, float2 *dout, size_t dstride, const ppp::Step &p) {
        const cp::Geom &g = c->g;
        const CbArgs a{din, c->held.now(), c->taps, c->a_dev, c->st.held, p.F, (p.F + g.T - 1) / g.T, dstride, c->magic,
                       c->M, g.Mp, c->L / c->M, c->D, c->st.rot, g.steps, g.pitch, g.groups, g.fold_shift, g.b_floats, (uint32_t)g.a_floats,
                       (uint32_t)c->negative_first()};
        return cb_launch(c, a, dout);
    });
}

int hzsdr_chanbank_pending(const hzsdr_chanbank *c, size_t *samples_held, uint64_t *frame_index) { return hz::pp::pending(c, samples_held, frame_index); }

int hzsdr_chanbank_plan(const hzsdr_chanbank *c, size_t *tile_frames, size_t *tile_rows, int *form) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (tile_frames) *tile_frames = c->g.T;
    if (tile_rows) *tile_rows = (size_t)c->g.row_tiles * 16;
    if (form) *form = c->g.a_lds ? HZSDR_CHANBANK_FORM_A_LDS : 0;
    return HZSDR_OK;
}

int hzsdr_chanbank_readout(const hzsdr_chanbank *c, int what, size_t index, void *dst, size_t cap) {
    using namespace hz;
    if (!c || !dst) return HZSDR_ERR_INVALID_ARGUMENT;
    const void *src;
    size_t n, size;
    switch (what) {
    case HZSDR_CHANBANK_READ_DFT:
        if (index >= c->M) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "chanbank: no such row of the table");
        src = c->W.data() + index * c->g.Mp, n = c->g.Mp, size = sizeof(cb::c32);
        break;
    case HZSDR_CHANBANK_READ_TAPS: src = c->taps_host.data(), n = c->L, size = sizeof(float); break;
    default: return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "chanbank: unknown read-out");
    }
    if (cap < n) return fail(c->ctx, HZSDR_ERR_DST_TOO_SMALL, "chanbank: the read-out buffer is too small");
    memcpy(dst, src, n * size);
    return HZSDR_OK;
}

int hzsdr_chanbank_reset(hzsdr_chanbank *c) { return hz::pp::reset(c); }

int hzsdr_chanbank_free(hzsdr_chanbank *c) { return hz::pp::release(c, {c ? c->a_dev : nullptr}); }

}  // extern "C"

#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
