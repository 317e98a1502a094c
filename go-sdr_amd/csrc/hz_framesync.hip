// hz_framesync.hip -- the frame sync bank (include/hzsdr_framesync.h): hard decisions, a sync-word search under up to
// four hypotheses, a hold-off and the frames' payload bits, over R rows of soft symbols with a count per row.  The
// arithmetic of every bit is hz_framesync_math.h (shared with the host restatement of tests/host/framesync_ref.cpp);
// the host arithmetic (the validation, where a window lies in the ring, the state's layout) is hz_framesync_plan.h.
//
// One kernel, a bit-ring kernel: the wave, its row, the tiles, the ring in the wave's LDS and the loop over them are
// hz_bitring.h, the object around it hz_framebank.h.  Nothing here is sequential along a row but the hold-off, and that
// runs over candidates.  Per tile, lane l tests the window of the frame that COMPLETES at the tile's bit l: two ring
// words (at most two distinct addresses over the wave: broadcasts), a funnel shift, and per hypothesis an xor, the mask
// and a population count, the words being wave-uniform scalars.  A ballot of the candidates is almost always zero;
// otherwise a wave-uniform loop over its set bits in ascending order applies the hold-off, claims slot f, and the 64
// lanes extract the frame from the ring a 64-bit word each: funnel shift, map, the bits of each byte reversed.
// No inline assembly, vector stores only.
#include "hz_chain_host.h"
#include "../../include/hzsdr_framesync.h"
#include "hz_framebank.h"
#include "hz_framesync_math.h"
#include "hz_framesync_plan.h"

struct hzsdr_framesync : hz::fb::Bank {  // a row's state: bits consumed, hold, last raw decision, g.HW words of history
    static constexpr const char *noun = "framesync";
    static constexpr uint32_t kStLast = hz::fp::kStLast, kStHist = hz::fp::kStHist;
    hz::fp::Config q;
    hz::fp::Geom g{};
};

namespace hz {

struct FsArgs : br::RowArgs {
    uint32_t B, W, P, K, c, FB, PW;
    uint32_t thr, H;
    uint64_t holdoff, mask;  // (the mask and the words in the stream's order: earliest bit lowest)
    uint64_t words[fp::kMaxHyp];
    uint32_t maps[fp::kMaxHyp];
};

template <bool B2>
__global__ __launch_bounds__(fp::kLanes) void framesync_rows_kernel(FsArgs a) {
    extern __shared__ __align__(16) unsigned char fs_lds[];
    uint64_t *ring = (uint64_t *)fs_lds;
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = fp::wave_first_row(blockIdx.x, a.G), g = fp::wave_row_count(blockIdx.x, a.G, a.R);

#pragma unroll 1
    for (uint32_t r = 0; r < g; r++) {
        const size_t row = (size_t)row0 + r;
        const br::Row w = br::open_row(a, ring, row, a.B, fp::kStLast, fp::kStHist, lane);
        const uint32_t m = w.m, tiles = br::tiles_of(m);
        const uint64_t bits0 = w.bits0;
        uint64_t hold = w.z[fp::kStHold];
        uint32_t carry = w.carry, f = 0;
        uint32_t cur[fp::kChunk], nxt[fp::kChunk];
        br::fetch(cur, w.in, a.step, 0, m, lane);
#pragma unroll 1
        for (uint32_t t0 = 0; t0 < tiles; t0 += fp::kChunk) {
            if (t0 + fp::kChunk < tiles) br::fetch(nxt, w.in, a.step, t0 + fp::kChunk, m, lane);
            br::chunk_words(a, ring, cur, t0, tiles, m, carry, lane);
            // the search: lane l, the frame that completes at the tile's bit l
#pragma unroll 1
            for (uint32_t t = t0; t < t0 + fp::kChunk && t < tiles; t++) {
                const uint32_t tn = br::tile_bits(t, m);
                const uint64_t x = br::ring_bits(ring, fp::window_bit(t, lane, a.c), a.RW);
                uint32_t best = 65u, bh = 0;
#pragma unroll
                for (uint32_t h = 0; h < fp::kMaxHyp; h++) {
                    if (h < a.H) {
                        const uint32_t d = fm::distance(x, a.words[h], a.mask);
                        if (d < best) best = d, bh = h;
                    }
                }
                const uint64_t done = bits0 + (uint64_t)t * fp::kTileBits + lane;  // the stream's bit that completes the frame
                const bool valid = lane < tn && done >= a.K && (!B2 || (lane & 1u));
                uint64_t cand = __ballot(valid && best <= a.thr);
                while (cand) {  // wave-uniform, ascending
                    const uint32_t l = (uint32_t)__builtin_ctzll(cand);
                    cand &= cand - 1;
                    const uint64_t start = bits0 + (uint64_t)t * fp::kTileBits + l + 1 - a.P;  // the payload's first bit: e + 1
                    const uint64_t s = B2 ? start >> 1 : start;
                    if (s < hold) continue;
                    hold = s + a.holdoff;
                    if (f < a.cap) {
                        const uint32_t d = __shfl(best, (int)l), hh = __shfl(bh, (int)l);
                        const uint32_t map = hh == 0 ? a.maps[0] : (hh == 1 ? a.maps[1] : (hh == 2 ? a.maps[2] : a.maps[3]));
                        const size_t slot = row * a.cap + f;
                        if (lane == 0) {
                            a.positions[slot] = s;
                            a.info[slot] = d | (hh << 8);
                        }
                        uint8_t *dst = a.out + row * a.out_stride + (size_t)f * a.FB;
                        const uint64_t pay = fp::window_bit(t, l, a.c) + a.W;
                        for (uint32_t j = lane; j < a.PW; j += fp::kLanes) {
                            const uint32_t bits = a.P - 64 * j < 64 ? a.P - 64 * j : 64;
                            const uint64_t p = fm::map_word(br::ring_bits(ring, pay + 64ull * j, a.RW), (int)map, B2) & fm::low_mask(bits);
                            br::store_out_word(dst, j, fm::out_word(p), a.FB - 8 * j < 8 ? a.FB - 8 * j : 8);
                        }
                    }
                    f++;
                }
            }
            br::rotate(cur, nxt);
        }
        if (lane == 0) w.z[fp::kStHold] = hold;
        br::close_row(a, ring, w, row, m, bits0, carry, f, fp::kStLast, fp::kStHist, lane);
    }
}

static bool fs_complex(const hzsdr_framesync *f) { return f->q.kind == HZSDR_FMT_C64; }

}  // namespace hz

extern "C" {

int hzsdr_framesync_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, unsigned word_bits, uint64_t mask, unsigned thr, unsigned hyps,
                           const uint64_t *words, const unsigned *maps, unsigned payload_bits, int diff, uint64_t holdoff, size_t rows,
                           hzsdr_framesync **out) {
    using namespace hz;
    HZ_TRY(fb::check_create(ctx, kind, rows, out));
    if (!words || !maps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: null words or maps");
    if (diff < 0) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: diff is 0, 1 or 2");
    fp::Config q{kind, bits_per_symbol, word_bits, mask, thr, hyps, {0, 0, 0, 0}, {0, 0, 0, 0}, payload_bits, (uint32_t)diff, holdoff};
    for (unsigned h = 0; h < hyps && h < fp::kMaxHyp; h++) q.words[h] = words[h], q.maps[h] = maps[h];
    if (const char *why = fp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("framesync: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_framesync *f = new hzsdr_framesync{};
    f->ctx = ctx, f->R = (uint32_t)rows, f->q = q, f->g = fp::geom(f->R, q.W, q.P);
    f->per = f->g.per, f->frame_bytes = f->g.FB, f->symbol_floats = fs_complex(f) ? 2 : 1;
    auto undo = [&](int rc) {
        hzsdr_framesync_free(f);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&f->state, fb::state_words(f) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->maxc, sizeof(uint32_t));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "framesync_create", __FILE__, __LINE__));
    const int rc = fb::initial_state(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_framesync_push(hzsdr_framesync *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap,
                         size_t out_stride, uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count) {
    using namespace hz;
    return fb::push(f, in, n, in_stride, in_counts, out, cap, out_stride, positions, info, counts, max_count, [&](const br::RowArgs &rows) {
        const fp::Config &q = f->q;
        const fp::Geom &g = f->g;
        FsArgs a{};
        (br::RowArgs &)a = rows;
        a.step = fs_complex(f) && q.B == 1 ? 2 : 1, a.diff = q.diff;
        a.B = q.B, a.W = q.W, a.P = q.P, a.K = g.K, a.c = g.c, a.FB = g.FB, a.PW = g.PW;
        a.thr = q.thr, a.H = q.H, a.holdoff = q.holdoff, a.mask = fm::reverse_bits(q.mask, q.W);
        for (uint32_t h = 0; h < q.H; h++) a.words[h] = fm::reverse_bits(q.words[h], q.W), a.maps[h] = q.maps[h];
        const dim3 grid(g.waves), block(fp::kLanes);
        if (q.B == 2) return launch_fv(framesync_rows_kernel<true>, grid, block, g.lds_bytes, f->ctx->stream, a);
        return launch_fv(framesync_rows_kernel<false>, grid, block, g.lds_bytes, f->ctx->stream, a);
    });
}

int hzsdr_framesync_get_state(hzsdr_framesync *f, uint64_t *positions, uint64_t *holds, uint8_t *history, uint8_t *last, size_t rows_cap) {
    using namespace hz;
    if (!f || !holds) return HZSDR_ERR_INVALID_ARGUMENT;
    return fb::get_state(f, positions, history, last, rows_cap, f->q.B, [&](size_t r, const uint64_t *zr) { holds[r] = zr[fp::kStHold]; });
}

int hzsdr_framesync_set_state(hzsdr_framesync *f, const uint64_t *positions, const uint64_t *holds, const uint8_t *history, const uint8_t *last,
                              size_t rows) {
    using namespace hz;
    if (!f || !holds) return HZSDR_ERR_INVALID_ARGUMENT;
    return fb::set_state(
        f, positions, history, last, rows, f->q.B, "a position above 2^62 or a last decision above 1", [](size_t) { return true; },
        [&](size_t r, uint64_t *zr) { zr[fp::kStHold] = holds[r]; });
}

int hzsdr_framesync_positions(hzsdr_framesync *f, uint64_t *positions, size_t rows_cap) { return hz::fb::positions(f, positions, rows_cap, f ? f->q.B : 1); }

int hzsdr_framesync_plan(const hzsdr_framesync *f, size_t *rows_per_wave, size_t *tile_bits, size_t *ring_words, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_per_wave) *rows_per_wave = f->g.G;
    if (tile_bits) *tile_bits = hz::fp::kTileBits;
    if (ring_words) *ring_words = f->g.RW;
    if (form)
        *form = (hz::fs_complex(f) ? HZSDR_FRAMESYNC_FORM_COMPLEX : 0) | (f->q.B == 2 ? HZSDR_FRAMESYNC_FORM_DIBIT : 0) |
                (f->q.diff ? HZSDR_FRAMESYNC_FORM_DIFF : 0);
    return HZSDR_OK;
}

int hzsdr_framesync_reset(hzsdr_framesync *f) { return hz::fb::reset(f); }

int hzsdr_framesync_free(hzsdr_framesync *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->state, f->maxc});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"
