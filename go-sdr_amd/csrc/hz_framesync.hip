// hz_framesync.hip -- the frame sync bank (include/hzsdr_framesync.h): hard decisions, a sync-word search under up to
// four hypotheses, a hold-off and the frames' payload bits, over R rows of soft symbols with a count per row.  The
// arithmetic of every bit is hz_framesync_math.h (shared with the host restatement of tests/host/framesync_ref.cpp);
// the host arithmetic (the validation, the history ring, the state's layout) is hz_framesync_plan.h.
//
// One kernel.  The workgroup is one wave and owns ONE row (G rows, one after the other, where the plan says so; it
// says 1: hz_framesync_plan.h has the measurement).  Nothing here is sequential along a row but the hold-off, and that
// runs over candidates: lane = float.  Time goes by in tiles of 64 floats, one coalesced 256-byte load each, kChunk tiles'
// loads in flight in registers while the chunk before them is worked on:
//   1. per tile a __ballot of the sign tests is the tile's 64 bits, the earliest lowest (with diff: xored with itself
//      shifted by one under the carried raw bit); lane 0 writes the word into the ring in the wave's own LDS;
//   2. per tile lane l tests the window of the frame that COMPLETES at the tile's bit l: two ring words (at most two
//      distinct addresses over the wave: broadcasts), a funnel shift, and per hypothesis an xor, the mask and a
//      population count, the words being wave-uniform scalars.  A ballot of the candidates is almost always zero;
//      otherwise a wave-uniform loop over its set bits in ascending order applies the hold-off, claims slot f, and the
//      64 lanes extract the frame from the ring a 64-bit word each: funnel shift, map, the bits of each byte reversed,
//      whole-word stores where the destination is aligned;
// and behind the row's last tile the ring is re-aligned into the row's state.  No inline assembly, vector stores only.
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_framesync.h"
#include "hz_framesync_math.h"
#include "hz_framesync_plan.h"
#include "hz_rowwave.h"

struct hzsdr_framesync {
    hzsdr_ctx *ctx;
    hz::fp::Config q;
    uint32_t R;
    hz::fp::Geom g{};
    uint64_t *state = nullptr;  // R rows of g.per words: bits consumed, hold, last raw decision, g.HW words of history
    uint32_t *maxc = nullptr;
};

namespace hz {

struct FsArgs {
    const uint32_t *in;  // the rows' floats as their bit patterns; row r starts r * in_stride floats in
    size_t in_stride;
    uint64_t n;  // symbols a row may hold in the push
    const uint32_t *in_counts;
    uint8_t *out;
    size_t out_stride;  // bytes
    uint64_t *positions;
    uint32_t *info, *counts;
    uint32_t cap;
    uint64_t *state;
    uint32_t *maxc;
    uint32_t R, G;
    uint32_t B, W, P, K, HW, RW, c, FB, PW, per;
    uint32_t step;  // floats from one decision's float to the next: 2 on complex rows read Re only
    uint32_t thr, H, diff;
    uint64_t holdoff, mask;       // (the mask and the words in the stream's order: earliest bit lowest)
    uint64_t words[fp::kMaxHyp];
    uint32_t maps[fp::kMaxHyp];
};

// kChunk tiles of a row from tile t0 on into registers: lane = float
__device__ __forceinline__ void fs_fetch(uint32_t (&raw)[fp::kChunk], const uint32_t *in, uint32_t step, uint32_t t0, uint32_t m, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < fp::kChunk; k++) {
        const uint64_t bit = (uint64_t)(t0 + k) * fp::kTileBits + lane;
        if (bit < m) raw[k] = in[bit * step];
    }
}

__device__ __forceinline__ uint64_t fs_ring_bits(const uint64_t *ring, uint64_t bit, uint32_t RW) {
    const uint32_t w = (uint32_t)(bit >> 6);
    return fm::funnel(ring[fp::ring_slot(w, RW)], ring[fp::ring_slot(w + 1, RW)], (uint32_t)bit & 63u);
}

template <bool B2>
__global__ __launch_bounds__(fp::kLanes) void framesync_rows_kernel(FsArgs a) {
    extern __shared__ __align__(16) unsigned char fs_lds[];
    uint64_t *ring = (uint64_t *)fs_lds;
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = fp::wave_first_row(blockIdx.x, a.G), g = fp::wave_row_count(blockIdx.x, a.G, a.R);

#pragma unroll 1
    for (uint32_t r = 0; r < g; r++) {
        const size_t row = (size_t)row0 + r;
        uint64_t cnt = a.in_counts ? a.in_counts[row] : a.n;
        if (cnt > a.n) cnt = a.n;
        const uint32_t m = (uint32_t)cnt * a.B;  // the bits this push consumes (n is below 2^31)
        const uint32_t tiles = m / fp::kTileBits + (m % fp::kTileBits ? 1u : 0u);
        uint64_t *z = a.state + row * a.per;
        const uint64_t bits0 = z[fp::kStBits];
        uint64_t hold = z[fp::kStHold];
        uint32_t carry = (uint32_t)z[fp::kStLast] & 1u;
        for (uint32_t j = lane; j < a.HW; j += fp::kLanes) ring[fp::ring_slot(j, a.RW)] = z[fp::kStHist + j];
        rw::wave_sync();

        const uint32_t *in = a.in + row * a.in_stride;
        uint32_t f = 0;
        uint32_t cur[fp::kChunk], nxt[fp::kChunk];
        fs_fetch(cur, in, a.step, 0, m, lane);
#pragma unroll 1
        for (uint32_t t0 = 0; t0 < tiles; t0 += fp::kChunk) {
            if (t0 + fp::kChunk < tiles) fs_fetch(nxt, in, a.step, t0 + fp::kChunk, m, lane);
            // 1. the chunk's words into the ring
#pragma unroll
            for (uint32_t k = 0; k < fp::kChunk; k++) {
                const uint32_t t = t0 + k;
                if (t < tiles) {
                    const uint32_t left = m - t * fp::kTileBits, tn = left < fp::kTileBits ? left : fp::kTileBits;
                    const uint64_t raw = __ballot(lane < tn && fm::decide(cur[k]) != 0);
                    const uint64_t w = fm::diff_word(raw, carry, (int)a.diff);
                    carry = (uint32_t)(raw >> (tn - 1)) & 1u;
                    if (lane == 0) ring[fp::ring_slot(fp::tile_word(t, a.HW), a.RW)] = w;
                }
            }
            rw::wave_sync();
            // 2. the search: lane l, the frame that completes at the tile's bit l
#pragma unroll 1
            for (uint32_t t = t0; t < t0 + fp::kChunk && t < tiles; t++) {
                const uint32_t left = m - t * fp::kTileBits, tn = left < fp::kTileBits ? left : fp::kTileBits;
                const uint64_t x = fs_ring_bits(ring, fp::window_bit(t, lane, a.c), a.RW);
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
                            const uint64_t p = fm::map_word(fs_ring_bits(ring, pay + 64ull * j, a.RW), (int)map, B2) & fm::low_mask(bits);
                            const uint64_t y = fm::out_word(p);
                            const uint32_t nb = a.FB - 8 * j < 8 ? a.FB - 8 * j : 8;
                            uint8_t *q = dst + 8 * (size_t)j;
                            if (nb == 8 && ((uintptr_t)q & 7u) == 0) {
                                *(uint64_t *)q = y;
                            } else {
                                for (uint32_t b = 0; b < nb; b++) q[b] = (uint8_t)(y >> (8 * b));
                            }
                        }
                    }
                    f++;
                }
            }
            rw::wave_sync();  // (the next chunk's words overwrite the oldest)
#pragma unroll
            for (uint32_t k = 0; k < fp::kChunk; k++) cur[k] = nxt[k];
        }

        // the row's state: the ring re-aligned behind the m bits of the push
        if (m) {
            for (uint32_t j = lane; j < a.HW; j += fp::kLanes) z[fp::kStHist + j] = fs_ring_bits(ring, 64ull * j + m, a.RW);
        }
        if (lane == 0) {
            z[fp::kStBits] = bits0 + m;
            z[fp::kStHold] = hold;
            z[fp::kStLast] = carry;
            a.counts[row] = f;
            if (a.maxc) atomicMax(a.maxc, f);
        }
        rw::wave_sync();  // (the next row's history overwrites the ring)
    }
}

static size_t fs_state_words(const hzsdr_framesync *f) { return (size_t)f->R * f->g.per; }
static bool fs_complex(const hzsdr_framesync *f) { return f->q.kind == HZSDR_FMT_C64; }
static size_t fs_symbol_floats(const hzsdr_framesync *f) { return fs_complex(f) ? 2 : 1; }

static int fs_initial_state(hzsdr_framesync *f) {
    std::vector<uint64_t> z(fs_state_words(f), 0);
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

static int fs_download(hzsdr_framesync *f, std::vector<uint64_t> &z) {
    z.resize(fs_state_words(f));
    HZ_TRY(enter(f->ctx));
    HZ_HIP(f->ctx, hipMemcpyAsync(z.data(), f->state, z.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, f->ctx->stream));
    HZ_HIP(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_framesync_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, unsigned word_bits, uint64_t mask, unsigned thr, unsigned hyps,
                           const uint64_t *words, const unsigned *maps, unsigned payload_bits, int diff, uint64_t holdoff, size_t rows,
                           hzsdr_framesync **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != HZSDR_SYMSYNC_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "framesync: real float32 or complex64 rows");
    if (rows == 0 || rows > fp::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: 1 ... 8192 rows");
    if (!words || !maps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: null words or maps");
    if (diff < 0) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: diff is 0, 1 or 2");
    fp::Config q{kind, bits_per_symbol, word_bits, mask, thr, hyps, {0, 0, 0, 0}, {0, 0, 0, 0}, payload_bits, (uint32_t)diff, holdoff};
    for (unsigned h = 0; h < hyps && h < fp::kMaxHyp; h++) q.words[h] = words[h], q.maps[h] = maps[h];
    if (const char *why = fp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("framesync: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_framesync *f = new hzsdr_framesync{ctx, q, (uint32_t)rows};
    f->g = fp::geom(f->R, q.W, q.P);
    auto undo = [&](int rc) {
        hzsdr_framesync_free(f);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&f->state, fs_state_words(f) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->maxc, sizeof(uint32_t));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "framesync_create", __FILE__, __LINE__));
    const int rc = fs_initial_state(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_framesync_push(hzsdr_framesync *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap,
                         size_t out_stride, uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count) {
    using namespace hz;
    if (max_count) *max_count = 0;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R, FB = f->g.FB;
    if (n && (!in || !counts)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: null input or counts");
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: in_stride is below the symbols of the push");
    if (n > fp::kMaxPush) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: the push is too long");
    if (cap > 0xffffffffull / FB) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: cap is too large");
    if (R > 1 && out_stride < cap * FB) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "framesync: out_stride is below cap frames");
    if (n && cap && (!out || !positions || !info)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: null out, positions or info");
    HZ_TRY(enter(ctx));
    if (n == 0) {  // no row consumes anything: no frame, the state as it is
        if (counts && ctx->memspace == HZSDR_MEM_HOST) memset(counts, 0, R * sizeof(uint32_t));
        if (counts && ctx->memspace != HZSDR_MEM_HOST) HZ_HIP(ctx, hipMemsetAsync(counts, 0, R * sizeof(uint32_t), ctx->stream));
        return HZSDR_OK;
    }
    Stage st(ctx);
    const void *din, *dic = nullptr;
    void *dout = out, *dpos = positions, *dinfo = info, *dcounts;
    size_t dstride, ostride = out_stride;
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, fs_symbol_floats(f) * sizeof(float), &din, &dstride));
    if (in_counts) HZ_TRY(st.in(1, in_counts, R * sizeof(uint32_t), &dic));
    if (cap) {
        // the slots behind a row's count stay as they are: a HOST context's rows go up before they come back
        const size_t width = cap * FB;
        if (R == 1 || out_stride == width) {
            HZ_TRY(st.out_preserve(2, out, R * width, &dout));
            ostride = width;
        } else {
            const void *up;
            HZ_TRY(st.in_rows(2, out, R, width, out_stride, 1, &up, &ostride));
            HZ_TRY(st.out_rows(2, out, R, width, out_stride, 1, &dout, &ostride));
        }
        HZ_TRY(st.out_preserve(3, positions, R * cap * sizeof(uint64_t), &dpos));
        HZ_TRY(st.out_preserve(4, info, R * cap * sizeof(uint32_t), &dinfo));
    }
    HZ_TRY(st.out(5, counts, R * sizeof(uint32_t), &dcounts));
    if (max_count) HZ_HIP(ctx, hipMemsetAsync(f->maxc, 0, sizeof(uint32_t), ctx->stream));
    const fp::Config &q = f->q;
    const fp::Geom &g = f->g;
    FsArgs a{};
    a.in = (const uint32_t *)din, a.in_stride = dstride * fs_symbol_floats(f), a.n = n, a.in_counts = (const uint32_t *)dic;
    a.out = (uint8_t *)dout, a.out_stride = ostride, a.positions = (uint64_t *)dpos, a.info = (uint32_t *)dinfo, a.counts = (uint32_t *)dcounts;
    a.cap = (uint32_t)cap, a.state = f->state, a.maxc = max_count ? f->maxc : nullptr;
    a.R = f->R, a.G = g.G;
    a.B = q.B, a.W = q.W, a.P = q.P, a.K = g.K, a.HW = g.HW, a.RW = g.RW, a.c = g.c, a.FB = g.FB, a.PW = g.PW, a.per = g.per;
    a.step = fs_complex(f) && q.B == 1 ? 2 : 1;
    a.thr = q.thr, a.H = q.H, a.diff = q.diff, a.holdoff = q.holdoff, a.mask = fm::reverse_bits(q.mask, q.W);
    for (uint32_t h = 0; h < q.H; h++) a.words[h] = fm::reverse_bits(q.words[h], q.W), a.maps[h] = q.maps[h];
    const dim3 grid(g.waves), block(fp::kLanes);
    if (q.B == 2)
        HZ_TRY(launch_fv(framesync_rows_kernel<true>, grid, block, g.lds_bytes, ctx->stream, a));
    else
        HZ_TRY(launch_fv(framesync_rows_kernel<false>, grid, block, g.lds_bytes, ctx->stream, a));
    HZ_HIP(ctx, hipGetLastError());
    HZ_TRY(st.finish());
    if (max_count) {
        uint32_t m = 0;
        HZ_HIP(ctx, hipMemcpyAsync(&m, f->maxc, sizeof m, hipMemcpyDeviceToHost, ctx->stream));
        HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *max_count = m;
    }
    return HZSDR_OK;
}

int hzsdr_framesync_get_state(hzsdr_framesync *f, uint64_t *positions, uint64_t *holds, uint8_t *history, uint8_t *last, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions || !holds || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "framesync: the state arrays are too small");
    std::vector<uint64_t> z;
    HZ_TRY(fs_download(f, z));
    const size_t hb = fp::history_bytes(f->g.K);
    for (size_t r = 0; r < f->R; r++) {
        const uint64_t *zr = z.data() + r * f->g.per;
        positions[r] = zr[fp::kStBits] / f->q.B;
        holds[r] = zr[fp::kStHold];
        last[r] = (uint8_t)(zr[fp::kStLast] & 1u);
        fp::history_to_bytes(zr + fp::kStHist, f->g, history + r * hb);
    }
    return HZSDR_OK;
}

int hzsdr_framesync_set_state(hzsdr_framesync *f, const uint64_t *positions, const uint64_t *holds, const uint8_t *history, const uint8_t *last,
                              size_t rows) {
    using namespace hz;
    if (!f || !positions || !holds || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows != f->R) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: the state has one entry per row");
    for (size_t r = 0; r < rows; r++)
        if (positions[r] > (~0ull >> 2) || last[r] > 1) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "framesync: a position above 2^62 or a last decision above 1");
    std::vector<uint64_t> z(fs_state_words(f), 0);
    const size_t hb = fp::history_bytes(f->g.K);
    for (size_t r = 0; r < rows; r++) {
        uint64_t *zr = z.data() + r * f->g.per;
        zr[fp::kStBits] = positions[r] * f->q.B;
        zr[fp::kStHold] = holds[r];
        zr[fp::kStLast] = last[r];
        fp::history_from_bytes(history + r * hb, f->g, zr + fp::kStHist);
    }
    HZ_TRY(enter(f->ctx));
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

int hzsdr_framesync_positions(hzsdr_framesync *f, uint64_t *positions, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "framesync: the positions array is too small");
    std::vector<uint64_t> z;
    HZ_TRY(fs_download(f, z));
    for (size_t r = 0; r < f->R; r++) positions[r] = z[r * f->g.per + fp::kStBits] / f->q.B;
    return HZSDR_OK;
}

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

int hzsdr_framesync_reset(hzsdr_framesync *f) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return fs_initial_state(f);
}

int hzsdr_framesync_free(hzsdr_framesync *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->state, f->maxc});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"
