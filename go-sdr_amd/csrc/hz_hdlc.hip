// hz_hdlc.hip -- the HDLC deframer bank (include/hzsdr_hdlc.h): hard decisions, the flags and aborts, the frames between
// two flags with their stuffed bits deleted and their FCS checked, over R rows of soft symbols with a count per row.
// The arithmetic of every bit and word is hz_hdlc_math.h (shared with the host restatement of tests/host/hdlc_ref.cpp);
// the host arithmetic (the validation, the ring, the FCS table, the state's layout) is hz_hdlc_plan.h.
//
// One kernel, the frame sync kernel's shape in its front half: the workgroup is one wave and owns ONE row, lane = float,
// a tile is 64 floats and one coalesced load, kChunk tiles' loads are in flight in registers while the chunk before them
// is worked on, a __ballot of the sign tests is the tile's word, and the words go into a ring in the wave's own LDS.
// Then, per tile:
//   1. lane l tests the window b[i-7 ... i] of the tile's bit l: two ring words, a funnel shift, two compares; one
//      ballot is the flags, one the aborts.  A wave-uniform loop over their union in ascending order carries the
//      previous event (kind and end) in scalars;
//   2. per flag-flag pair the raw span's length is tested against [8 min_bytes, Lmax] first.  Then lane j takes the
//      span's word j from the ring (up to kMaxPass words a lane), forms its stuffed mask -- the five bits in front of
//      the word read from the ring too -- and a wave-wide sum of the population counts gives u.  Unless u is a whole
//      number of bytes within the bounds, that is all;
//   3. the compaction: every lane deletes its stuffed bits from its word, an inclusive scan of the kept counts gives
//      its output bit offset, and the piece is ORed into one or two words of the frame buffer behind the ring
//      (ds_or_b64: pieces of neighbouring lanes share a word);
//   4. the FCS.  A frame of up to kWalkBytes bytes is walked byte by byte through a 256-entry table that the wave
//      builds in its LDS.  A longer one is combined: lane q runs its whole output word through the register from 0
//      (lane 0: from the initial value) and multiplies by x^(64 (whole words behind it)) from the table made at create;
//      a wave-wide xor is the register in front of the frame's last word, which then goes through it bit by bit
//      (hz_hdlc_plan.h has the measurement that sets kWalkBytes);
//   5. the slot f is claimed behind the verdict, and lane q stores output word q: whole 64-bit words where the
//      destination is aligned, the tail byte by byte;
// and behind the row's last tile the ring is re-aligned into the row's state.  No inline assembly, vector stores only.
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_hdlc.h"
#include "hz_hdlc_math.h"
#include "hz_hdlc_plan.h"
#include "hz_rowwave.h"

struct hzsdr_hdlc {
    hzsdr_ctx *ctx;
    hz::hp::Config q;
    uint32_t R;
    hz::hp::Geom g{};
    uint64_t *state = nullptr;  // R rows of g.per words: bits consumed, event end, event kind, last raw decision, g.HW words of history
    uint32_t *tab = nullptr;    // hp::kPowers powers of x^64 in the FCS register's form
    uint32_t *maxc = nullptr;
};

namespace hz {

struct HdArgs {
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
    const uint32_t *tab;
    uint32_t *maxc;
    uint32_t R, G;
    uint32_t HW, RW, OW, Lmax, per;
    uint32_t step;  // floats from one decision's float to the next: 2 on complex rows
    uint32_t diff, fcs, min_bytes, max_bytes, msb_first, keep_bad;
};

__device__ __forceinline__ void hd_fetch(uint32_t (&raw)[hp::kChunk], const uint32_t *in, uint32_t step, uint32_t t0, uint32_t m, uint32_t lane) {
#pragma unroll
    for (uint32_t k = 0; k < hp::kChunk; k++) {
        const uint64_t bit = (uint64_t)(t0 + k) * hp::kTileBits + lane;
        if (bit < m) raw[k] = in[bit * step];
    }
}

__device__ __forceinline__ uint64_t hd_ring_bits(const uint64_t *ring, uint64_t bit, uint32_t RW) {
    const uint32_t w = (uint32_t)(bit >> 6);
    return fm::funnel(ring[hp::ring_slot(w, RW)], ring[hp::ring_slot(w + 1, RW)], (uint32_t)bit & 63u);
}

// a value every lane holds alike, as scalars: the event loop's conditions stay wave-uniform for the compiler too
__device__ __forceinline__ uint32_t hd_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t hd_uniform(uint64_t v) { return ((uint64_t)hd_uniform((uint32_t)(v >> 32)) << 32) | hd_uniform((uint32_t)v); }

__device__ __forceinline__ uint32_t hd_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint32_t hd_wave_xor(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint32_t hd_wave_scan(uint32_t v, uint32_t lane) {  // inclusive
#pragma unroll
    for (uint32_t o = 1; o < hp::kLanes; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ __launch_bounds__(hp::kLanes) void hdlc_rows_kernel(HdArgs a) {
    extern __shared__ __align__(16) unsigned char hd_lds[];
    uint64_t *ring = (uint64_t *)hd_lds;
    unsigned long long *obuf = (unsigned long long *)(ring + a.RW);
    const uint32_t lane = threadIdx.x;
    const uint32_t row0 = hp::wave_first_row(blockIdx.x, a.G), g = hp::wave_row_count(blockIdx.x, a.G, a.R);
    const uint32_t poly = hm::fcs_poly(a.fcs);
    uint32_t *btab = (uint32_t *)(obuf + a.OW);  // the register behind a byte, for each of its 256 values
    if (a.fcs) {
        for (uint32_t e = lane; e < 256; e += hp::kLanes) btab[e] = hm::fcs_table_entry(e, poly);
        rw::wave_sync();
    }

#pragma unroll 1
    for (uint32_t r = 0; r < g; r++) {
        const size_t row = (size_t)row0 + r;
        uint64_t cnt = a.in_counts ? a.in_counts[row] : a.n;
        if (cnt > a.n) cnt = a.n;
        const uint32_t m = hd_uniform((uint32_t)cnt);  // the bits this push consumes (n is below 2^31)
        const uint32_t tiles = m / hp::kTileBits + (m % hp::kTileBits ? 1u : 0u);
        uint64_t *z = a.state + row * a.per;
        const uint64_t bits0 = hd_uniform(z[hp::kStBits]);
        uint64_t evend = hd_uniform(z[hp::kStEvEnd]);
        uint32_t evkind = hd_uniform((uint32_t)z[hp::kStEvKind] & 1u);
        uint32_t carry = hd_uniform((uint32_t)z[hp::kStLast] & 1u);
        for (uint32_t j = lane; j < a.HW; j += hp::kLanes) ring[hp::ring_slot(j, a.RW)] = z[hp::kStHist + j];
        rw::wave_sync();

        const uint32_t *in = a.in + row * a.in_stride;
        uint32_t f = 0;
        uint32_t cur[hp::kChunk], nxt[hp::kChunk];
        hd_fetch(cur, in, a.step, 0, m, lane);
#pragma unroll 1
        for (uint32_t t0 = 0; t0 < tiles; t0 += hp::kChunk) {
            if (t0 + hp::kChunk < tiles) hd_fetch(nxt, in, a.step, t0 + hp::kChunk, m, lane);
            // the chunk's words into the ring
#pragma unroll
            for (uint32_t k = 0; k < hp::kChunk; k++) {
                const uint32_t t = t0 + k;
                if (t < tiles) {
                    const uint32_t left = m - t * hp::kTileBits, tn = left < hp::kTileBits ? left : hp::kTileBits;
                    const uint64_t raw = __ballot(lane < tn && fm::decide(cur[k]) != 0);
                    const uint64_t w = fm::diff_word(raw, carry, (int)a.diff) & fm::low_mask(tn);
                    carry = (uint32_t)(raw >> (tn - 1)) & 1u;
                    if (lane == 0) ring[hp::ring_slot(hp::tile_word(t, a.HW), a.RW)] = w;
                }
            }
            rw::wave_sync();
#pragma unroll 1
            for (uint32_t t = t0; t < t0 + hp::kChunk && t < tiles; t++) {
                const uint32_t left = m - t * hp::kTileBits, tn = left < hp::kTileBits ? left : hp::kTileBits;
                // 1. the events: lane l, the window that ends at the tile's bit l
                const uint32_t x = (uint32_t)hd_ring_bits(ring, hp::window_bit(t, lane, a.HW), a.RW) & 0xFFu;
                const uint64_t flags = __ballot(lane < tn && hm::is_flag(x)), aborts = __ballot(lane < tn && hm::is_abort(x));
                uint64_t ev = flags | aborts;
                while (ev) {  // wave-uniform, ascending
                    const uint32_t l = (uint32_t)__builtin_ctzll(ev);
                    ev &= ev - 1;
                    const uint64_t end = bits0 + (uint64_t)t * hp::kTileBits + l + 1;
                    const uint32_t kind = (uint32_t)(flags >> l) & 1u;
                    const uint64_t d = end - evend;
                    const bool pair = kind == hp::kEvFlag && evkind == hp::kEvFlag && d > 8 && hp::span_fits(d - 8, a.min_bytes, a.Lmax);
                    const uint64_t from = evend;
                    evkind = kind, evend = end;
                    if (!pair) continue;
                    // 2. the span's words, their stuffed masks, u
                    const uint32_t L = (uint32_t)d - 8, NW = (L + 63) / 64;
                    const uint64_t start = hp::span_bit(t, l, a.HW, (uint32_t)d);
                    uint64_t w[hp::kMaxPass], sm[hp::kMaxPass];
                    uint32_t val[hp::kMaxPass], stuffed = 0;
#pragma unroll
                    for (uint32_t p = 0; p < hp::kMaxPass; p++) {
                        w[p] = 0, sm[p] = 0, val[p] = 0;
                        if (64 * p < NW) {
                            const uint32_t j = lane + 64 * p;
                            if (64 * j < L) {
                                val[p] = L - 64 * j < 64 ? L - 64 * j : 64;
                                w[p] = hd_ring_bits(ring, start + 64ull * j, a.RW) & fm::low_mask(val[p]);
                                const uint32_t b5 = j ? (uint32_t)hd_ring_bits(ring, start + 64ull * j - 5, a.RW) & 31u : 0u;
                                sm[p] = hm::stuffed_mask(w[p], b5) & fm::low_mask(val[p]);
                                stuffed += (uint32_t)__builtin_popcountll(sm[p]);
                            }
                        }
                    }
                    const uint32_t u = L - hd_uniform(hd_wave_sum(stuffed));
                    if (!hp::well_formed(u, a.min_bytes, a.max_bytes)) continue;
                    // 3. the compaction into the frame buffer
                    const uint32_t NO = (u + 63) / 64, nbytes = u / 8;
                    for (uint32_t q = lane; q < NO; q += hp::kLanes) obuf[q] = 0;
                    rw::wave_sync();
                    uint32_t base = 0;
#pragma unroll
                    for (uint32_t p = 0; p < hp::kMaxPass; p++) {
                        if (64 * p < NW) {
                            const uint32_t k = val[p] - (uint32_t)__builtin_popcountll(sm[p]);
                            const uint64_t c = hm::delete_bits(w[p], sm[p]);
                            const uint32_t incl = hd_wave_scan(k, lane);
                            const uint32_t o = base + incl - k, sh = o & 63u;
                            if (k) {
                                atomicOr(&obuf[o >> 6], (unsigned long long)(c << sh));
                                if (sh + k > 64) atomicOr(&obuf[(o >> 6) + 1], (unsigned long long)(c >> (64 - sh)));
                            }
                            base += hd_uniform((uint32_t)__shfl((int)incl, 63));
                        }
                    }
                    rw::wave_sync();
                    // 4. the FCS
                    uint32_t good = 1;
                    if (a.fcs && nbytes <= hp::kWalkBytes) {  // a short frame: every lane walks its bytes through the table
                        uint32_t c = hm::fcs_init(a.fcs);
                        for (uint32_t k = 0; k < nbytes; k++) c = hm::fcs_byte(c, (uint32_t)(obuf[k >> 3] >> (8 * (k & 7))), btab);
                        good = hd_uniform(c) == hm::fcs_good(a.fcs) ? 1u : 0u;
                    } else if (a.fcs) {
                        uint32_t acc = 0;
                        for (uint32_t q = lane; q + 1 < NO; q += hp::kLanes) {  // the whole words in front of the last
                            const uint32_t part = hm::fcs_word(q == 0 ? hm::fcs_init(a.fcs) : 0u, obuf[q], 64, poly);
                            acc ^= hm::fcs_mulmod(a.tab[NO - 2 - q], part, a.fcs, poly);
                        }
                        const uint32_t front = NO == 1 ? hm::fcs_init(a.fcs) : hd_uniform(hd_wave_xor(acc));
                        good = hd_uniform(hm::fcs_word(front, obuf[NO - 1], u - 64 * (NO - 1), poly)) == hm::fcs_good(a.fcs) ? 1u : 0u;
                    }
                    // 5. the slot, behind the verdict
                    if (a.keep_bad || good) {
                        if (f < a.cap) {
                            const size_t slot = row * a.cap + f;
                            if (lane == 0) {
                                a.positions[slot] = from;
                                a.info[slot] = nbytes | (good << 31);
                            }
                            uint8_t *dst = a.out + row * a.out_stride + (size_t)f * a.max_bytes;
                            for (uint32_t q = lane; q < NO; q += hp::kLanes) {
                                const uint64_t y = a.msb_first ? fm::out_word(obuf[q]) : (uint64_t)obuf[q];
                                const uint32_t nb = nbytes - 8 * q < 8 ? nbytes - 8 * q : 8;
                                uint8_t *p8 = dst + 8 * (size_t)q;
                                if (nb == 8 && ((uintptr_t)p8 & 7u) == 0) {
                                    *(uint64_t *)p8 = y;
                                } else {
                                    for (uint32_t b = 0; b < nb; b++) p8[b] = (uint8_t)(y >> (8 * b));
                                }
                            }
                        }
                        f++;
                    }
                    rw::wave_sync();  // (the next frame clears the buffer)
                }
            }
            rw::wave_sync();  // (the next chunk's words overwrite the oldest)
#pragma unroll
            for (uint32_t k = 0; k < hp::kChunk; k++) cur[k] = nxt[k];
        }

        // the row's state: the ring re-aligned behind the m bits of the push
        if (m) {
            for (uint32_t j = lane; j < a.HW; j += hp::kLanes) z[hp::kStHist + j] = hd_ring_bits(ring, 64ull * j + m, a.RW);
        }
        if (lane == 0) {
            z[hp::kStBits] = bits0 + m;
            z[hp::kStEvEnd] = evend;
            z[hp::kStEvKind] = evkind;
            z[hp::kStLast] = carry;
            a.counts[row] = f;
            if (a.maxc) atomicMax(a.maxc, f);
        }
        rw::wave_sync();  // (the next row's history overwrites the ring)
    }
}

static size_t hd_state_words(const hzsdr_hdlc *f) { return (size_t)f->R * f->g.per; }
static bool hd_complex(const hzsdr_hdlc *f) { return f->q.kind == HZSDR_FMT_C64; }
static size_t hd_symbol_floats(const hzsdr_hdlc *f) { return hd_complex(f) ? 2 : 1; }

static int hd_initial_state(hzsdr_hdlc *f) {
    std::vector<uint64_t> z(hd_state_words(f), 0);  // (the event in front of the stream: an abort that ends at 0)
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

static int hd_download(hzsdr_hdlc *f, std::vector<uint64_t> &z) {
    z.resize(hd_state_words(f));
    HZ_TRY(enter(f->ctx));
    HZ_HIP(f->ctx, hipMemcpyAsync(z.data(), f->state, z.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, f->ctx->stream));
    HZ_HIP(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_hdlc_create(hzsdr_ctx *ctx, int kind, int diff, unsigned fcs, unsigned min_bytes, unsigned max_bytes, int msb_first, int keep_bad, size_t rows,
                      hzsdr_hdlc **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != HZSDR_SYMSYNC_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "hdlc: real float32 or complex64 rows");
    if (rows == 0 || rows > hp::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: 1 ... 8192 rows");
    if (diff < 0 || msb_first < 0 || keep_bad < 0) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: diff, msb_first and keep_bad are not negative");
    const hp::Config q{kind, (uint32_t)diff, fcs, min_bytes, max_bytes, (uint32_t)msb_first, (uint32_t)keep_bad};
    if (const char *why = hp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("hdlc: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_hdlc *f = new hzsdr_hdlc{ctx, q, (uint32_t)rows};
    f->g = hp::geom(f->R, q.max_bytes);
    auto undo = [&](int rc) {
        hzsdr_hdlc_free(f);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&f->state, hd_state_words(f) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->tab, hp::kPowers * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->maxc, sizeof(uint32_t));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "hdlc_create", __FILE__, __LINE__));
    uint32_t tab[hp::kPowers];
    hp::fcs_powers(q.fcs, tab);
    int rc = bank_upload(ctx, f->tab, tab, sizeof tab);
    if (rc == HZSDR_OK) rc = hd_initial_state(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_hdlc_push(hzsdr_hdlc *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap, size_t out_stride,
                    uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count) {
    using namespace hz;
    if (max_count) *max_count = 0;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R, FB = f->q.max_bytes;
    if (n && (!in || !counts)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: null input or counts");
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: in_stride is below the symbols of the push");
    if (n > hp::kMaxPush) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: the push is too long");
    if (cap > 0xffffffffull / FB) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: cap is too large");
    if (R > 1 && out_stride < cap * FB) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "hdlc: out_stride is below cap frames");
    if (n && cap && (!out || !positions || !info)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: null out, positions or info");
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
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, hd_symbol_floats(f) * sizeof(float), &din, &dstride));
    if (in_counts) HZ_TRY(st.in(1, in_counts, R * sizeof(uint32_t), &dic));
    if (cap) {
        // the slots behind a row's count and every slot's tail stay as they are: a HOST context's rows go up before they come back
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
    const hp::Config &q = f->q;
    const hp::Geom &g = f->g;
    HdArgs a{};
    a.in = (const uint32_t *)din, a.in_stride = dstride * hd_symbol_floats(f), a.n = n, a.in_counts = (const uint32_t *)dic;
    a.out = (uint8_t *)dout, a.out_stride = ostride, a.positions = (uint64_t *)dpos, a.info = (uint32_t *)dinfo, a.counts = (uint32_t *)dcounts;
    a.cap = (uint32_t)cap, a.state = f->state, a.tab = f->tab, a.maxc = max_count ? f->maxc : nullptr;
    a.R = f->R, a.G = g.G;
    a.HW = g.HW, a.RW = g.RW, a.OW = g.OW, a.Lmax = g.Lmax, a.per = g.per;
    a.step = hd_complex(f) ? 2 : 1;
    a.diff = q.diff, a.fcs = q.fcs, a.min_bytes = q.min_bytes, a.max_bytes = q.max_bytes, a.msb_first = q.msb_first, a.keep_bad = q.keep_bad;
    HZ_TRY(launch_fv(hdlc_rows_kernel, dim3(g.waves), dim3(hp::kLanes), g.lds_bytes, ctx->stream, a));
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

int hzsdr_hdlc_get_state(hzsdr_hdlc *f, uint64_t *positions, uint64_t *events, uint8_t *kinds, uint8_t *history, uint8_t *last, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions || !events || !kinds || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "hdlc: the state arrays are too small");
    std::vector<uint64_t> z;
    HZ_TRY(hd_download(f, z));
    const size_t hb = hp::history_bytes(f->g.K);
    for (size_t r = 0; r < f->R; r++) {
        const uint64_t *zr = z.data() + r * f->g.per;
        positions[r] = zr[hp::kStBits];
        events[r] = zr[hp::kStEvEnd];
        kinds[r] = (uint8_t)(zr[hp::kStEvKind] & 1u);
        last[r] = (uint8_t)(zr[hp::kStLast] & 1u);
        hp::history_to_bytes(zr + hp::kStHist, f->g, history + r * hb);
    }
    return HZSDR_OK;
}

int hzsdr_hdlc_set_state(hzsdr_hdlc *f, const uint64_t *positions, const uint64_t *events, const uint8_t *kinds, const uint8_t *history,
                         const uint8_t *last, size_t rows) {
    using namespace hz;
    if (!f || !positions || !events || !kinds || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows != f->R) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: the state has one entry per row");
    for (size_t r = 0; r < rows; r++)
        if (positions[r] > (~0ull >> 2) || events[r] > positions[r] || kinds[r] > 1 || last[r] > 1)
            return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: a position above 2^62, an event behind the position, a kind or a last decision above 1");
    std::vector<uint64_t> z(hd_state_words(f), 0);
    const size_t hb = hp::history_bytes(f->g.K);
    for (size_t r = 0; r < rows; r++) {
        uint64_t *zr = z.data() + r * f->g.per;
        zr[hp::kStBits] = positions[r];
        zr[hp::kStEvEnd] = events[r];
        zr[hp::kStEvKind] = kinds[r];
        zr[hp::kStLast] = last[r];
        hp::history_from_bytes(history + r * hb, f->g, zr + hp::kStHist);
    }
    HZ_TRY(enter(f->ctx));
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

int hzsdr_hdlc_positions(hzsdr_hdlc *f, uint64_t *positions, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "hdlc: the positions array is too small");
    std::vector<uint64_t> z;
    HZ_TRY(hd_download(f, z));
    for (size_t r = 0; r < f->R; r++) positions[r] = z[r * f->g.per + hp::kStBits];
    return HZSDR_OK;
}

int hzsdr_hdlc_plan(const hzsdr_hdlc *f, size_t *rows_per_wave, size_t *tile_bits, size_t *ring_words, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_per_wave) *rows_per_wave = f->g.G;
    if (tile_bits) *tile_bits = hz::hp::kTileBits;
    if (ring_words) *ring_words = f->g.RW;
    if (form)
        *form = (hz::hd_complex(f) ? HZSDR_HDLC_FORM_COMPLEX : 0) | (f->q.diff ? HZSDR_HDLC_FORM_DIFF : 0) | (f->q.fcs == 16 ? HZSDR_HDLC_FORM_FCS16 : 0) |
                (f->q.fcs == 32 ? HZSDR_HDLC_FORM_FCS32 : 0) | (f->q.msb_first ? HZSDR_HDLC_FORM_MSB_FIRST : 0) | (f->q.keep_bad ? HZSDR_HDLC_FORM_KEEP_BAD : 0);
    return HZSDR_OK;
}

int hzsdr_hdlc_reset(hzsdr_hdlc *f) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return hd_initial_state(f);
}

int hzsdr_hdlc_free(hzsdr_hdlc *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->state, f->tab, f->maxc});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"
