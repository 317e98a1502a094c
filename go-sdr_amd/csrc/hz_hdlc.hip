// hz_hdlc.hip -- the HDLC deframer bank (include/hzsdr_hdlc.h): hard decisions, the flags and aborts, the frames between
// two flags with their stuffed bits deleted and their FCS checked, over R rows of soft symbols with a count per row.
// The arithmetic of every bit and word is hz_hdlc_math.h (shared with the host restatement of tests/host/hdlc_ref.cpp);
// the host arithmetic (the validation, where a window and a span lie in the ring, the FCS table, the state's layout) is
// hz_hdlc_plan.h.
//
// One kernel, a bit-ring kernel: the wave, its row, the tiles, the ring in the wave's LDS and the loop over them are
// hz_bitring.h, the object around it hz_framebank.h.  Per tile:
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
//   5. the slot f is claimed behind the verdict, and lane q stores output word q.
// No inline assembly, vector stores only.
#include "hz_chain_host.h"
#include "../../include/hzsdr_hdlc.h"
#include "hz_framebank.h"
#include "hz_hdlc_math.h"
#include "hz_hdlc_plan.h"

struct hzsdr_hdlc : hz::fb::Bank {  // a row's state: bits consumed, event end, event kind, last raw decision, g.HW words of history
    static constexpr const char *noun = "hdlc";
    static constexpr uint32_t kStLast = hz::hp::kStLast, kStHist = hz::hp::kStHist;
    hz::hp::Config q;
    hz::hp::Geom g{};
    uint32_t *tab = nullptr;  // hp::kPowers powers of x^64 in the FCS register's form
};

namespace hz {

struct HdArgs : br::RowArgs {
    const uint32_t *tab;
    uint32_t OW, Lmax;
    uint32_t fcs, min_bytes, max_bytes, msb_first, keep_bad;
};

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
        const br::Row w0 = br::open_row(a, ring, row, 1, hp::kStLast, hp::kStHist, lane);
        const uint32_t m = hd_uniform(w0.m), tiles = br::tiles_of(m);
        const uint64_t bits0 = hd_uniform(w0.bits0);
        uint64_t evend = hd_uniform(w0.z[hp::kStEvEnd]);
        uint32_t evkind = hd_uniform((uint32_t)w0.z[hp::kStEvKind] & 1u);
        uint32_t carry = hd_uniform(w0.carry), f = 0;
        uint32_t cur[hp::kChunk], nxt[hp::kChunk];
        br::fetch(cur, w0.in, a.step, 0, m, lane);
#pragma unroll 1
        for (uint32_t t0 = 0; t0 < tiles; t0 += hp::kChunk) {
            if (t0 + hp::kChunk < tiles) br::fetch(nxt, w0.in, a.step, t0 + hp::kChunk, m, lane);
            br::chunk_words(a, ring, cur, t0, tiles, m, carry, lane);
#pragma unroll 1
            for (uint32_t t = t0; t < t0 + hp::kChunk && t < tiles; t++) {
                const uint32_t tn = br::tile_bits(t, m);
                // 1. the events: lane l, the window that ends at the tile's bit l
                const uint32_t x = (uint32_t)br::ring_bits(ring, hp::window_bit(t, lane, a.HW), a.RW) & 0xFFu;
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
                                w[p] = br::ring_bits(ring, start + 64ull * j, a.RW) & fm::low_mask(val[p]);
                                const uint32_t b5 = j ? (uint32_t)br::ring_bits(ring, start + 64ull * j - 5, a.RW) & 31u : 0u;
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
                                br::store_out_word(dst, q, y, nbytes - 8 * q < 8 ? nbytes - 8 * q : 8);
                            }
                        }
                        f++;
                    }
                    rw::wave_sync();  // (the next frame clears the buffer)
                }
            }
            br::rotate(cur, nxt);
        }
        if (lane == 0) {
            w0.z[hp::kStEvEnd] = evend;
            w0.z[hp::kStEvKind] = evkind;
        }
        br::close_row(a, ring, w0, row, m, bits0, carry, f, hp::kStLast, hp::kStHist, lane);
    }
}

static bool hd_complex(const hzsdr_hdlc *f) { return f->q.kind == HZSDR_FMT_C64; }

}  // namespace hz

extern "C" {

int hzsdr_hdlc_create(hzsdr_ctx *ctx, int kind, int diff, unsigned fcs, unsigned min_bytes, unsigned max_bytes, int msb_first, int keep_bad, size_t rows,
                      hzsdr_hdlc **out) {
    using namespace hz;
    HZ_TRY(fb::check_create(ctx, kind, rows, out));
    if (diff < 0 || msb_first < 0 || keep_bad < 0) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "hdlc: diff, msb_first and keep_bad are not negative");
    const hp::Config q{kind, (uint32_t)diff, fcs, min_bytes, max_bytes, (uint32_t)msb_first, (uint32_t)keep_bad};
    if (const char *why = hp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("hdlc: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_hdlc *f = new hzsdr_hdlc{};
    f->ctx = ctx, f->R = (uint32_t)rows, f->q = q, f->g = hp::geom(f->R, q.max_bytes);
    f->per = f->g.per, f->frame_bytes = q.max_bytes, f->symbol_floats = hd_complex(f) ? 2 : 1;
    auto undo = [&](int rc) {
        hzsdr_hdlc_free(f);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&f->state, fb::state_words(f) * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->tab, hp::kPowers * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->maxc, sizeof(uint32_t));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "hdlc_create", __FILE__, __LINE__));
    uint32_t tab[hp::kPowers];
    hp::fcs_powers(q.fcs, tab);
    int rc = bank_upload(ctx, f->tab, tab, sizeof tab);
    if (rc == HZSDR_OK) rc = fb::initial_state(f);  // (the event in front of the stream: an abort that ends at 0)
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_hdlc_push(hzsdr_hdlc *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap, size_t out_stride,
                    uint64_t *positions, uint32_t *info, uint32_t *counts, size_t *max_count) {
    using namespace hz;
    return fb::push(f, in, n, in_stride, in_counts, out, cap, out_stride, positions, info, counts, max_count, [&](const br::RowArgs &rows) {
        const hp::Config &q = f->q;
        const hp::Geom &g = f->g;
        HdArgs a{};
        (br::RowArgs &)a = rows;
        a.step = f->symbol_floats, a.diff = q.diff;
        a.tab = f->tab, a.OW = g.OW, a.Lmax = g.Lmax;
        a.fcs = q.fcs, a.min_bytes = q.min_bytes, a.max_bytes = q.max_bytes, a.msb_first = q.msb_first, a.keep_bad = q.keep_bad;
        return launch_fv(hdlc_rows_kernel, dim3(g.waves), dim3(hp::kLanes), g.lds_bytes, f->ctx->stream, a);
    });
}

int hzsdr_hdlc_get_state(hzsdr_hdlc *f, uint64_t *positions, uint64_t *events, uint8_t *kinds, uint8_t *history, uint8_t *last, size_t rows_cap) {
    using namespace hz;
    if (!f || !events || !kinds) return HZSDR_ERR_INVALID_ARGUMENT;
    return fb::get_state(f, positions, history, last, rows_cap, 1, [&](size_t r, const uint64_t *zr) {
        events[r] = zr[hp::kStEvEnd];
        kinds[r] = (uint8_t)(zr[hp::kStEvKind] & 1u);
    });
}

int hzsdr_hdlc_set_state(hzsdr_hdlc *f, const uint64_t *positions, const uint64_t *events, const uint8_t *kinds, const uint8_t *history,
                         const uint8_t *last, size_t rows) {
    using namespace hz;
    if (!f || !positions || !events || !kinds) return HZSDR_ERR_INVALID_ARGUMENT;
    return fb::set_state(
        f, positions, history, last, rows, 1, "a position above 2^62, an event behind the position, a kind or a last decision above 1",
        [&](size_t r) { return events[r] <= positions[r] && kinds[r] <= 1; },
        [&](size_t r, uint64_t *zr) {
            zr[hp::kStEvEnd] = events[r];
            zr[hp::kStEvKind] = kinds[r];
        });
}

int hzsdr_hdlc_positions(hzsdr_hdlc *f, uint64_t *positions, size_t rows_cap) { return hz::fb::positions(f, positions, rows_cap, 1); }

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

int hzsdr_hdlc_reset(hzsdr_hdlc *f) { return hz::fb::reset(f); }

int hzsdr_hdlc_free(hzsdr_hdlc *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->state, f->tab, f->maxc});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"

