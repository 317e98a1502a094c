// hz_rs.hip -- the Reed-Solomon decoder bank (include/hzsdr_rs.h): frames of I symbol-interleaved codewords over GF(2^8),
// descrambled and mapped on the way in, to corrected data bytes and a verdict per frame, over R rows of `cap` frame slots
// with a count per row.  The arithmetic of every step is hz_rs_math.h (shared with the host restatement of
// tests/host/rs_ref.cpp); the host arithmetic (the validation, the table block, the LDS layout, the index maps) is
// hz_rs_plan.h.
//
// One kernel.  A workgroup is I waves and decodes one frame at a time; wave i owns codeword i.  Per frame:
//   1. all I 64 threads load the frame's F bytes (words where the slot is word-aligned), xor the scramble sequence, map
//      them through in_map and write them into LDS; one barrier;
//   2. wave i, lane j = syndrome j: Horner's rule over the n symbols of its codeword, each a broadcast read from LDS; the
//      multiply by the lane's root is two table reads in LDS, log then exp (or, built with -DHZ_RS_PRODUCTS, eight
//      register-held products selected by the bits of the running value: 5 us sooner with one codeword alone, but less
//      than half the rate with many, measured, profiles/rs_time.txt);
//   3. a __ballot of "syndrome != 0": a clean codeword is done here;
//   4. otherwise Berlekamp-Massey with lane = coefficient: the discrepancy is the xor over the lanes of Lambda_c S_{r-c},
//      formed as eight ballots with a popcount parity each, which leaves it in scalar registers, wave-uniform; B moves
//      up a lane per iteration; the walk ends as soon as the length passes t;
//   5. the evaluator's coefficients, lane = coefficient; the Chien search with the n positions dealt over the 64 lanes
//      in up to 4 passes, a ballot counting the roots; the lanes that found a root compute Forney's value for it;
//   6. only when the roots are as many as the locator's degree are the corrections applied, in LDS; a second barrier;
//   7. the first I k bytes go out through out_map, whole words where aligned and whole, bytes otherwise: exact at byte
//      granularity, the neighbouring bytes stay; thread 0 writes info.
// Nothing depends on data for its memory safety: the length L is at most t <= 32 before it indexes anything, positions
// come from the lane number, and every table index is a sum of table values inside the table by construction.
// No inline assembly, vector stores only.
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_rs.h"
#include "hz_decodebank.h"
#include "hz_rowwave.h"
#include "hz_rs_math.h"
#include "hz_rs_plan.h"

struct hzsdr_rs : hz::db::Bank {
    static constexpr const char *noun = "rs";
    hz::rsp::Config q;
    hz::rsp::Geom g{};
    uint8_t *tables = nullptr;  // g.table_bytes
};

namespace hz {

#ifdef HZ_RS_PRODUCTS
constexpr bool kRsLogMul = false;
#else
constexpr bool kRsLogMul = true;
#endif

// (dbp::FrameArgs with a slot pitch beside each stride, laid out as it was: with the pitches moved behind `info` the
// kernel's scalar registers were renumbered, and one case of nine then timed 0.1 us above both runs of the build before)
struct RsArgs {
    const uint8_t *in;
    size_t in_stride, in_pitch;
    const uint32_t *in_counts;
    uint8_t *out;
    size_t out_stride, out_pitch;
    uint32_t *info;
    const uint8_t *tables;
    uint32_t cap, slots;
    rsm::Code code;
    uint32_t I, F, IK, t;
    uint32_t off_frame, off_wave, off_res;
};

// the xor of x (8 bits) over the wave's lanes, wave-uniform
__device__ __forceinline__ uint32_t rs_wave_xor(uint32_t x) {
    uint32_t d = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) d |= ((uint32_t)__popcll(__ballot((x >> b) & 1u)) & 1u) << b;
    return d;
}

template <bool LOGMUL>
__global__ __launch_bounds__(rsp::kMaxInterleave * rsp::kLanes) void rs_frames_kernel(RsArgs a) {
    extern __shared__ __align__(16) unsigned char rs_lds[];
    const uint8_t *exp = rs_lds + rsp::kTabExp, *log = rs_lds + rsp::kTabLog, *imap = rs_lds + rsp::kTabIn, *omap = rs_lds + rsp::kTabOut;
    uint8_t *frame = rs_lds + a.off_frame;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, nthr = blockDim.x;
    uint8_t *wl = rs_lds + a.off_wave + wave * rsp::kWaveBytes;
    uint8_t *syn = wl + rsp::kWaveSyn, *lamA = wl + rsp::kWaveLam, *omgA = wl + rsp::kWaveOmg;
    int32_t *res = (int32_t *)(rs_lds + a.off_res);
    const uint8_t *scr = a.tables + rsp::kTabBytes;
    const rsm::Code c = a.code;

    for (uint32_t i = tid; i < rsp::kTabBytes / 4; i += nthr) ((uint32_t *)rs_lds)[i] = ((const uint32_t *)a.tables)[i];
    __syncthreads();

    // the lane's constants: its root, as a log or as eight products
    const uint32_t jroot = lane < c.nroots ? lane : 0u, lroot = rsm::root_log(c, jroot);
    uint32_t P[8];
    rsm::products(exp[lroot], c.poly, P);

#pragma unroll 1
    for (uint32_t slot = blockIdx.x; slot < a.slots; slot += gridDim.x) {
        uint32_t r, f;
        if (!dbp::slot_frame(slot, a.cap, a.in_counts, &r, &f)) continue;  // uniform over the workgroup
        const uint8_t *src = a.in + (size_t)r * a.in_stride + (size_t)f * a.in_pitch;
        uint8_t *dst = a.out + (size_t)r * a.out_stride + (size_t)f * a.out_pitch;

        // 1. the frame, prepared
        uint32_t whole = 0;
        if (((uintptr_t)src & 3u) == 0) {
            whole = a.F >> 2;
            for (uint32_t w = tid; w < whole; w += nthr) {
                const uint32_t x = ((const uint32_t *)src)[w] ^ ((const uint32_t *)scr)[w];
                ((uint32_t *)frame)[w] = (uint32_t)imap[x & 0xffu] | (uint32_t)imap[(x >> 8) & 0xffu] << 8 | (uint32_t)imap[(x >> 16) & 0xffu] << 16 |
                                         (uint32_t)imap[x >> 24] << 24;
            }
        }
        for (uint32_t m = 4 * whole + tid; m < a.F; m += nthr) frame[m] = imap[src[m] ^ scr[m]];
        __syncthreads();

        // 2. the syndromes: lane = syndrome
        uint32_t s = 0;
#pragma unroll 4
        for (uint32_t p = 0; p < c.n; p++) {
            const uint32_t v = frame[rsp::frame_index(wave, p, a.I)];
            s = (LOGMUL ? rsm::mul_log(s, lroot, exp, log) : rsm::mul_products(s, P)) ^ v;
        }
        if (lane >= c.nroots) s = 0;

        // 3. clean?
        int32_t e = 0;
        if (__ballot(s != 0) != 0) {
            syn[lane] = (uint8_t)s;
            rw::wave_sync();
            // 4. Berlekamp-Massey: lane = coefficient
            uint32_t lam = lane == 0 ? 1u : 0u, B = lam, L = 0;
#pragma unroll 1
            for (uint32_t it = 0; it < c.nroots; it++) {
                const uint32_t sv = lane <= it ? syn[rsp::bm_syndrome(it, lane)] : 0u;
                const uint32_t d = rs_wave_xor(rsm::bm_term(lam, sv, c.poly));
                uint32_t bs = (uint32_t)__shfl_up((int)B, 1);
                if (lane == 0) bs = 0;
                if (d) {
                    const uint32_t nl = rsm::bm_lambda(lam, d, bs, c.poly);
                    if (2 * L <= it) {
                        B = rsm::bm_b(lam, rsm::inv(d, exp, log), c.poly);
                        L = it + 1 - L;
                    } else {
                        B = bs;
                    }
                    lam = nl;
                } else {
                    B = bs;
                }
                if (L > a.t) break;
            }
            if (L > a.t || L == 0) {
                e = rsm::kFailed;
            } else {
                // 5. the evaluator, the roots and their values (L <= t <= 32 from here on)
                lamA[lane] = (uint8_t)lam;
                rw::wave_sync();
                omgA[lane] = lane < L ? (uint8_t)rsm::omega_coeff(lamA, syn, lane, c.poly) : (uint8_t)0;
                rw::wave_sync();
                uint32_t roots = 0, ev[rsp::kPasses], hits = 0;
#pragma unroll
                for (uint32_t q = 0; q < rsp::kPasses; q++) {
                    const uint32_t p = rsp::chien_position(q, lane);
                    const bool valid = p < c.n;
                    const uint32_t xl = valid ? rsm::locator_log(c, p) : 0u;
                    const bool hit = valid && rsm::poly_eval(lamA, L, exp[rsm::neg_log(xl)], c.poly) == 0;
                    roots += (uint32_t)__popcll(__ballot(hit));
                    ev[q] = hit ? rsm::forney(lamA, omgA, L, xl, c, exp, log) : 0u;
                    hits |= (hit ? 1u : 0u) << q;
                }
                // 6. as many roots as the degree, or nothing is changed
                if (roots == L) {
#pragma unroll
                    for (uint32_t q = 0; q < rsp::kPasses; q++)
                        if ((hits >> q) & 1u) frame[rsp::frame_index(wave, rsp::chien_position(q, lane), a.I)] ^= (uint8_t)ev[q];
                    e = (int32_t)L;
                } else {
                    e = rsm::kFailed;
                }
            }
        }
        if (lane == 0) res[wave] = e;
        __syncthreads();

        // 7. the data bytes and info
        whole = 0;
        if (((uintptr_t)dst & 3u) == 0) {
            whole = a.IK >> 2;
            for (uint32_t w = tid; w < whole; w += nthr) {
                const uint32_t x = ((const uint32_t *)frame)[w];
                ((uint32_t *)dst)[w] = (uint32_t)omap[x & 0xffu] | (uint32_t)omap[(x >> 8) & 0xffu] << 8 | (uint32_t)omap[(x >> 16) & 0xffu] << 16 |
                                       (uint32_t)omap[x >> 24] << 24;
            }
        }
        for (uint32_t m = 4 * whole + tid; m < a.IK; m += nthr) dst[m] = omap[frame[m]];
        if (tid == 0) {
            uint32_t E = 0, nfail = 0;
            for (uint32_t i = 0; i < a.I; i++) {
                if (res[i] < 0)
                    nfail++;
                else
                    E += (uint32_t)res[i];
            }
            a.info[slot] = E | nfail << 16 | (nfail == 0 ? 1u << 31 : 0u);
        }
        __syncthreads();  // (the next slot's frame overwrites the LDS)
    }
}

}  // namespace hz

extern "C" {

int hzsdr_rs_create(hzsdr_ctx *ctx, unsigned gfpoly, unsigned fcr, unsigned prim, unsigned nroots, unsigned n, unsigned interleave,
                    const uint8_t *in_map, const uint8_t *out_map, const uint8_t *scramble, size_t scramble_len, size_t rows, hzsdr_rs **out) {
    using namespace hz;
    HZ_TRY(db::check_create(ctx, dbp::kBits, rows, out));  // (bytes: no kind to refuse)
    if (scramble_len > rsp::kMaxScramble || (scramble_len && !scramble)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "rs: a scramble sequence of 0 ... 2040 bytes");
    const rsp::Config q{gfpoly, fcr, prim, nroots, n, interleave, (uint32_t)scramble_len};
    if (const char *why = rsp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("rs: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_rs *v = new hzsdr_rs{{ctx, (uint32_t)rows}, q};
    v->g = rsp::geom(q);
    auto undo = [&](int rc) {
        hzsdr_rs_free(v);
        return rc;
    };
    std::vector<uint8_t> block;
    if (!rsp::build_block(q, v->g, in_map, out_map, scramble, block)) return undo(fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "rs: gfpoly is not primitive"));
    const int rc = db::upload(ctx, "rs_create", {{(void **)&v->tables, block.data(), block.size()}});
    if (rc != HZSDR_OK) return undo(rc);
    *out = v;
    return HZSDR_OK;
}

int hzsdr_rs_decode(hzsdr_rs *v, const uint8_t *in, size_t in_stride, size_t in_pitch, const uint32_t *in_counts, size_t cap, uint8_t *out,
                    size_t out_stride, size_t out_pitch, uint32_t *info) {
    using namespace hz;
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    const rsp::Geom &g = v->g;
    const dbp::Call c{(uintptr_t)in, (uintptr_t)out, in_stride, in_pitch, out_stride, out_pitch, cap, v->R, info != nullptr};
    return db::decode(v, rsp::slots(g), 1, c, in_counts, info, [&](const dbp::FrameArgs &fa, uint32_t cap, uint32_t slots) {
        RsArgs a{};
        a.in = (const uint8_t *)fa.in, a.in_stride = fa.in_stride, a.in_pitch = in_pitch, a.in_counts = fa.in_counts;
        a.out = fa.out, a.out_stride = fa.out_stride, a.out_pitch = out_pitch, a.info = fa.info, a.tables = v->tables;
        a.cap = cap, a.slots = slots;
        a.code = rsm::Code{v->q.gfpoly, v->q.fcr, v->q.prim, v->q.nroots, v->q.n};
        a.I = v->q.interleave, a.F = g.F, a.IK = g.IK, a.t = g.t;
        a.off_frame = g.off_frame, a.off_wave = g.off_wave, a.off_res = g.off_res;
        return launch_fv(rs_frames_kernel<kRsLogMul>, dim3(rsp::groups_for(slots)), dim3(g.threads), g.lds_bytes, v->ctx->stream, a);
    });
}

int hzsdr_rs_sizes(const hzsdr_rs *v, size_t *k, size_t *t, size_t *frame_bytes, size_t *data_bytes) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    if (k) *k = v->g.k;
    if (t) *t = v->g.t;
    if (frame_bytes) *frame_bytes = v->g.F;
    if (data_bytes) *data_bytes = v->g.IK;
    return HZSDR_OK;
}

int hzsdr_rs_plan(const hzsdr_rs *v, size_t *waves_per_group, size_t *lds_bytes, size_t *groups_per_cu, size_t *max_groups) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    if (waves_per_group) *waves_per_group = v->g.waves;
    if (lds_bytes) *lds_bytes = v->g.lds_bytes;
    if (groups_per_cu) *groups_per_cu = v->g.groups_per_cu;
    if (max_groups) *max_groups = hz::rsp::kMaxGroups;
    return HZSDR_OK;
}

int hzsdr_rs_free(hzsdr_rs *v) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(v->ctx, {v->tables});
    delete v;
    return HZSDR_OK;
}

}  // extern "C"
