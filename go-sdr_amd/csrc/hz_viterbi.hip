// hz_viterbi.hip -- the Viterbi decoder bank (include/hzsdr_viterbi.h): convolutionally coded frames, hard bits or soft
// floats, to data bits, a path metric and a CRC verdict per frame, over R rows of `cap` frame slots with a count per row.
// The arithmetic of every step is hz_viterbi_math.h (shared with the host restatement of tests/host/viterbi_ref.cpp); the
// host arithmetic (the validation, the index table, the dealing of frames and states to lanes, the LDS layout) is
// hz_viterbi_plan.h.
//
// One kernel.  The workgroup is one wave; lane = state.  S = 64: one frame per wave; S < 64: G = 64 / S frames side by
// side, each on a lane group of its own; S = 128, 256: SPL = 2, 4 states per lane, state s on lane s & 63 in register
// s >> 6.  A wave takes G frame slots, then those a grid further on.  Per frame:
//   1. per tile of 64 steps, each lane quantises the received values of one step (n loads through the index table, no
//      division) and writes them as ONE packed word into LDS: a step's values are uniform over a frame's lanes;
//   2. per step: the word of the step (read one step ahead), the two predecessor metrics by lane exchange (the expected
//      code bits of both incoming branches are constants of the lane, in registers), add, compare, select with the tie
//      to b = 0, and a __ballot of the decisions is the step's decision word, which lane 0 writes: into the wave's LDS,
//      or, where the plan says so, into the bank's device scratch;
//   3. the end state (state 0, or the smallest metric by a lane reduction over metric << 16 | state); the traceback is
//      sequential: the first lane of each frame walks it, over the LDS (the scratch comes back a chunk at a time),
//      gathering the decoded bits into 64-bit words, the earliest bit lowest;
//   4. the frame's lanes store the words as the frame sync bank stores payload words (whole words where aligned and
//      whole, bytes otherwise); the first lane runs the CRC over a byte table in LDS and writes info.
// uint32 metrics as the definition has them: no renormalisation.  No inline assembly, vector stores only.
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_viterbi.h"
#include "hz_decodebank.h"
#include "hz_rowwave.h"
#include "hz_viterbi_math.h"
#include "hz_viterbi_plan.h"

struct hzsdr_viterbi : hz::db::Bank {
    static constexpr const char *noun = "viterbi";
    hz::vp::Config q;
    hz::vp::Geom g{};
    uint16_t *idx = nullptr;       // T n entries
    uint32_t *crc_table = nullptr;  // 256 entries (C != 0)
    uint64_t *scratch = nullptr;    // FORM_SCRATCH: g.scratch_words
};

namespace hz {

struct VtArgs : dbp::FrameArgs {
    const uint16_t *idx;
    const uint32_t *crc_table;
    uint64_t *scratch;
    uint32_t cap, slots;  // slots: R * cap
    uint32_t K, n, S, G, gshift;  // (a frame's lanes: 1 << gshift)
    uint32_t T, D, N, FB, DB, DW, tiles, chunk;
    uint32_t off_tb, off_crc, off_dec;
    uint32_t gens[vp::kMaxRate], inv;
    int term;
    float scale;
    uint32_t C, poly, init, xorout;
};

template <int SPL, bool SOFT, bool SCRATCH>
__global__ __launch_bounds__(vp::kLanes) void viterbi_frames_kernel(VtArgs a) {
    extern __shared__ __align__(16) unsigned char vt_lds[];
    uint32_t *qs = (uint32_t *)vt_lds;                  // the tile: word g * 64 + step
    uint64_t *tb = (uint64_t *)(vt_lds + a.off_tb);     // the decoded words: g * DW + word
    uint32_t *ct = (uint32_t *)(vt_lds + a.off_crc);    // the CRC's byte table
    uint64_t *dl = (uint64_t *)(vt_lds + a.off_dec);    // the decisions: a.chunk steps of SPL words
    constexpr int H = SPL > 1 ? SPL / 2 : 1;            // the predecessor pairs a lane needs per step
    const uint32_t lane = threadIdx.x;
    const uint32_t g = lane >> a.gshift, gbase = g << a.gshift, sl = lane - gbase, gsz = 1u << a.gshift;

    // the lane's constants: the code bits its states expect on both incoming branches, and where the predecessors live
    uint32_t e0[SPL], e1[SPL];
#pragma unroll
    for (int k = 0; k < SPL; k++) {
        const uint32_t s = vp::lane_state((uint32_t)k, sl);
        e0[k] = vm::expected(vm::branch_reg(s, 0, a.K), a.gens, a.n, a.inv);
        e1[k] = vm::expected(vm::branch_reg(s, 1, a.K), a.gens, a.n, a.inv);
    }
    const uint32_t src0 = vp::pred_lane(gbase, sl, 0, a.S, SPL), src1 = vp::pred_lane(gbase, sl, 1, a.S, SPL);
    const bool upper = vp::pred_reg(0, sl, SPL) != 0;  // (SPL > 1: pair h is in the registers 2 h and 2 h + 1; this lane needs the odd one)

    if (a.C) {
        for (uint32_t i = lane; i < 256; i += vp::kLanes) ct[i] = a.crc_table[i];
    }
    uint64_t *sc = SCRATCH ? a.scratch + (size_t)blockIdx.x * a.T * SPL : nullptr;
    rw::wave_sync();

#pragma unroll 1
    for (uint32_t base = blockIdx.x * a.G; base < a.slots; base += gridDim.x * a.G) {
        const uint32_t slot = base + g;
        uint32_t r = 0, f = 0;
        bool act = false;
        if (slot < a.slots) {
            uint32_t rr, ff;  // (locals keep the instruction stream of the lines written out, move for move)
            act = dbp::slot_frame(slot, a.cap, a.in_counts, &rr, &ff);
            r = rr, f = ff;
        }
        if (__ballot(act) == 0) continue;  // wave-uniform
        const uint8_t *fbits = (const uint8_t *)a.in + (size_t)r * a.in_stride + (size_t)f * a.FB;
        const float *fsoft = (const float *)a.in + (size_t)r * a.in_stride + (size_t)f * a.N;

        uint32_t m[SPL];
#pragma unroll
        for (int k = 0; k < SPL; k++) m[k] = (k == 0 && sl == 0) ? 0u : vm::kInf;

#pragma unroll 1
        for (uint32_t tile = 0; tile < a.tiles; tile++) {
            const uint32_t t0 = tile * vp::kTileSteps, tn = a.T - t0 < vp::kTileSteps ? a.T - t0 : vp::kTileSteps;
            // 1. the tile's values: lane = step
            for (uint32_t tl = sl; tl < vp::kTileSteps; tl += gsz) {
                uint32_t qw = 0;
                const uint32_t t = t0 + tl;
                if (act && t < a.T) {
#pragma unroll
                    for (uint32_t j = 0; j < vp::kMaxRate; j++) {
                        if (j < a.n) {
                            const uint32_t ix = a.idx[t * a.n + j];
                            if (ix != vm::kPunctured) qw |= vm::pack_q(SOFT ? vm::quantise(fsoft[ix], a.scale) : vm::hard(vm::packed_bit(fbits, ix)), j);
                        }
                    }
                }
                qs[g * vp::kTileSteps + tl] = qw;
            }
            rw::wave_sync();
            // 2. the steps
            uint32_t qw = qs[g * vp::kTileSteps];
#pragma unroll 1
            for (uint32_t tl = 0; tl < tn; tl++) {
                const uint32_t qn = qs[g * vp::kTileSteps + ((tl + 1) & (vp::kTileSteps - 1))];
                uint32_t pm[H][2];
#pragma unroll
                for (int h = 0; h < H; h++) {
                    if constexpr (SPL == 1) {
                        pm[h][0] = (uint32_t)__shfl((int)m[0], (int)src0);
                        pm[h][1] = (uint32_t)__shfl((int)m[0], (int)src1);
                    } else {
                        const uint32_t l0 = (uint32_t)__shfl((int)m[2 * h], (int)src0), u0 = (uint32_t)__shfl((int)m[2 * h + 1], (int)src0);
                        const uint32_t l1 = (uint32_t)__shfl((int)m[2 * h], (int)src1), u1 = (uint32_t)__shfl((int)m[2 * h + 1], (int)src1);
                        pm[h][0] = upper ? u0 : l0;
                        pm[h][1] = upper ? u1 : l1;
                    }
                }
#pragma unroll
                for (int k = 0; k < SPL; k++) {
                    const int h = (int)vp::pair_of((uint32_t)k, SPL);
                    const uint32_t d = vm::acs(pm[h][0], vm::branch_cost(qw, e0[k]), pm[h][1], vm::branch_cost(qw, e1[k]), &m[k]);
                    const uint64_t w = __ballot(d != 0);
                    if (lane == 0) {
                        const size_t at = (size_t)(t0 + tl) * SPL + k;
                        if (SCRATCH)
                            sc[at] = w;
                        else
                            dl[at] = w;
                    }
                }
                qw = qn;
            }
            rw::wave_sync();  // (the next tile's values overwrite these)
        }

        // 3. the end state and its metric
        uint32_t es = 0, fin = 0;
        if (a.term == vp::kTail) {
            fin = (uint32_t)__shfl((int)m[0], (int)gbase);
        } else {
            unsigned long long key = ~0ull;
#pragma unroll
            for (int k = 0; k < SPL; k++) {
                const unsigned long long mine = ((unsigned long long)m[k] << 16) | vp::lane_state((uint32_t)k, sl);
                key = mine < key ? mine : key;
            }
            for (uint32_t off = gsz >> 1; off; off >>= 1) {
                const unsigned long long other = __shfl_xor(key, (int)off);
                key = other < key ? other : key;
            }
            es = (uint32_t)key & 0xffffu, fin = (uint32_t)(key >> 16);
        }
        if (SCRATCH) __threadfence();  // lane 0's decision words, before the wave's other lanes read them back
        rw::wave_sync();

        // the traceback: the frame's first lane, from the last chunk of steps to the first
        {
            uint32_t s = es;
            uint64_t acc = 0;
#pragma unroll 1
            for (int32_t c0 = (int32_t)(((a.T - 1) / a.chunk) * a.chunk); c0 >= 0; c0 -= (int32_t)a.chunk) {
                const uint32_t cn = a.T - (uint32_t)c0 < a.chunk ? a.T - (uint32_t)c0 : a.chunk;
                if (SCRATCH) {
                    for (uint32_t i = lane; i < cn * SPL; i += vp::kLanes) dl[i] = sc[(size_t)c0 * SPL + i];
                    rw::wave_sync();
                }
                if (sl == 0) {
#pragma unroll 1
                    for (int32_t t = c0 + (int32_t)cn - 1; t >= c0; t--) {
                        if ((uint32_t)t < a.D) {
                            acc |= (uint64_t)vm::input_of(s, a.K) << ((uint32_t)t & 63u);
                            if (((uint32_t)t & 63u) == 0) tb[g * a.DW + ((uint32_t)t >> 6)] = acc, acc = 0;
                        }
                        const uint32_t d = (uint32_t)(dl[vp::dec_word((uint32_t)t, (uint32_t)c0, s, SPL)] >> vp::dec_bit(gbase, s)) & 1u;
                        s = vm::predecessor(s, d, a.S);
                    }
                }
                if (SCRATCH) rw::wave_sync();  // (the next chunk overwrites this one)
            }
        }
        rw::wave_sync();

        // 4. the decoded bytes, the CRC, info
        if (act) {
            uint8_t *dst = a.out + (size_t)r * a.out_stride + (size_t)f * a.DB;
            for (uint32_t j = sl; j < a.DW; j += gsz) {
                const uint64_t y = fm::out_word(tb[g * a.DW + j]);
                const uint32_t nb = a.DB - 8 * j < 8 ? a.DB - 8 * j : 8;
                uint8_t *p = dst + 8 * (size_t)j;
                if (nb == 8 && ((uintptr_t)p & 7u) == 0) {
                    *(uint64_t *)p = y;
                } else {
                    for (uint32_t b = 0; b < nb; b++) p[b] = (uint8_t)(y >> (8 * b));
                }
            }
            if (sl == 0) {
                uint32_t ok = 0;
                if (a.C) {
                    const uint64_t *w = tb + g * a.DW;
                    const uint32_t bits = a.D - a.C, bytes = bits >> 3;
                    uint32_t reg = a.init;
                    uint64_t y = 0;
                    for (uint32_t b = 0; b < bytes; b++) {
                        if ((b & 7u) == 0) y = fm::out_word(w[b >> 3]);
                        reg = vm::crc_byte(reg, vm::stream_byte(y, b & 7u), a.C, ct);
                    }
                    for (uint32_t k = 8 * bytes; k < bits; k++) reg = vm::crc_step(reg, (uint32_t)(w[k >> 6] >> (k & 63u)) & 1u, a.C, a.poly);
                    reg ^= a.xorout;
                    uint32_t sent = 0;
                    for (uint32_t k = bits; k < a.D; k++) sent = (sent << 1) | ((uint32_t)(w[k >> 6] >> (k & 63u)) & 1u);
                    ok = reg == sent ? 1u : 0u;
                }
                a.info[slot] = fin | (ok << 31);
            }
        }
        rw::wave_sync();  // (the next slots' words overwrite the LDS)
    }
}

template <int SPL> static int vt_launch(hzsdr_viterbi *v, const VtArgs &a, dim3 grid) {
    const dim3 block(vp::kLanes);
    const size_t lds = v->g.lds_bytes;
    hipStream_t s = v->ctx->stream;
    const bool soft = v->q.kind == vp::kSoftF32, scr = v->g.form == vp::kFormScratch;
    if (soft && scr) return launch_fv(viterbi_frames_kernel<SPL, true, true>, grid, block, lds, s, a);
    if (soft) return launch_fv(viterbi_frames_kernel<SPL, true, false>, grid, block, lds, s, a);
    if (scr) return launch_fv(viterbi_frames_kernel<SPL, false, true>, grid, block, lds, s, a);
    return launch_fv(viterbi_frames_kernel<SPL, false, false>, grid, block, lds, s, a);
}

}  // namespace hz

extern "C" {

int hzsdr_viterbi_create(hzsdr_ctx *ctx, int kind, unsigned K, unsigned n, const unsigned *gens, unsigned inv, uint64_t pattern,
                         unsigned pattern_bits, int termination, size_t data_bits, float scale, unsigned crc_bits, uint32_t crc_poly,
                         uint32_t crc_init, uint32_t crc_xorout, size_t rows, hzsdr_viterbi **out) {
    using namespace hz;
    HZ_TRY(db::check_create(ctx, kind, rows, out));
    if (!gens) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "viterbi: null generators");
    vp::Config q{kind, K, n, {0, 0, 0, 0}, inv, pattern, pattern_bits, termination, data_bits, scale, crc_bits, crc_poly, crc_init, crc_xorout};
    for (unsigned j = 0; j < n && j < vp::kMaxRate; j++) q.gens[j] = gens[j];
    if (const char *why = vp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("viterbi: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_viterbi *v = new hzsdr_viterbi{{ctx, (uint32_t)rows}, q};
    v->g = vp::geom(q);
    auto undo = [&](int rc) {
        hzsdr_viterbi_free(v);
        return rc;
    };
    std::vector<uint16_t> idx;
    vp::build_index(q, v->g, idx);
    uint32_t table[256];
    for (uint32_t b = 0; q.C && b < 256; b++) table[b] = vm::crc_table_entry(b, q.C, q.poly);
    const int rc = db::upload(ctx, "viterbi_create",
                              {{(void **)&v->idx, idx.data(), idx.size() * sizeof(uint16_t)},
                               {(void **)&v->crc_table, table, q.C ? sizeof table : 0},
                               {(void **)&v->scratch, nullptr, v->g.scratch_words * sizeof(uint64_t)}});
    if (rc != HZSDR_OK) return undo(rc);
    *out = v;
    return HZSDR_OK;
}

int hzsdr_viterbi_decode(hzsdr_viterbi *v, const void *in, size_t in_stride, const uint32_t *in_counts, size_t cap, uint8_t *out,
                         size_t out_stride, uint32_t *info) {
    using namespace hz;
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    const vp::Config &q = v->q;
    const vp::Geom &g = v->g;
    const bool bits = q.kind == vp::kBits;
    const size_t w = bits ? g.FB : g.N;
    const dbp::Call c{(uintptr_t)in, (uintptr_t)out, in_stride, w, out_stride, g.DB, cap, v->R, info != nullptr};
    return db::decode(v, dbp::dense(w, g.DB), bits ? 1 : sizeof(float), c, in_counts, info, [&](const dbp::FrameArgs &fa, uint32_t cap, uint32_t slots) {
        VtArgs a{};
        static_cast<dbp::FrameArgs &>(a) = fa;
        a.idx = v->idx, a.crc_table = v->crc_table, a.scratch = v->scratch;
        a.cap = cap, a.slots = slots;
        a.K = q.K, a.n = q.n, a.S = g.S, a.G = g.G, a.gshift = (uint32_t)__builtin_ctz(g.gsz);
        a.T = g.T, a.D = (uint32_t)q.D, a.N = g.N, a.FB = g.FB, a.DB = g.DB, a.DW = g.DW, a.tiles = g.tiles, a.chunk = g.chunk;
        a.off_tb = g.off_tb, a.off_crc = g.off_crc, a.off_dec = g.off_dec;
        for (uint32_t j = 0; j < vp::kMaxRate; j++) a.gens[j] = q.gens[j];
        a.inv = q.inv, a.term = q.term, a.scale = q.scale, a.C = q.C, a.poly = q.poly, a.init = q.init, a.xorout = q.xorout;
        const dim3 grid(vp::waves_for(g, slots));
        return g.SPL == 1 ? vt_launch<1>(v, a, grid) : g.SPL == 2 ? vt_launch<2>(v, a, grid) : vt_launch<4>(v, a, grid);
    });
}

int hzsdr_viterbi_sizes(const hzsdr_viterbi *v, size_t *N, size_t *FB, size_t *T, size_t *DB) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    if (N) *N = v->g.N;
    if (FB) *FB = v->g.FB;
    if (T) *T = v->g.T;
    if (DB) *DB = v->g.DB;
    return HZSDR_OK;
}

int hzsdr_viterbi_plan(const hzsdr_viterbi *v, size_t *frames_per_wave, size_t *states_per_lane, size_t *decision_bytes, int *form) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    if (frames_per_wave) *frames_per_wave = v->g.G;
    if (states_per_lane) *states_per_lane = v->g.SPL;
    if (decision_bytes) *decision_bytes = v->g.decision_bytes;
    if (form) *form = v->g.form == hz::vp::kFormLds ? HZSDR_VITERBI_FORM_LDS : HZSDR_VITERBI_FORM_SCRATCH;
    return HZSDR_OK;
}

int hzsdr_viterbi_free(hzsdr_viterbi *v) {
    if (!v) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(v->ctx, {v->idx, v->crc_table, v->scratch});
    delete v;
    return HZSDR_OK;
}

}  // extern "C"
