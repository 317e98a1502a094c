// hz_ldpc.hip -- the LDPC decoder bank (include/hzsdr_ldpc.h): frames of soft floats or hard bits to data bits, the
// unsatisfied checks, the iterations run and a verdict per frame, over R rows of `cap` frame slots with a count per row.
// The arithmetic of every edge and check is hz_ldpc_math.h (shared with the host restatement of tests/host/ldpc_ref.cpp);
// the host arithmetic (the validation, the edge tables, the dealing of frames to workgroups and threads, the LDS layout)
// is hz_ldpc_plan.h.
//
// One kernel.  A workgroup decodes G frames side by side, frame g on the threads [g T, (g + 1) T), T a multiple of 64,
// and walks on from one group of slots to the next.  A frame's P (int16), q (int8) and messages (int8 per edge) stay in
// LDS from the first load to the packed store; the edge tables are in LDS too where the plan found room, else they are
// read through the cache.  Per frame:
//   1. the frame's threads quantise its received values, one coalesced read, into q and P; punctured variables get 0;
//   2. per iteration, the check pass: a thread walks a check's edges twice -- t_e = clamp(P[v] - r_e) into the message's
//      own byte, gathering the parity of the hard bits, par, m1, m2 and the first edge of m1; then r_e from its t_e --
//      and a __ballot with a popcount per wave adds the unsatisfied checks to the frame's counter; behind a barrier every
//      thread reads the counters: a frame whose count is 0 has converged and stops, the workgroup leaves when none goes on;
//   3. the variable pass: P[v] = q[v] + the messages of the variable's edges, an integer sum; a barrier; the next check
//      pass counts the new hard bits' unsatisfied checks while it prepares the next iteration's messages;
//   4. the frame's threads pack hard[0 ... D-1] a byte each and store them; the first writes info.
// Messages are written in the check pass alone and P in the variable pass alone, so ONE generation of P is enough, and
// every sum has the order of the tables: no atomics on the state.  Nothing data-dependent indexes memory: every index is
// an entry of the tables checked at create.  No inline assembly, vector stores only.
#include <string>
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_ldpc.h"
#include "hz_decodebank.h"
#include "hz_ldpc_math.h"
#include "hz_ldpc_plan.h"

struct hzsdr_ldpc : hz::db::Bank {
    static constexpr const char *noun = "ldpc";
    hz::lp::Config q;
    hz::lp::Geom g{};
    uint32_t *row_ptr = nullptr, *vptr = nullptr;
    uint16_t *col = nullptr, *vedge = nullptr;
};

namespace hz {

struct LdArgs : dbp::FrameArgs {
    const uint32_t *row_ptr, *vptr;
    const uint16_t *col, *vedge;
    uint32_t cap, slots;  // slots: R * cap
    uint32_t m, n, E, head, N, D, FB, DB, T, G;
    uint32_t off_rowptr, off_vptr, off_col, off_vedge, off_frames, frame_bytes, off_q, off_r;
    float scale;
    int level;
    uint32_t max_iters, a, beta;
};

template <bool SOFT, bool TLDS>
__global__ __launch_bounds__(lp::kMaxThreads) void ldpc_frames_kernel(LdArgs a) {
    extern __shared__ __align__(16) unsigned char ld_lds[];
    uint32_t *ucnt = (uint32_t *)ld_lds;  // the unsatisfied checks: generation (it & 1), frame g
    const uint32_t tid = threadIdx.x, g = tid / a.T, t = tid - g * a.T, threads = a.G * a.T;

    const uint32_t *row_ptr = a.row_ptr, *vptr = a.vptr;
    const uint16_t *col = a.col, *vedge = a.vedge;
    if constexpr (TLDS) {
        uint32_t *lr = (uint32_t *)(ld_lds + a.off_rowptr), *lv = (uint32_t *)(ld_lds + a.off_vptr);
        uint16_t *lc = (uint16_t *)(ld_lds + a.off_col), *le = (uint16_t *)(ld_lds + a.off_vedge);
        for (uint32_t i = tid; i <= a.m; i += threads) lr[i] = a.row_ptr[i];
        for (uint32_t i = tid; i <= a.n; i += threads) lv[i] = a.vptr[i];
        for (uint32_t i = tid; i < a.E; i += threads) lc[i] = a.col[i], le[i] = a.vedge[i];
        row_ptr = lr, vptr = lv, col = lc, vedge = le;
    }
    unsigned char *fr = ld_lds + a.off_frames + g * a.frame_bytes;
    int16_t *P = (int16_t *)fr;
    int8_t *q = (int8_t *)(fr + a.off_q), *r = (int8_t *)(fr + a.off_r);

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
        if (tid < 2 * lp::kMaxGroup) ucnt[tid] = 0;

        // 1. q and P; the messages start at 0
        if (act) {
            const uint8_t *fbits = (const uint8_t *)a.in + (size_t)row * a.in_stride + (size_t)f * a.FB;
            const float *fsoft = (const float *)a.in + (size_t)row * a.in_stride + (size_t)f * a.N;
            for (uint32_t v = t; v < a.n; v += a.T) {
                int qv = 0;
                const uint32_t i = v - a.head;  // (wraps above N when v < head)
                if (i < a.N) qv = SOFT ? lm::quantise(fsoft[i], a.scale) : lm::hard(lm::packed_bit(fbits, i), a.level);
                q[v] = (int8_t)qv, P[v] = (int16_t)qv;
            }
            for (uint32_t e = t; e < a.E; e += a.T) r[e] = 0;
        }
        __syncthreads();

        uint32_t it = 0, fin_u = 0, fin_it = 0;
        bool running = act;
#pragma unroll 1
        for (;;) {
            const uint32_t gen = (it & 1u) * lp::kMaxGroup;
            // 2. the check pass: the unsatisfied checks of P, and the messages of iteration it + 1
            if (running) {
                const bool last = it == a.max_iters;
                uint32_t cnt = 0;
#pragma unroll 1
                for (uint32_t c0 = 0; c0 < a.m; c0 += a.T) {  // (the same trips on every lane of a wave)
                    const uint32_t c = c0 + t;
                    uint32_t syn = 0;
                    if (c < a.m) {
                        const uint32_t beg = row_ptr[c], end = row_ptr[c + 1];
                        lm::Check ck = lm::check_start();
                        for (uint32_t e = beg; e < end; e++) {
                            const int p = P[col[e]];
                            const int te = lm::to_check(p, r[e]);
                            syn ^= p > 0 ? 1u : 0u;
                            lm::check_take(ck, e - beg, te);
                            r[e] = (int8_t)te;
                        }
                        if (!last) {
                            const int s1 = lm::scaled(ck.m1, a.a, a.beta), s2 = lm::scaled(ck.m2, a.a, a.beta);
                            for (uint32_t e = beg; e < end; e++) r[e] = (int8_t)lm::to_variable(ck, e - beg, r[e], s1, s2);
                        }
                    }
                    cnt += (uint32_t)__popcll(__ballot(syn != 0));
                }
                if ((tid & (lp::kLanes - 1)) == 0 && cnt) atomicAdd(&ucnt[gen + g], cnt);
            }
            __syncthreads();
            bool more = false;
            uint32_t mine = 0;
            for (uint32_t k = 0; k < a.G; k++) {
                const uint32_t uk = ucnt[gen + k];
                more |= uk != 0;
                if (k == g) mine = uk;
            }
            more = more && it < a.max_iters;
            if (running && (mine == 0 || it == a.max_iters)) running = false, fin_u = mine, fin_it = it;
            if (!more) break;  // workgroup-uniform
            if (tid < lp::kMaxGroup) ucnt[(lp::kMaxGroup - gen) + tid] = 0;  // the other generation: last read before the previous barrier
            // 3. the variable pass
            if (running) {
#pragma unroll 1
                for (uint32_t v = t; v < a.n; v += a.T) {
                    int s = q[v];
                    const uint32_t end = vptr[v + 1];
                    for (uint32_t k = vptr[v]; k < end; k++) s += r[vedge[k]];
                    P[v] = (int16_t)s;
                }
            }
            it++;
            __syncthreads();
        }

        // 4. the packed bytes and info
        if (act) {
            uint8_t *dst = a.out + (size_t)row * a.out_stride + (size_t)f * a.DB;
            for (uint32_t j = t; j < a.DB; j += a.T) {
                uint32_t byte = 0;
                for (uint32_t b = 0; b < 8; b++) {
                    const uint32_t v = 8 * j + b;
                    if (v < a.D && P[v] > 0) byte |= 0x80u >> b;
                }
                dst[j] = (uint8_t)byte;
            }
            if (t == 0) a.info[base + g] = lm::info_word(fin_u, fin_it);
        }
        __syncthreads();  // (the next group's state and counters overwrite these)
    }
}

}  // namespace hz

extern "C" {

int hzsdr_ldpc_create(hzsdr_ctx *ctx, int kind, size_t checks, size_t variables, const uint32_t *row_ptr, const uint32_t *col, size_t edges,
                      size_t head, size_t received, size_t data_bits, float scale, unsigned level, unsigned max_iters, unsigned norm,
                      unsigned offset, size_t rows, hzsdr_ldpc **out) {
    using namespace hz;
    HZ_TRY(db::check_create(ctx, kind, rows, out));
    if (!row_ptr || !col) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "ldpc: null row_ptr or col");
    lp::Config q{kind, checks, variables, edges, head, received, data_bits, scale, level, max_iters, norm, offset};
    if (const char *why = lp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("ldpc: ") + why);
    if (const char *why = lp::check_code(q, row_ptr, col)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("ldpc: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_ldpc *l = new hzsdr_ldpc{{ctx, (uint32_t)rows}, q};
    l->g = lp::geom(q);
    auto undo = [&](int rc) {
        hzsdr_ldpc_free(l);
        return rc;
    };
    lp::Tables t;
    lp::build_tables(q, row_ptr, col, t);
    const int rc = db::upload(ctx, "ldpc_create",
                              {{(void **)&l->row_ptr, t.row_ptr.data(), t.row_ptr.size() * sizeof(uint32_t)},
                               {(void **)&l->vptr, t.vptr.data(), t.vptr.size() * sizeof(uint32_t)},
                               {(void **)&l->col, t.col.data(), t.col.size() * sizeof(uint16_t)},
                               {(void **)&l->vedge, t.vedge.data(), t.vedge.size() * sizeof(uint16_t)}});
    if (rc != HZSDR_OK) return undo(rc);
    *out = l;
    return HZSDR_OK;
}

int hzsdr_ldpc_decode(hzsdr_ldpc *l, const void *in, size_t in_stride, const uint32_t *in_counts, size_t cap, uint8_t *out, size_t out_stride,
                      uint32_t *info) {
    using namespace hz;
    if (!l) return HZSDR_ERR_INVALID_ARGUMENT;
    const lp::Config &q = l->q;
    const lp::Geom &g = l->g;
    const bool bits = q.kind == lp::kBits;
    const size_t w = bits ? g.FB : g.N;
    const dbp::Call c{(uintptr_t)in, (uintptr_t)out, in_stride, w, out_stride, g.DB, cap, l->R, info != nullptr};
    return db::decode(l, dbp::dense(w, g.DB), bits ? 1 : sizeof(float), c, in_counts, info, [&](const dbp::FrameArgs &fa, uint32_t cap, uint32_t slots) {
        LdArgs a{};
        static_cast<dbp::FrameArgs &>(a) = fa;
        a.row_ptr = l->row_ptr, a.vptr = l->vptr, a.col = l->col, a.vedge = l->vedge;
        a.cap = cap, a.slots = slots;
        a.m = g.m, a.n = g.n, a.E = g.E, a.head = g.head, a.N = g.N, a.D = g.D, a.FB = g.FB, a.DB = g.DB, a.T = g.T, a.G = g.G;
        a.off_rowptr = g.off_rowptr, a.off_vptr = g.off_vptr, a.off_col = g.off_col, a.off_vedge = g.off_vedge;
        a.off_frames = g.off_frames, a.frame_bytes = g.frame_bytes, a.off_q = g.off_q, a.off_r = g.off_r;
        a.scale = q.scale, a.level = (int)q.level, a.max_iters = q.max_iters, a.a = q.a, a.beta = q.beta;
        const dim3 grid(lp::groups_for(g, slots)), block(g.G * g.T);
        const bool soft = !bits, tlds = g.form == lp::kFormTablesLds;
        hipStream_t s = l->ctx->stream;
        if (soft && tlds) return launch_fv(ldpc_frames_kernel<true, true>, grid, block, g.lds_bytes, s, a);
        if (soft) return launch_fv(ldpc_frames_kernel<true, false>, grid, block, g.lds_bytes, s, a);
        if (tlds) return launch_fv(ldpc_frames_kernel<false, true>, grid, block, g.lds_bytes, s, a);
        return launch_fv(ldpc_frames_kernel<false, false>, grid, block, g.lds_bytes, s, a);
    });
}

int hzsdr_ldpc_sizes(const hzsdr_ldpc *l, size_t *N, size_t *FB, size_t *n, size_t *m, size_t *E, size_t *DB) {
    if (!l) return HZSDR_ERR_INVALID_ARGUMENT;
    if (N) *N = l->g.N;
    if (FB) *FB = l->g.FB;
    if (n) *n = l->g.n;
    if (m) *m = l->g.m;
    if (E) *E = l->g.E;
    if (DB) *DB = l->g.DB;
    return HZSDR_OK;
}

int hzsdr_ldpc_plan(const hzsdr_ldpc *l, size_t *frames_per_group, size_t *threads_per_frame, size_t *frame_lds_bytes, int *form) {
    if (!l) return HZSDR_ERR_INVALID_ARGUMENT;
    if (frames_per_group) *frames_per_group = l->g.G;
    if (threads_per_frame) *threads_per_frame = l->g.T;
    if (frame_lds_bytes) *frame_lds_bytes = l->g.frame_bytes;
    if (form) *form = l->g.form == hz::lp::kFormTablesLds ? HZSDR_LDPC_FORM_TABLES_LDS : HZSDR_LDPC_FORM_TABLES_CACHE;
    return HZSDR_OK;
}

int hzsdr_ldpc_free(hzsdr_ldpc *l) {
    if (!l) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(l->ctx, {l->row_ptr, l->vptr, l->col, l->vedge});
    delete l;
    return HZSDR_OK;
}

}  // extern "C"
