// hz_softframe.hip -- the soft frame bank (include/hzsdr_softframe.h): the payload floats of the frames a frame sync
// bank found, through each frame's hypothesis map, over R rows of soft symbols with a count per row.  Every index is
// hz_softframe_plan.h (shared with the host restatement of tests/host/softframe_ref.cpp): the window test, the line
// history ++ input, the maps on bit patterns.
//
// Two stream-ordered kernels per push.
//   1. The gather: one workgroup per (row, frame slot); those whose slot is at or behind min(counts[r], cap) leave at
//      once (the counts are on the device: the grid is rows * cap).  The window test decides, wave-uniformly, between
//      the quiet-NaN fill and the copy; the copy moves the frame's P floats kThreads at a time, lane = float, loads
//      and stores coalesced, each float from the history or from the push's input as its line index says, the map
//      applied in registers.  At B = 2 a lane moves one 8-byte pair (a pair never straddles history and input);
//      where a pointer or a pitch is not 8-byte aligned the float-by-float form runs instead: the same bits.
//   2. The carry: the new history is the line from float c * B on, written into the bank's SECOND history buffer (a
//      push with c < Kh takes floats from the old history that it would otherwise have overwritten); the two buffers
//      change places on the host.  Its workgroup 0 of a row advances the row's position.
// No inline assembly, vector stores only.
#include <vector>

#include "hz_chain_host.h"
#include "../../include/hzsdr_softframe.h"
#include "hz_softframe_plan.h"

struct hzsdr_softframe {
    hzsdr_ctx *ctx;
    hz::sfp::Config q;
    uint32_t R;
    hz::sfp::Geom g{};
    uint64_t *pos = nullptr;               // R positions, in symbols
    uint32_t *hist[2] = {nullptr, nullptr};  // R rows of g.HF floats each; hist[cur] is the state
    int cur = 0;
};

namespace hz {

struct SfArgs {
    const uint32_t *in;  // the rows' floats as their bit patterns; row r starts r * in_stride floats in
    size_t in_stride;
    uint64_t n;
    const uint32_t *in_counts;
    const uint64_t *positions;
    const uint32_t *info, *counts;
    uint32_t cap;
    uint32_t *out;
    size_t out_stride;  // floats
    uint32_t *status;
    uint64_t *pos;
    const uint32_t *hist;
    uint32_t *hist_next;
    uint32_t B, P, H, Kh, HF, in_step;
    uint32_t maps[sfp::kMaxHyp];
};

template <bool PAIR>
__global__ __launch_bounds__(sfp::kThreads) void softframe_gather_kernel(SfArgs a) {
    const uint32_t slot = blockIdx.x, tid = threadIdx.x;
    const uint32_t row = slot / a.cap, f = slot - row * a.cap;
    uint32_t cnt = a.counts[row];
    if (cnt > a.cap) cnt = a.cap;
    if (f >= cnt) return;
    const uint64_t s = a.positions[slot];
    const uint32_t h = (a.info[slot] >> 8) & 0xffu;
    const uint64_t c = sfp::consumed(a.in_counts ? a.in_counts[row] : a.n, a.n);
    const uint64_t p0 = a.pos[row];
    const uint32_t st = sfp::window_status(s, h, a.H, p0, p0 + c, a.Kh);
    uint32_t *dst = a.out + (size_t)row * a.out_stride + (size_t)f * a.P;
    if (tid == 0) a.status[slot] = st;
    if (st != sfp::kServed) {
        for (uint32_t k = tid; k < a.P; k += sfp::kThreads) dst[k] = sfp::kQuietNaN;
        return;
    }
    const uint32_t map = h == 0 ? a.maps[0] : (h == 1 ? a.maps[1] : (h == 2 ? a.maps[2] : a.maps[3]));
    const uint64_t v0 = sfp::line_start(s, p0, a.Kh, a.B);
    const uint32_t *hist = a.hist + (size_t)row * a.HF;
    const uint32_t *in = a.in + (size_t)row * a.in_stride;
    if (PAIR) {
        for (uint32_t k = 2 * tid; k < a.P; k += 2 * sfp::kThreads) {
            const uint64_t v = v0 + k;
            uint2 x = sfp::in_history(v, a.HF) ? *(const uint2 *)(hist + v) : *(const uint2 *)(in + sfp::input_float(v, a.HF, 1));
            sfp::map_pair(x.x, x.y, map);
            *(uint2 *)(dst + k) = x;
        }
    } else {
        for (uint32_t k = tid; k < a.P; k += sfp::kThreads) {
            const uint64_t v = v0 + sfp::map_source(k, map, a.B);
            const uint32_t x = sfp::in_history(v, a.HF) ? hist[v] : in[sfp::input_float(v, a.HF, a.in_step)];
            dst[k] = x ^ sfp::map_flip(k, map, a.B);
        }
    }
}

__global__ __launch_bounds__(sfp::kThreads) void softframe_carry_kernel(SfArgs a) {
    const uint32_t row = blockIdx.y, j = blockIdx.x * sfp::kThreads + threadIdx.x;
    const uint64_t c = sfp::consumed(a.in_counts ? a.in_counts[row] : a.n, a.n);
    if (j < a.HF) {
        const uint64_t v = sfp::carried_float(c, a.B, j);
        const uint32_t *in = a.in + (size_t)row * a.in_stride;
        a.hist_next[(size_t)row * a.HF + j] = sfp::in_history(v, a.HF) ? a.hist[(size_t)row * a.HF + v] : in[sfp::input_float(v, a.HF, a.in_step)];
    }
    if (j == 0) a.pos[row] += c;
}

static size_t sf_hist_bytes(const hzsdr_softframe *f) { return ((size_t)f->R * f->g.HF + 1) * sizeof(uint32_t); }

static int sf_initial_state(hzsdr_softframe *f) {
    HZ_HIP(f->ctx, hipMemsetAsync(f->pos, 0, f->R * sizeof(uint64_t), f->ctx->stream));
    HZ_HIP(f->ctx, hipMemsetAsync(f->hist[f->cur], 0, sf_hist_bytes(f), f->ctx->stream));
    HZ_HIP(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return HZSDR_OK;
}

static int sf_download(hzsdr_softframe *f, uint64_t *positions, float *history) {
    HZ_TRY(enter(f->ctx));
    HZ_HIP(f->ctx, hipMemcpyAsync(positions, f->pos, f->R * sizeof(uint64_t), hipMemcpyDeviceToHost, f->ctx->stream));
    if (history && f->g.HF)
        HZ_HIP(f->ctx, hipMemcpyAsync(history, f->hist[f->cur], (size_t)f->R * f->g.HF * sizeof(float), hipMemcpyDeviceToHost, f->ctx->stream));
    HZ_HIP(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return HZSDR_OK;
}

}  // namespace hz

extern "C" {

int hzsdr_softframe_create(hzsdr_ctx *ctx, int kind, unsigned bits_per_symbol, unsigned payload_bits, unsigned hyps, const unsigned *maps,
                           size_t rows, hzsdr_softframe **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != HZSDR_SYMSYNC_REAL_F32 && kind != HZSDR_FMT_C64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "softframe: real float32 or complex64 rows");
    if (rows == 0 || rows > sfp::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "softframe: 1 ... 8192 rows");
    if (!maps) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "softframe: null maps");
    sfp::Config q{kind, bits_per_symbol, payload_bits, hyps, {0, 0, 0, 0}};
    for (unsigned h = 0; h < hyps && h < sfp::kMaxHyp; h++) q.maps[h] = maps[h];
    if (const char *why = sfp::check_config(q)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string("softframe: ") + why);
    HZ_TRY(enter(ctx));
    hzsdr_softframe *f = new hzsdr_softframe{ctx, q, (uint32_t)rows};
    f->g = sfp::geom(q);
    auto undo = [&](int rc) {
        hzsdr_softframe_free(f);
        return rc;
    };
    hipError_t e = hipMalloc((void **)&f->pos, rows * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc((void **)&f->hist[0], sf_hist_bytes(f));
    if (e == hipSuccess) e = hipMalloc((void **)&f->hist[1], sf_hist_bytes(f));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, "softframe_create", __FILE__, __LINE__));
    const int rc = sf_initial_state(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

int hzsdr_softframe_push(hzsdr_softframe *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, const uint64_t *positions,
                         const uint32_t *info, const uint32_t *counts, size_t cap, float *out, size_t out_stride, uint32_t *status) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R, P = f->q.P;
    const sfp::Geom &g = f->g;
    const char *why = nullptr;
    const int bad = sfp::check_call(f->q, {n, in_stride, cap, out_stride, R, in != nullptr, positions != nullptr, info != nullptr, counts != nullptr,
                                           out != nullptr, status != nullptr}, &why);
    if (bad) return fail(ctx, bad == sfp::kDstTooSmall ? HZSDR_ERR_DST_TOO_SMALL : HZSDR_ERR_INVALID_ARGUMENT, std::string("softframe: ") + why);
    HZ_TRY(enter(ctx));
    if (n == 0 && cap == 0) return HZSDR_OK;
    Stage st(ctx);
    const void *din = nullptr, *dic = nullptr, *dpos = nullptr, *dinfo = nullptr, *dcounts = nullptr;
    void *dout = out, *dstatus = status;
    size_t dstride = in_stride, ostride = out_stride;
    if (n) HZ_TRY(st.in_rows(0, in, R, n, in_stride, g.sym_floats * sizeof(float), &din, &dstride));
    if (in_counts) HZ_TRY(st.in(1, in_counts, R * sizeof(uint32_t), &dic));
    if (cap) {
        HZ_TRY(st.in(2, positions, R * cap * sizeof(uint64_t), &dpos));
        HZ_TRY(st.in(3, info, R * cap * sizeof(uint32_t), &dinfo));
        HZ_TRY(st.in(4, counts, R * sizeof(uint32_t), &dcounts));
        // the slots behind a row's count stay as they are
        HZ_TRY(stage_out_rows_preserved(st, 5, out, R, cap * P, out_stride, sizeof(float), &dout, &ostride));
        HZ_TRY(st.out_preserve(6, status, R * cap * sizeof(uint32_t), &dstatus));
    }
    SfArgs a{};
    a.in = (const uint32_t *)din, a.in_stride = dstride * g.sym_floats, a.n = n, a.in_counts = (const uint32_t *)dic;
    a.positions = (const uint64_t *)dpos, a.info = (const uint32_t *)dinfo, a.counts = (const uint32_t *)dcounts, a.cap = (uint32_t)cap;
    a.out = (uint32_t *)dout, a.out_stride = ostride, a.status = (uint32_t *)dstatus;
    a.pos = f->pos, a.hist = f->hist[f->cur], a.hist_next = f->hist[f->cur ^ 1];
    a.B = f->q.B, a.P = f->q.P, a.H = f->q.H, a.Kh = g.Kh, a.HF = g.HF, a.in_step = g.in_step;
    for (uint32_t h = 0; h < sfp::kMaxHyp; h++) a.maps[h] = f->q.maps[h];
    if (cap) {
        const bool pair = f->q.B == 2 && ((uintptr_t)a.in & 7u) == 0 && ((uintptr_t)a.out & 7u) == 0 && (R == 1 || ostride % 2 == 0);
        const dim3 grid((unsigned)(R * cap)), block(sfp::kThreads);
        if (pair)
            HZ_TRY(launch_fv(softframe_gather_kernel<true>, grid, block, 0, ctx->stream, a));
        else
            HZ_TRY(launch_fv(softframe_gather_kernel<false>, grid, block, 0, ctx->stream, a));
        HZ_HIP(ctx, hipGetLastError());
    }
    if (n) {
        const dim3 grid(g.HF ? (g.HF + sfp::kThreads - 1) / sfp::kThreads : 1u, (unsigned)R), block(sfp::kThreads);
        HZ_TRY(launch_fv(softframe_carry_kernel, grid, block, 0, ctx->stream, a));
        HZ_HIP(ctx, hipGetLastError());
        f->cur ^= 1;
    }
    return st.finish();
}

int hzsdr_softframe_get_state(hzsdr_softframe *f, uint64_t *positions, float *history, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions || (!history && f->g.HF)) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "softframe: the state arrays are too small");
    return sf_download(f, positions, history);
}

int hzsdr_softframe_set_state(hzsdr_softframe *f, const uint64_t *positions, const float *history, size_t rows) {
    using namespace hz;
    if (!f || !positions || (!history && f->g.HF)) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows != f->R) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "softframe: the state has one entry per row");
    for (size_t r = 0; r < rows; r++)
        if (positions[r] > sfp::kMaxPosition) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, "softframe: a position above 2^62");
    HZ_TRY(enter(f->ctx));
    HZ_TRY(bank_upload(f->ctx, f->pos, positions, rows * sizeof(uint64_t)));
    if (f->g.HF) HZ_TRY(bank_upload(f->ctx, f->hist[f->cur], history, rows * f->g.HF * sizeof(float)));
    return HZSDR_OK;
}

int hzsdr_softframe_positions(hzsdr_softframe *f, uint64_t *positions, size_t rows_cap) {
    using namespace hz;
    if (!f || !positions) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, "softframe: the positions array is too small");
    return sf_download(f, positions, nullptr);
}

int hzsdr_softframe_plan(const hzsdr_softframe *f, size_t *step_floats, size_t *history_floats, int *form) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    if (step_floats) *step_floats = f->g.step;
    if (history_floats) *history_floats = f->g.HF;
    if (form) *form = hz::sfp::form(f->q);
    return HZSDR_OK;
}

int hzsdr_softframe_reset(hzsdr_softframe *f) {
    using namespace hz;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return sf_initial_state(f);
}

int hzsdr_softframe_free(hzsdr_softframe *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(f->ctx, {f->pos, f->hist[0], f->hist[1]});
    delete f;
    return HZSDR_OK;
}

}  // extern "C"
