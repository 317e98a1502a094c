// hz_framebank.h -- the host side of the bit-ring banks (hz_framesync.hip, hz_hdlc.hip): what their objects hold alike
// and the calls over it, around the kernels that hz_bitring.h describes.  A bank's object derives from Bank and adds its
// configuration `q`, its geometry `g` (a br::Ring and a br::Deal among it) and, as statics, the noun that starts its
// messages and where a row's state keeps the last raw decision and the history (kStLast, kStHist; the bits consumed are
// word 0 and the bank's own words lie between).  Nothing here knows which bank it serves.
#pragma once
#include <vector>

#include "hz_bitring.h"
#include "hz_common.h"

namespace hz {
// (hidden: the instantiations below add nothing to the library's dynamic symbols)
namespace fb __attribute__((visibility("hidden"))) {

struct Bank {
    hzsdr_ctx *ctx = nullptr;
    uint32_t R = 0;
    uint32_t per = 0;            // a row's state, in uint64 words
    uint32_t frame_bytes = 0;    // a slot of `out`
    uint32_t symbol_floats = 1;  // 2 on complex rows
    uint64_t *state = nullptr;   // R rows of `per` words on the device
    uint32_t *maxc = nullptr;
};

template <class F> std::string who(const char *msg) { return std::string(F::noun) + ": " + msg; }

// the checks in front of a create
template <class F> int check_create(hzsdr_ctx *ctx, int kind, size_t rows, F **out) {
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != br::kRealF32 && kind != br::kC64) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, who<F>("real float32 or complex64 rows"));
    if (rows == 0 || rows > br::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("1 ... 8192 rows"));
    return HZSDR_OK;
}

inline size_t state_words(const Bank *f) { return (size_t)f->R * f->per; }

// every word zero: nothing consumed, a history of zeros, and what the bank's own words mean by 0
inline int initial_state(Bank *f) {
    std::vector<uint64_t> z(state_words(f), 0);
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

inline int download(Bank *f, std::vector<uint64_t> &z) {
    z.resize(state_words(f));
    HZ_TRY(enter(f->ctx));
    HZ_HIP(f->ctx, hipMemcpyAsync(z.data(), f->state, z.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, f->ctx->stream));
    HZ_HIP(f->ctx, hipStreamSynchronize(f->ctx->stream));
    return HZSDR_OK;
}

// B: bits per symbol
template <class F> int positions(F *f, uint64_t *positions, size_t rows_cap, uint32_t B) {
    if (!f || !positions) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, who<F>("the positions array is too small"));
    std::vector<uint64_t> z;
    HZ_TRY(download(f, z));
    for (size_t r = 0; r < f->R; r++) positions[r] = z[r * f->per] / B;
    return HZSDR_OK;
}

template <class F> int reset(F *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return initial_state(f);
}

// own(r, zr): the bank's own words of row r, out of the row's state zr (its arrays are not null)
template <class F, class Own> int get_state(F *f, uint64_t *positions, uint8_t *history, uint8_t *last, size_t rows_cap, uint32_t B, Own own) {
    if (!f || !positions || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows_cap < f->R) return fail(f->ctx, HZSDR_ERR_DST_TOO_SMALL, who<F>("the state arrays are too small"));
    std::vector<uint64_t> z;
    HZ_TRY(download(f, z));
    const size_t hb = br::history_bytes(f->g.K);
    for (size_t r = 0; r < f->R; r++) {
        const uint64_t *zr = z.data() + r * f->per;
        positions[r] = zr[0] / B;
        last[r] = (uint8_t)(zr[F::kStLast] & 1u);
        own(r, zr);
        br::history_to_bytes(zr + F::kStHist, f->g, history + r * hb);
    }
    return HZSDR_OK;
}

// valid(r): row r of the caller's state can be one; refusal: what cannot, behind the noun; own(r, zr): the bank's own
// words of row r into the row's state zr
template <class F, class Valid, class Own>
int set_state(F *f, const uint64_t *positions, const uint8_t *history, const uint8_t *last, size_t rows, uint32_t B, const char *refusal, Valid valid,
              Own own) {
    if (!f || !positions || !history || !last) return HZSDR_ERR_INVALID_ARGUMENT;
    if (rows != f->R) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("the state has one entry per row"));
    for (size_t r = 0; r < rows; r++)
        if (positions[r] > (~0ull >> 2) || last[r] > 1 || !valid(r)) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>(refusal));
    std::vector<uint64_t> z(state_words(f), 0);
    const size_t hb = br::history_bytes(f->g.K);
    for (size_t r = 0; r < rows; r++) {
        uint64_t *zr = z.data() + r * f->per;
        zr[0] = positions[r] * B;
        zr[F::kStLast] = last[r];
        own(r, zr);
        br::history_from_bytes(history + r * hb, f->g, zr + F::kStHist);
    }
    HZ_TRY(enter(f->ctx));
    return bank_upload(f->ctx, f->state, z.data(), z.size() * sizeof(uint64_t));
}

// A push: the checks in their order, the push of no symbols, the rows staged, launch(RowArgs) -> status with the
// pointers, the strides, n, cap, state, maxc and R of the arguments' leading part filled in, the rows brought back, the
// largest count read.
template <class F, class Launch>
int push(F *f, const void *in, size_t n, size_t in_stride, const uint32_t *in_counts, uint8_t *out, size_t cap, size_t out_stride, uint64_t *positions,
         uint32_t *info, uint32_t *counts, size_t *max_count, Launch launch) {
    if (max_count) *max_count = 0;
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R, FB = f->frame_bytes;
    if (n && (!in || !counts)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("null input or counts"));
    if (R > 1 && in_stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("in_stride is below the symbols of the push"));
    if (n > br::kMaxPush) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("the push is too long"));
    if (cap > 0xffffffffull / FB) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("cap is too large"));
    if (R > 1 && out_stride < cap * FB) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, who<F>("out_stride is below cap frames"));
    if (n && cap && (!out || !positions || !info)) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("null out, positions or info"));
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
    HZ_TRY(st.in_rows(0, in, R, n, in_stride, f->symbol_floats * sizeof(float), &din, &dstride));
    if (in_counts) HZ_TRY(st.in(1, in_counts, R * sizeof(uint32_t), &dic));
    if (cap) {
        // the slots behind a row's count, and what of a slot the frame does not fill, stay as they are
        HZ_TRY(stage_out_rows_preserved(st, 2, out, R, cap * FB, out_stride, 1, &dout, &ostride));
        HZ_TRY(st.out_preserve(3, positions, R * cap * sizeof(uint64_t), &dpos));
        HZ_TRY(st.out_preserve(4, info, R * cap * sizeof(uint32_t), &dinfo));
    }
    HZ_TRY(st.out(5, counts, R * sizeof(uint32_t), &dcounts));
    if (max_count) HZ_HIP(ctx, hipMemsetAsync(f->maxc, 0, sizeof(uint32_t), ctx->stream));
    br::RowArgs a{};
    a.in = (const uint32_t *)din, a.in_stride = dstride * f->symbol_floats, a.n = n, a.in_counts = (const uint32_t *)dic;
    a.out = (uint8_t *)dout, a.out_stride = ostride, a.positions = (uint64_t *)dpos, a.info = (uint32_t *)dinfo, a.counts = (uint32_t *)dcounts;
    a.cap = (uint32_t)cap, a.state = f->state, a.maxc = max_count ? f->maxc : nullptr;
    a.R = f->R, a.G = f->g.G, a.HW = f->g.HW, a.RW = f->g.RW, a.per = f->per;
    HZ_TRY(launch(a));
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

}  // namespace fb
}  // namespace hz
