// hz_decodebank.h -- the host side of the decoder banks (hz_viterbi.hip, hz_ldpc.hip, hz_rs.hip): what their objects
// hold alike and the calls over it, around the kernels.  A bank's object derives from Bank and adds its configuration,
// its geometry, its device tables and, as a static, the noun that starts its messages.  A bank decodes
// min(counts[r], cap) frames of every row into a block of data bytes and an info word per slot, leaves every other slot
// as it was and keeps no state; the arithmetic of a call is hz_decodebank_plan.h.  Nothing here knows which bank it serves.
// The demapper bank (hz_demap.hip) in front of them is the same call with floats on both sides and no info word: run().
#pragma once
#include <string>

#include "hz_common.h"
#include "hz_decodebank_plan.h"

namespace hz {
// (hidden: the instantiations below add nothing to the library's dynamic symbols)
namespace db __attribute__((visibility("hidden"))) {

struct Bank {
    hzsdr_ctx *ctx = nullptr;
    uint32_t R = 0;
};

template <class F> std::string who(const char *msg) { return std::string(F::noun) + ": " + msg; }

// the checks in front of a create (a bank of one input kind passes kBits)
template <class F> int check_create(hzsdr_ctx *ctx, int kind, size_t rows, F **out) {
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (kind != dbp::kBits && kind != dbp::kSoftF32) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, who<F>("packed bits or soft float32 input"));
    if (rows == 0 || rows > dbp::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, who<F>("1 ... 8192 rows"));
    return HZSDR_OK;
}

// (a create's device tables: Table and upload of hz_common.h)
using hz::Table;
using hz::upload;

// A call: the checks in their order, the rows staged (`isz`: the bytes of an input element), launch(FrameArgs, cap,
// slots) -> status with the leading part of the kernel's arguments filled in, the rows brought back.
// `osz`: the bytes of an output element (the decoders write bytes; hz_demap.hip writes floats and has no info word:
// a null `info` is not staged); `check(&why)` is the call's validation.
template <class F, class Check, class Launch>
int run(F *f, const dbp::Slots &s, size_t isz, size_t osz, const dbp::Call &c, const uint32_t *in_counts, uint32_t *info, Check check, Launch launch) {
    hzsdr_ctx *ctx = f->ctx;
    const char *why = nullptr;
    const int bad = check(&why);
    if (bad) return fail(ctx, bad == dbp::kDstTooSmall ? HZSDR_ERR_DST_TOO_SMALL : HZSDR_ERR_INVALID_ARGUMENT, who<F>(why));
    HZ_TRY(enter(ctx));
    Stage st(ctx);
    const size_t R = c.rows, cap = c.cap;
    const size_t iw = (cap - 1) * c.in_pitch + s.in_width, ow = (cap - 1) * c.out_pitch + s.out_width;
    const void *din, *dic = nullptr;
    void *dout = (void *)c.out, *dinfo = info;
    size_t istride = R > 1 ? c.in_stride : iw, ostride = R > 1 ? c.out_stride : ow;
    HZ_TRY(st.in_rows(0, (const void *)c.in, R, iw, istride, isz, &din, &istride));
    if (in_counts) HZ_TRY(st.in(1, in_counts, R * sizeof(uint32_t), &dic));
    // the slots behind a row's count, and what lies between a slot's data and the next slot, stay as they are
    HZ_TRY(stage_out_rows_preserved(st, 2, (void *)c.out, R, ow, c.out_stride, osz, &dout, &ostride));
    if (info) HZ_TRY(st.out_preserve(3, info, R * cap * sizeof(uint32_t), &dinfo));
    HZ_TRY(launch(dbp::FrameArgs{din, istride, (const uint32_t *)dic, (uint8_t *)dout, ostride, (uint32_t *)dinfo}, (uint32_t)cap, (uint32_t)(R * cap)));
    HZ_HIP(ctx, hipGetLastError());
    return st.finish();
}
template <class F, class Launch>
int decode(F *f, const dbp::Slots &s, size_t isz, const dbp::Call &c, const uint32_t *in_counts, uint32_t *info, Launch launch) {
    return run(f, s, isz, 1, c, in_counts, info, [&](const char **why) { return dbp::check_call(s, c, why); }, launch);
}

}  // namespace db
}  // namespace hz
