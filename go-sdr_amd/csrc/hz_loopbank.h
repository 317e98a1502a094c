// hz_loopbank.h -- the host side of the row-wave banks (hz_iir.hip, hz_symsync.hip, hz_carrier.hip, hz_agc.hip): what
// their objects hold alike and the calls over it, around the kernels that hz_rowwave.h describes.  Two layers:
//   Bank      rows, a state array of 32-bit words on the device that the caller may read and replace, the position;
//             get_state, set_state, position, plan, the equal-count push around a launch, destroy.  The IIR bank stops
//             here: its coefficients, its create and its reset are its own.
//   LoopBank  on top, parameter sets -- one for all rows, or one per row -- and the loop constants derived from them
//             (their bookkeeping, HIP-free, is hz_paramsets.h); create, set_params, reset.  The symbol-timing bank adds its smallest advance and a device word behind
//             these, and keeps its own push (a bound, a destination preserved, counts).
// A bank's object derives from one of the two and adds its kind and its geometry `g`; a loop bank describes itself by
// a struct B:
//   Obj                          the object, a LoopBank; Obj::noun starts its messages
//   kParams                      floats per parameter set
//   check_params(p) -> why       the refusal of one set, or null
//   derive(p) -> Obj::Loop       one set's loop constants
//   check_kind(ctx, kind)        the status and message of a kind the bank does not have
//   shape(f, kind)               kind, geometry and state words of the new object (ctx, R, per_row are set)
//   initial(f, r, set, z)        row r's entries of the initial state z (+0 elsewhere) from parameter set `set`
// The equalizer bank (hz_equalizer.hip), whose create takes a mode, a tap count and a centre beside the kind, has a create
// of its own over stage_params, commit_params and initial_state, and a push of its own; the rest it takes from here.
// Nothing here knows which bank it serves.
#pragma once
#include "hz_common.h"
#include "hz_paramsets.h"
#include "hz_rowwave_plan.h"

namespace hz {
namespace lb {

template <typename W> struct Bank {
    static_assert(sizeof(W) == sizeof(uint32_t), "the state moves as 32-bit words");
    hzsdr_ctx *ctx = nullptr;
    uint32_t R = 0;
    bool per_row = false;
    W *state = nullptr;  // `words` of them on the device
    size_t words = 0;
    uint64_t pos = 0;  // samples consumed per row
};

template <typename L, typename W> struct LoopBank : Bank<W>, ParamSets<L> {
    using Loop = L;
    using Word = W;
    L *loop_rows = nullptr;  // per_row: `loop` on the device
    size_t sets() const { return this->per_row ? this->R : 1; }
};

// ---- Bank ----

inline int state_get(hzsdr_ctx *ctx, const char *who, void *dst, size_t cap, const void *src_dev, size_t words) {
    if (cap < words) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, std::string(who) + ": the state array is too small");
    HZ_TRY(enter(ctx));
    HZ_HIP(ctx, hipMemcpyAsync(dst, src_dev, words * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return HZSDR_OK;
}

template <class F, typename W> int get_state(F *f, W *state, size_t cap) {
    if (!f || !state) return HZSDR_ERR_INVALID_ARGUMENT;
    return state_get(f->ctx, F::noun, state, cap, f->state, f->words);
}

// msg: what the state has, behind the noun
template <class F, typename W> int set_state(F *f, const W *state, size_t count, uint64_t position, const char *msg) {
    if (!f || !state) return HZSDR_ERR_INVALID_ARGUMENT;
    if (count != f->words) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string(F::noun) + ": " + msg);
    HZ_TRY(enter(f->ctx));
    HZ_TRY(bank_upload(f->ctx, f->state, state, f->words * sizeof(uint32_t)));  // (the caller's array is free to go)
    f->pos = position;
    return HZSDR_OK;
}

template <class F> int position(const F *f, uint64_t *position) {
    if (!f || !position) return HZSDR_ERR_INVALID_ARGUMENT;
    *position = f->pos;
    return HZSDR_OK;
}

// form: the bank's own flags (f is not null)
template <class F> int plan(const F *f, size_t *rows_per_wave, size_t *tile_samples, int *form_out, int form) {
    if (rows_per_wave) *rows_per_wave = f->g.G;
    if (tile_samples) *tile_samples = f->g.T;
    if (form_out) *form_out = form;
    return HZSDR_OK;
}

// behind whatever still runs on the context's stream the state and the bank's `own` device buffers go, then the object
// (f is not null: the caller has read `own` out of it)
template <class F> int destroy(F *f, std::initializer_list<void *> own) {
    bank_release(f->ctx, {f->state});
    for (void *p : own)
        if (p) (void)hipFree(p);
    delete f;
    return HZSDR_OK;
}

// The rows of a push as the caller gives them (p null: no such rows), and as the kernel gets them.
struct RowsIn {
    const void *p;
    size_t stride, size;  // samples from row to row; bytes per sample
};
struct RowsOut {
    void *p;
    size_t cap, stride, size;
};
struct DevRows {
    const void *in;
    size_t in_stride;
    void *out;
    size_t out_stride;
    float *track;
    size_t track_stride;
};

// A push of n samples per row that writes n outputs per row and, where asked for, n float32 track values: the checks
// in their order, the rows staged, launch(DevRows) -> status, the position moved, the rows brought back.  In place
// (out.p == in.p) is for rows whose outputs have the size of their samples.
template <class F, class Launch> int push_rows(F *f, size_t n, RowsIn in, RowsOut out, RowsOut track, Launch launch) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = f->ctx;
    const size_t R = f->R;
    const std::string who = F::noun, w = who + ": ";
    if (n && !in.p) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "null input");
    if (R > 1 && in.stride < n) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "in_stride is below the samples of the push");
    if (f->pos + n < f->pos) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "the push is too long");
    HZ_TRY(check_rows_out(ctx, F::noun, R, out.p, out.cap, out.stride, n, 0));
    if (track.p) HZ_TRY(check_rows_out(ctx, (who + " track").c_str(), R, track.p, track.cap, track.stride, n, 0));
    if (n && in.p == out.p) {
        if (in.size != out.size) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "in place is for float32 and complex64 rows");
        if (R > 1 && in.stride != out.stride) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "in place needs equal strides");
    }
    HZ_TRY(enter(ctx));
    if (n == 0) return HZSDR_OK;
    Stage st(ctx);
    DevRows d{};
    void *dtrack = nullptr;
    HZ_TRY(st.in_rows(0, in.p, R, n, in.stride, in.size, &d.in, &d.in_stride));
    HZ_TRY(st.out_rows(1, out.p, R, n, out.stride, out.size, &d.out, &d.out_stride));
    if (track.p) HZ_TRY(st.out_rows(2, track.p, R, n, track.stride, track.size, &dtrack, &d.track_stride));
    d.track = (float *)dtrack;
    HZ_TRY(launch(d));
    f->pos += n;
    return st.finish();
}

// ---- LoopBank ----

// the sets at `params` checked and derived into `next` (hz_paramsets.h); the object is only read
template <class B> int stage_params(const typename B::Obj *f, const float *params, ParamSets<typename B::Obj::Loop> &next) {
    const std::string w = std::string(B::Obj::noun) + ": ";
    if (!params) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, w + "null params");
    if (const char *why = stage_sets<B>(params, f->sets(), next)) return fail(f->ctx, HZSDR_ERR_INVALID_ARGUMENT, w + why);
    return HZSDR_OK;
}

// staged sets into the object: the host's copy, the derived constants, and the device's rows of constants (per-row
// parameters; shared ones travel with each launch).  The device's rows go first: a copy that fails leaves the object
// as it was.
template <class F> int commit_params(F *f, ParamSets<typename F::Loop> &next) {
    if (f->per_row) HZ_TRY(bank_upload(f->ctx, f->loop_rows, next.loop.data(), next.loop.size() * sizeof(typename F::Loop)));
    f->params.swap(next.params);
    f->loop.swap(next.loop);
    return HZSDR_OK;
}

template <class B> int initial_state(typename B::Obj *f) {
    std::vector<typename B::Obj::Word> z(f->words, 0);
    for (size_t r = 0; r < f->R; r++) B::initial(f, r, f->per_row ? r : 0, z.data());
    HZ_TRY(bank_upload(f->ctx, f->state, z.data(), f->words * sizeof(uint32_t)));
    f->pos = 0;
    return HZSDR_OK;
}

// Two ways back: before the context is entered nothing is on the device and the object is deleted as it is; behind it,
// destroy() waits for the stream and releases what was allocated so far.
template <class B> int create(hzsdr_ctx *ctx, int kind, const float *params, int per_row, size_t rows, typename B::Obj **out) {
    using Obj = typename B::Obj;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    HZ_TRY(B::check_kind(ctx, kind));
    if (rows == 0 || rows > rw::kMaxRows) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, std::string(Obj::noun) + ": 1 ... 8192 rows");
    Obj *f = new Obj{};
    f->ctx = ctx, f->R = (uint32_t)rows, f->per_row = per_row != 0;
    auto undo = [&](int rc) {
        destroy(f, {f->loop_rows});
        return rc;
    };
    ParamSets<typename Obj::Loop> next;
    int rc = stage_params<B>(f, params, next);
    if (rc == HZSDR_OK) rc = enter(ctx);
    if (rc != HZSDR_OK) {
        delete f;
        return rc;
    }
    B::shape(f, kind);
    hipError_t e = hipMalloc((void **)&f->state, f->words * sizeof(uint32_t));
    if (e == hipSuccess && f->per_row) e = hipMalloc((void **)&f->loop_rows, (size_t)f->R * sizeof(typename Obj::Loop));
    if (e != hipSuccess) return undo(hip_fail(ctx, e, (std::string(Obj::noun) + "_create").c_str(), __FILE__, __LINE__));
    rc = commit_params(f, next);
    if (rc == HZSDR_OK) rc = initial_state<B>(f);
    if (rc != HZSDR_OK) return undo(rc);
    *out = f;
    return HZSDR_OK;
}

template <class B> int set_params(typename B::Obj *f, const float *params) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    ParamSets<typename B::Obj::Loop> next;
    HZ_TRY(stage_params<B>(f, params, next));
    HZ_TRY(enter(f->ctx));
    return commit_params(f, next);  // (behind the pushes so far on the context's stream)
}

template <class B> int reset(typename B::Obj *f) {
    if (!f) return HZSDR_ERR_INVALID_ARGUMENT;
    HZ_TRY(enter(f->ctx));
    return initial_state<B>(f);
}

}  // namespace lb
}  // namespace hz
