// hz_rows.h -- the arithmetic of a call's rows, for Stage::in_rows / out_rows (hz_common.h, hz_ctx.hip): `rows` rows of
// `count` elements of `size` bytes, `pitch` elements from one row's start to the next.  How far the rows reach in the
// caller's memory, what a dense copy of them takes, and which way they travel.  No HIP in here: tests/host/rows_plan.cpp
// compiles it with the host compiler alone.
#pragma once
#include <stddef.h>

namespace hz {
namespace rows {

struct Span {
    bool ok;             // false: a product or sum below does not fit size_t (the other members are then zero)
    size_t elems;        // (rows - 1) * pitch + count: from the first row's first element to the last row's last
    size_t bytes;        // elems * size
    size_t dense_bytes;  // rows * count * size: the rows with no gap between them
};

// (nothing to move -- no rows or no elements -- is a span of zero whatever the pitch)
inline Span span(size_t rows, size_t count, size_t pitch, size_t size) {
    Span s{true, 0, 0, 0};
    if (rows == 0 || count == 0) return s;
    size_t gap, dense;
    if (__builtin_mul_overflow(rows - 1, pitch, &gap) || __builtin_add_overflow(gap, count, &s.elems) ||
        __builtin_mul_overflow(s.elems, size, &s.bytes) || __builtin_mul_overflow(rows, count, &dense) ||
        __builtin_mul_overflow(dense, size, &s.dense_bytes))
        return Span{false, 0, 0, 0};
    return s;
}

enum Route {
    kNothing,  // no rows or no elements: nothing is staged, nothing comes back
    kDense,    // one row, or no gap between the rows: one buffer of dense_bytes through Stage::in / out, all its routes
    kCaller,   // the kernel gets the caller's pointer and pitch
    kCopy2D,   // a dense copy in a device slot, one 2-D copy between it and the caller's rows
};

// host: a HOST context; pinned: the span's bytes lie inside memory the library pinned (asked only where it decides);
// dense_run: rows with no gap between them travel as one buffer (false: as rows with a gap do -- out_rows' keep_rows)
inline Route route(bool host, size_t rows, size_t count, size_t pitch, bool pinned, bool dense_run = true) {
    if (rows == 0 || count == 0) return kNothing;
    if (rows == 1 || (pitch == count && dense_run)) return kDense;
    return !host || pinned ? kCaller : kCopy2D;
}

}  // namespace rows
}  // namespace hz
