// hz_decodebank_plan.h -- the host arithmetic the decoder banks (hz_viterbi.hip, hz_ldpc.hip, hz_rs.hip) share, HIP-free
// so that tests/host/decodebank_plan.cpp can run it under the sanitizers: the limits and input kinds, the validation of
// a call over R rows of `cap` frame slots with a count per row, the leading arguments of the three kernels and which
// slots of a call hold a frame.  The three plan headers refer to it; nothing here knows which bank it serves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace dbp {

constexpr int kBits = 1, kSoftF32 = 32;  // HZSDR_<BANK>_BITS, HZSDR_<BANK>_SOFT_F32
constexpr uint32_t kMaxRows = 8192;
constexpr size_t kMaxFrames = (size_t)1 << 22;  // rows * cap at most

// the bytes of `bits` packed bits
constexpr uint32_t packed_bytes(uint32_t bits) { return (bits + 7) / 8; }

// the scale of soft input is finite and positive
inline const char *check_scale(float scale) { return scale > 0.0f && scale <= 3.402823466e38f ? nullptr : "scale is finite and positive"; }

// ---- a call ----
// What a bank's frames are to a call.  The widths are a frame's extent on either side, in the units of the strides
// (bytes, or floats of soft input): the least pitch from slot to slot.  The dense banks' slots lie a width apart and
// their buffers may overlap in any way; a pitched bank's caller names the pitches, in bytes, and the call may be in
// place, but not overlap in part.
struct Slots {
    size_t in_width, out_width;
    bool pitched;
    const char *in_stride_why, *out_stride_why;  // the bank's words for a row pitch below its cap slots
};
constexpr int kOk = 0, kInvalid = 1, kDstTooSmall = 2;
struct Call {
    uintptr_t in, out;
    size_t in_stride, in_pitch, out_stride, out_pitch, cap, rows;  // (a dense bank: the pitches are the widths)
    bool has_info;
};
// kOk, or what to refuse the call with and why (*why)
inline int check_call(const Slots &s, const Call &c, const char **why) {
    *why = nullptr;
    if (c.cap == 0 || c.cap > kMaxFrames / c.rows) return *why = "cap is at least 1 and rows * cap at most 2^22", kInvalid;
    if (!c.in || !c.out || !c.has_info) return *why = "null in, out or info", kInvalid;
    if (c.in_pitch < s.in_width) return *why = "in_pitch is below the frame bytes", kInvalid;
    if (c.out_pitch < s.out_width) return *why = "out_pitch is below the data bytes", kInvalid;
    if (c.rows > 1 && c.in_stride / c.cap < c.in_pitch) return *why = s.in_stride_why, kInvalid;
    if (c.rows > 1 && c.out_stride / c.cap < c.out_pitch) return *why = s.out_stride_why, kDstTooSmall;
    if (!s.pitched) return kOk;
    // (strides and pitches beyond any address space are refused here, before they are multiplied)
    const size_t lim = (size_t)1 << 40;
    if (c.in_pitch > lim || c.out_pitch > lim || (c.rows > 1 && (c.in_stride > lim || c.out_stride > lim))) return *why = "a pitch or stride beyond 2^40", kInvalid;
    const size_t ispan = (c.rows - 1) * (c.rows > 1 ? c.in_stride : 0) + (c.cap - 1) * c.in_pitch + s.in_width;
    const size_t ospan = (c.rows - 1) * (c.rows > 1 ? c.out_stride : 0) + (c.cap - 1) * c.out_pitch + s.out_width;
    if (c.in == c.out) {
        if (c.in_pitch != c.out_pitch || (c.rows > 1 && c.in_stride != c.out_stride)) return *why = "in place takes equal strides and pitches", kInvalid;
    } else if (c.in < c.out + ospan && c.out < c.in + ispan) {
        return *why = "in and out overlap in part", kInvalid;
    }
    return kOk;
}
// the dense banks' Slots: frames of `in_width` bytes or floats to `out_width` data bytes
constexpr Slots dense(size_t in_width, size_t out_width) {
    return {in_width, out_width, false, "in_stride is below cap frames", "out_stride is below cap frames"};
}

// ---- the kernels ----
// what the three kernels' arguments begin with; each goes on with its own, `cap` and `slots` (R * cap) among them, where
// they lay before the banks shared this: moving them ahead of a bank's tables changed the Viterbi kernel's registers
struct FrameArgs {
    const void *in;
    size_t in_stride;  // bytes (hard bits, symbols) or floats
    const uint32_t *in_counts;
    uint8_t *out;
    size_t out_stride;  // bytes
    uint32_t *info;
};
// the row *r and the frame *f of slot `slot` (below R * cap); whether the slot holds a frame of this call
HZ_HD bool slot_frame(uint32_t slot, uint32_t cap, const uint32_t *in_counts, uint32_t *r, uint32_t *f) {
    *r = slot / cap, *f = slot - *r * cap;
    const uint32_t cnt = in_counts ? in_counts[*r] : cap;
    return *f < (cnt < cap ? cnt : cap);
}

}  // namespace dbp
}  // namespace hz
