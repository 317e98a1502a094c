// hz_plan.h -- what the banks' plan headers (hz_*_plan.h) and math headers share: the host/device marker, the division
// by a reciprocal, and the window transposed by a decimation.  No HIP needed: tests/host/ compiles it with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HZ_HD __host__ __device__ inline
#else
#define HZ_HD inline
#endif

namespace hz {

// floor(w / d) by one multiplication and a shift, magic = floor(2^32 / d) + 1.  With magic * d = 2^32 + e, 0 < e <= d,
// (w * magic) >> 32 = floor(w / d + w e / (d 2^32)), which is floor(w / d) as long as w e < 2^32: EXACT FOR EVERY w WITH
// w * d < 2^32 (any d >= 1; the 64-bit product never wraps).  Each plan states its own range of w and d inside that
// and its test walks it (kDivRange in tests/host/*_plan.cpp).
inline uint64_t div_magic(uint32_t d) { return ((uint64_t)1 << 32) / d + 1; }
HZ_HD uint32_t div_by_magic(uint32_t w, uint64_t magic) { return (uint32_t)((w * magic) >> 32); }

// Value w of a window in LDS transposed by D: row w mod D of J slots, column w / D, so that values D apart -- the lanes
// of one read -- are neighbours.
HZ_HD uint32_t transposed_slot(uint32_t w, uint32_t D, uint32_t J) { return (w % D) * J + w / D; }

}  // namespace hz
