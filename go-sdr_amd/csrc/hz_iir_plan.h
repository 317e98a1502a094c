// hz_iir_plan.h -- the host arithmetic of the IIR bank (include/hzsdr_iir.h), HIP-free so that tests/host/iir_plan.cpp
// can run it under the sanitizers.  The bank is a row-wave bank: how the rows are dealt to waves, the tile and its
// address maps are hz_rowwave_plan.h, with the reasons.  Here: the limits of the cascade, the LDS request and the
// indices of the kept state.
#pragma once
#include "hz_rowwave_plan.h"

namespace hz {
namespace ip {

using rw::kMaxRows, rw::kLanes, rw::kWaves, rw::kMaxGroup, rw::kSteps, rw::kLdsBudget;
using rw::wave_first_row, rw::wave_row_count, rw::tile_slot, rw::move_slot, rw::walk_slot;

constexpr uint32_t kMaxSections = 8;
constexpr uint32_t kRunBytes = 256;  // consecutive bytes of a row that the loads of a tile cover at least

struct Geom : rw::Geom {
    size_t lds_bytes;
};

// rows: 1 ... kMaxRows; sample_bytes: of one input sample (2, 4 or 8); complex_rows: two recursions per row
// (T * sample_bytes >= kRunBytes for every kind: tests/host/iir_plan.cpp)
inline Geom iir_geom(uint32_t rows, uint32_t sample_bytes, bool complex_rows) {
    Geom g{rw::geom(rows, complex_rows), 0};
    g.lds_bytes = (size_t)rw::tile_floats(g) * 4;
    return g;
}

// the floats of the kept state: row, section, z1 / z2, re / im (include/hzsdr_iir.h)
HZ_HD size_t state_index(size_t row, uint32_t s, uint32_t z, uint32_t p, uint32_t S, uint32_t planes) {
    return ((row * S + s) * 2 + z) * planes + p;
}
inline size_t state_floats(uint32_t rows, uint32_t S, uint32_t planes) { return (size_t)rows * S * 2 * planes; }

}  // namespace ip
}  // namespace hz
