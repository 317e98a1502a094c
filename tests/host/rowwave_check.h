// rowwave_check.h -- what the plan programs of the row-wave banks (iir_plan.cpp, symsync_plan.cpp) check alike, over
// csrc/hz_rowwave_plan.h: CHECK, the lanes per bank of an access, the rows dealt to the waves, and the sample tile's
// address maps.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

#include "hz_rowwave_plan.h"

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            if (failures++ < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                          \
    } while (0)

// the largest number of lanes of one 32-lane group that share a bank
static uint32_t worst(const std::vector<uint32_t> &slots) {
    uint32_t w = 0;
    for (size_t base = 0; base < slots.size(); base += 32) {
        uint32_t per[32] = {0};
        for (size_t l = base; l < base + 32 && l < slots.size(); l++) {
            const uint32_t c = ++per[slots[l] % 32];
            if (c > w) w = c;
        }
    }
    return w;
}

// the waves' rows cover [0, R) exactly once, in order, 1 ... G rows each
static void check_rows(const hz::rw::Geom &g, uint32_t R) {
    using namespace hz::rw;
    uint32_t next = 0;
    CHECK(g.waves == (R + g.G - 1) / g.G);
    for (uint32_t w = 0; w < g.waves; w++) {
        const uint32_t c = wave_row_count(w, g.G, R);
        CHECK(wave_first_row(w, g.G) == next && c >= 1 && c <= g.G);
        next += c;
    }
    CHECK(next == R && wave_row_count(g.waves, g.G, R) == 0);
}

// the loader's slots are a bijection onto the tile's used floats, and the walk's slot of (row, sample) is the loader's;
// *move, *walk: the lanes per bank of the loader / storer (row fixed, lane = sample) and of the walk (sample fixed,
// lane = row)
static void check_tile(const hz::rw::Geom &g, uint32_t *move, uint32_t *walk) {
    using namespace hz::rw;
    const uint32_t floats = tile_floats(g);
    std::vector<int> seen(floats, 0);
    *move = *walk = 0;
    for (uint32_t p = 0; p < g.planes; p++) {
        for (uint32_t r = 0; r < g.G; r++)
            for (uint32_t k = 0; k < g.K; k++) {
                std::vector<uint32_t> slots;
                for (uint32_t lane = 0; lane < kLanes; lane++) {
                    const uint32_t s = move_slot(lane, k, r, p, g.P, g.T);
                    CHECK(s < floats);
                    if (s < floats) seen[s]++;
                    CHECK(s == walk_slot(r, lane + kLanes * k, p, g.P, g.T));
                    slots.push_back(s);
                }
                const uint32_t w = worst(slots);
                if (w > *move) *move = w;
            }
        for (uint32_t t = 0; t < g.T; t++) {
            std::vector<uint32_t> slots;
            for (uint32_t lane = 0; lane < g.G; lane++) slots.push_back(walk_slot(lane, t, p, g.P, g.T));
            const uint32_t w = worst(slots);
            if (w > *walk) *walk = w;
        }
    }
    uint32_t used = 0;
    for (uint32_t s = 0; s < floats; s++) {
        CHECK(seen[s] <= 1);
        used += seen[s];
    }
    CHECK(used == g.planes * g.T * g.G);
}
