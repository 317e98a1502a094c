// iir_plan.cpp -- csrc/hz_iir_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_iir_plan.py (what it shares with the symbol-timing bank, csrc/hz_rowwave_plan.h, by the checks of
// rowwave_check.h).  For every R = 1 ... 8192, each input kind (real float32; complex from 8-, 4- and 2-byte
// samples) and every S = 1 ... 8:
//   - the LDS request is planes * T * P * 4 bytes, inside the family's budget, and a tile covers 256 bytes of a row;
//   - the waves' rows cover [0, R) exactly once, in order, 1 ... G rows each, G <= kMaxGroup;
//   - the state index is a bijection onto [0, state_floats);
// and for every geometry that occurs (rows per wave, steps per lane, planes), from the maps the kernel itself uses:
//   - the loader's slots are a bijection onto the tile, and the recursion's slot of (row, sample) is the loader's;
//   - the lanes per bank, bank = slot mod 32, in each 32-lane group of both accesses (the loader / storer: row fixed,
//     lane = sample; the recursion: sample fixed, lane = row) are 1.
// Prints "banks: G K planes move walk" per geometry, "largest lds: bytes", and "iir_plan ok".
#include <set>
#include <tuple>

#include "hz_iir_plan.h"
#include "rowwave_check.h"

using namespace hz::ip;

static void check_geometry(const Geom &g) {
    uint32_t move, walk;
    check_tile(g, &move, &walk);
    CHECK(move == 1 && walk == 1);
    printf("banks: %u %u %u %u %u\n", g.G, g.K, g.planes, move, walk);
}

int main() {
    static_assert(kMaxRows == 8192 && kMaxSections == 8 && kLanes == 64, "the limits of include/hzsdr_iir.h");
    struct Kind {
        uint32_t bytes;
        bool cplx;
    };
    const Kind kinds[] = {{4, false}, {8, true}, {4, true}, {2, true}};
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> done;
    size_t largest = 0;
    for (uint32_t R = 1; R <= kMaxRows; R++)
        for (const Kind &kd : kinds) {
            const Geom g = iir_geom(R, kd.bytes, kd.cplx);
            CHECK(g.G >= 1 && g.G <= kMaxGroup && g.P >= g.G && (g.P & 1) && g.T == kLanes * g.K && g.K == kSteps);
            CHECK(g.planes == (kd.cplx ? 2u : 1u));
            CHECK((size_t)g.T * kd.bytes >= kRunBytes);
            CHECK(g.lds_bytes == (size_t)g.planes * g.T * g.P * 4 && g.lds_bytes <= kLdsBudget);
            if (g.lds_bytes > largest) largest = g.lds_bytes;
            check_rows(g, R);
            for (uint32_t S = 1; S <= kMaxSections; S++) {
                CHECK(state_floats(R, S, g.planes) == (size_t)R * S * 2 * g.planes);
                // the first, a middle and the last row's state values are consecutive runs in row order
                for (uint32_t r : {0u, R / 2, R - 1}) {
                    size_t want = (size_t)r * S * 2 * g.planes;
                    for (uint32_t s = 0; s < S; s++)
                        for (uint32_t z = 0; z < 2; z++)
                            for (uint32_t p = 0; p < g.planes; p++) CHECK(state_index(r, s, z, p, S, g.planes) == want++);
                }
            }
            if (done.insert({g.G, g.K, g.planes}).second) check_geometry(g);
        }
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("iir_plan ok\n");
    return 0;
}
