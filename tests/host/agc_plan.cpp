// agc_plan.cpp -- csrc/hz_agc_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_agc_plan.py (what it shares with the other row-wave banks, csrc/hz_rowwave_plan.h, by the checks of
// rowwave_check.h).  For every R = 1 ... 8192, both kinds:
//   - the LDS request is (1 + planes) T P * 4 bytes, inside the family's budget;
//   - the waves' rows cover [0, R) exactly once, in order, 1 ... G rows each, G <= kMaxGroup;
// for every rows-per-wave that occurs, from the maps the kernel itself uses, over ALL planes of the request (the gain
// plane and the sample planes):
//   - the loader's / storer's slots are a bijection onto the planes and the walk's slot of (row, sample) is the
//     loader's, one lane per bank in both; the gain plane is plane 0 and the sample planes lie behind it;
// the derivation of iref and the validation of the parameters at their edges;
// no overflow: at the extreme accepted sets, with the error held at -1 (an infinite level) and at +1 (a zero level),
// 2^20 steps of agc_step keep g finite, above zero and inside [gmin, gmax], equal to agc_step_plain and to a float64
// evaluation of g (1 + r e) rounded once and clamped -- under the sanitizer.
// Prints "banks: G planes load walk" per rows-per-wave and kind, "largest lds: bytes", and "agc_plan ok".
#include <cmath>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "hz_agc_plan.h"
#include "rowwave_check.h"

using namespace hz::ap;
namespace am = hz::am;

static void check_geometry(const Geom &g) {
    hz::rw::Geom all = g;  // every plane of the request, the gain plane included
    all.planes = g.planes + 1;
    CHECK((size_t)hz::rw::tile_floats(all) * 4 == g.lds_bytes);
    uint32_t load, walk;
    check_tile(all, &load, &walk);
    CHECK(load == 1 && walk == 1);
    // the planes do not meet: the gain plane is the first T P floats, the sample planes follow
    for (uint32_t t : {0u, g.T - 1})
        for (uint32_t r : {0u, g.G - 1}) {
            CHECK(tile_slot(t, r, kGainPlane, g.P, g.T) < g.T * g.P);
            for (uint32_t p = 0; p < g.planes; p++) {
                const uint32_t s = tile_slot(t, r, kSamplePlane + p, g.P, g.T);
                CHECK(s >= (1 + p) * g.T * g.P && s < (2 + p) * g.T * g.P);
            }
        }
    printf("banks: %u %u %u %u\n", g.G, all.planes, load, walk);
}

static void check_validation() {
    const float good[7] = {1.0f, 0.1f, 0.01f, 0.0f, 1.0f, 0.5f, 2.0f};
    CHECK(check_params(good) == nullptr);
    const float lo = kLow, hi = kHigh, lo_dn = nextafterf(lo, 0.0f), hi_up = nextafterf(hi, INFINITY), half_up = nextafterf(0.5f, 1.0f);
    struct Edge {
        float q[7];
        bool ok;
    };
    const Edge edges[] = {
        {{lo, 0.0f, 0.0f, 0.0f, lo, lo, lo}, true},          {{hi, 0.5f, 0.5f, 3e38f, hi, hi, hi}, true},
        {{lo_dn, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false}, {{hi_up, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false},
        {{0.0f, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false},  {{-1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false},
        {{1.0f, half_up, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false}, {{1.0f, 0.1f, half_up, 0.0f, 1.0f, 0.5f, 2.0f}, false},
        {{1.0f, -1e-45f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false}, {{1.0f, 0.1f, -1e-45f, 0.0f, 1.0f, 0.5f, 2.0f}, false},
        {{1.0f, 0.1f, 0.1f, -1e-45f, 1.0f, 0.5f, 2.0f}, false}, {{1.0f, 0.1f, 0.1f, -0.0f, 1.0f, 0.5f, 2.0f}, true},
        {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, lo_dn, 2.0f}, false},   {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, hi_up}, false},
        {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 1.0f, 1.0f}, true},     {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, nextafterf(1.0f, 2.0f), 2.0f}, false},
        {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, nextafterf(1.0f, 0.0f)}, false}, {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 2.0f, 0.5f}, false},
        {{NAN, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false},     {{1.0f, INFINITY, 0.1f, 0.0f, 1.0f, 0.5f, 2.0f}, false},
        {{1.0f, 0.1f, NAN, 0.0f, 1.0f, 0.5f, 2.0f}, false},     {{1.0f, 0.1f, 0.1f, INFINITY, 1.0f, 0.5f, 2.0f}, false},
        {{1.0f, 0.1f, 0.1f, 0.0f, NAN, 0.5f, 2.0f}, false},     {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, NAN, 2.0f}, false},
        {{1.0f, 0.1f, 0.1f, 0.0f, 1.0f, 0.5f, INFINITY}, false},
    };
    for (const Edge &e : edges) CHECK((check_params(e.q) == nullptr) == e.ok);
    // iref: in float64, exact for powers of two, inside [2^-64, 2^64] at the edges
    CHECK(derive(edges[0].q).iref == kHigh && derive(edges[1].q).iref == kLow);
    const float third[7] = {3.0f, 0.1f, 0.01f, 0.25f, 1.0f, 0.5f, 2.0f};
    const am::Loop k = derive(third);
    CHECK(k.iref == (float)(1.0 / 3.0) && k.attack == 0.1f && k.decay == 0.01f && k.floor == 0.25f && k.gmin == 0.5f && k.gmax == 2.0f);
    CHECK(initial_gain(third) == 1.0f);
}

// 2^20 steps from g_start with the level held at a (infinite: e = -1; zero: e = +1)
static void check_no_overflow(const float *q, float g_start, float a) {
    const am::Loop k = derive(q);
    float g = g_start;
    for (uint32_t n = 0; n < (1u << 20); n++) {
        const float b = am::agc_drive(a, k.iref, k.floor);
        const float e = a == 0.0f ? 1.0f : -1.0f;
        CHECK(fmaf(-b, g, 1.0f) == (a == 0.0f ? 1.0f : -INFINITY));
        const float next = am::agc_step(g, b, k), plain = am::agc_step_plain(g, a, k);
        const double r = e < 0.0f ? (double)k.attack : (double)k.decay;
        float want = (float)((double)g * (1.0 + r * (double)e));  // g (1 + r e): exact in float64, rounded once, as the fmaf
        CHECK(std::isfinite(want) && want > 0.0f && want >= 0.5f * g && want <= 1.5f * g);
        want = want < k.gmin ? k.gmin : (want > k.gmax ? k.gmax : want);
        CHECK(next == want && plain == want);
        CHECK(std::isfinite(next) && next >= k.gmin && next <= k.gmax && next >= kLow && next <= kHigh);
        g = next;
        if (failures) return;
    }
    // (the largest rates reach the range's edge, 128 octaves away at most, well inside 2^20 steps; a rate of 0 holds)
    const float rate = a == 0.0f ? k.decay : k.attack;
    if (rate == 0.5f) CHECK(g == (a == 0.0f ? k.gmax : k.gmin));
    if (rate == 0.0f) CHECK(g == g_start);
}

int main() {
    static_assert(kMaxRows == 8192 && kLanes == 64 && kParams == 7 && kRealF32 == 32 && kC64 == 1, "the limits of include/hzsdr_agc.h");
    static_assert(sizeof(am::Loop) == 24, "six words per row on the device");
    std::set<std::pair<uint32_t, int>> done;
    size_t largest = 0;
    for (uint32_t R = 1; R <= kMaxRows; R++)
        for (int cplx = 0; cplx < 2; cplx++) {
            const Geom g = agc_geom(R, cplx != 0);
            CHECK(g.G >= 1 && g.G <= kMaxGroup && g.G == (R + 1023) / 1024 && g.P >= g.G && (g.P & 1) && g.T == 256 && g.K == kSteps);
            CHECK(g.planes == 1u + cplx && g.lds_bytes == (size_t)(2 + cplx) * g.T * g.P * 4);
            CHECK(g.lds_bytes <= 3u * 256u * 9u * 4u && g.lds_bytes < kLdsBudget);
            if (g.lds_bytes > largest) largest = g.lds_bytes;
            check_rows(g, R);
            if (done.insert({g.G, cplx}).second) check_geometry(g);
        }
    check_validation();
    const float widest[7] = {1.0f, 0.5f, 0.5f, 0.0f, 1.0f, kLow, kHigh}, top[7] = {kLow, 0.5f, 0.5f, 0.0f, kHigh, kHigh, kHigh};
    const float bottom[7] = {kHigh, 0.5f, 0.5f, 0.0f, kLow, kLow, kLow}, slow[7] = {kHigh, 0x1p-24f, 0x1p-24f, 0.0f, 1.0f, kLow, kHigh};
    const float still[7] = {kLow, 0.0f, 0.0f, 0.0f, 1.0f, kLow, kHigh};
    for (const float *q : {widest, top, bottom, slow, still})
        for (float a : {INFINITY, 0.0f})
            for (float g0 : {q[4], q[5], q[6]}) check_no_overflow(q, g0, a);
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("agc_plan ok\n");
    return 0;
}
