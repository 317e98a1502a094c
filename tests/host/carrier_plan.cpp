// carrier_plan.cpp -- csrc/hz_carrier_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_carrier_plan.py (what it shares with the IIR and the symbol-timing bank, csrc/hz_rowwave_plan.h, by the
// checks of rowwave_check.h).  For every R = 1 ... 8192, with and without the track:
//   - the LDS request is (2 + track) T P * 4 bytes, inside the family's budget;
//   - the waves' rows cover [0, R) exactly once, in order, 1 ... G rows each, G <= kMaxGroup;
//   - the state index is a bijection onto [0, state_words), theta before F;
// for every rows-per-wave that occurs, from the maps the kernel itself uses:
//   - the loader's slots are a bijection onto the re and im planes and the walk's slot of (row, sample) is the
//     loader's, one lane per bank in both; the track plane's slots lie behind them, inside the request, a bijection and
//     one lane per bank likewise;
// the derivation of the constants and the validation of the parameters at their edges;
// no int32 overflow: at the extreme accepted sets, with an error held at +1 and at -1 (the largest |dF| and |dtheta|
// the products give), 2^20 samples of steps 3 to 5 evaluated in int64 beside the int32 of hz_carrier_math.h: the two
// agree at every sample, |dF|, |dtheta| <= 2^29 and F stays inside its range -- and car_step itself, fed samples that
// hold the clipped error at +-1, under the sanitizer.
// Prints "banks: G load walk track_load track_walk" per rows-per-wave, "largest lds: bytes", and "carrier_plan ok".
#include <cmath>
#include <cstring>
#include <set>
#include <vector>

#include "hz_carrier_plan.h"
#include "rowwave_check.h"

using namespace hz::cp;
namespace cm = hz::cm;
namespace tn = hz::tn;

static void check_geometry(const Geom &g) {
    uint32_t load, walk, tload = 0, twalk = 0;
    check_tile(g, &load, &walk);
    const uint32_t base = hz::rw::tile_floats(g), floats = (uint32_t)(g.lds_bytes / 4);
    CHECK(floats == base + g.T * g.P);
    std::vector<int> seen(floats, 0);
    for (uint32_t r = 0; r < g.G; r++)
        for (uint32_t k = 0; k < g.K; k++) {
            std::vector<uint32_t> slots;
            for (uint32_t lane = 0; lane < kLanes; lane++) {
                const uint32_t s = move_slot(lane, k, r, kTrackPlane, g.P, g.T);
                CHECK(s >= base && s < floats);
                if (s < floats) seen[s]++;
                CHECK(s == walk_slot(r, lane + kLanes * k, kTrackPlane, g.P, g.T));
                slots.push_back(s);
            }
            const uint32_t w = worst(slots);
            if (w > tload) tload = w;
        }
    for (uint32_t t = 0; t < g.T; t++) {
        std::vector<uint32_t> slots;
        for (uint32_t lane = 0; lane < g.G; lane++) slots.push_back(walk_slot(lane, t, kTrackPlane, g.P, g.T));
        const uint32_t w = worst(slots);
        if (w > twalk) twalk = w;
    }
    uint32_t used = 0;
    for (uint32_t s = 0; s < floats; s++) {
        CHECK(seen[s] <= 1);
        used += seen[s];
    }
    CHECK(used == g.T * g.G);
    CHECK(load == 1 && walk == 1 && tload == 1 && twalk == 1);
    printf("banks: %u %u %u %u %u\n", g.G, load, walk, tload, twalk);
}

static void check_validation() {
    const float good[5] = {0.01f, 0.0001f, 0.01f, -0.02f, 0.02f};
    CHECK(check_params(good) == nullptr);
    const cm::Loop k = derive(good);
    CHECK(k.aw == (float)((double)0.01f * 4294967296.0) && k.bw == (float)((double)0.0001f * 4294967296.0));
    CHECK(k.f0 == (int32_t)llrint((double)0.01f * 4294967296.0) && k.fmin == (int32_t)llrint((double)-0.02f * 4294967296.0));
    CHECK(k.fmax == -k.fmin && k.fmin <= k.f0 && k.f0 <= k.fmax);
    const float up = nextafterf(0.125f, 1.0f), q = 0.25f, qup = nextafterf(0.25f, 1.0f);
    struct Edge {
        float q[5];
        bool ok;
    };
    const Edge edges[] = {
        {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, true},      {{0.125f, 0.125f, 0.0f, -q, q}, true},
        {{up, 0.0f, 0.0f, 0.0f, 0.0f}, false},       {{0.0f, up, 0.0f, 0.0f, 0.0f}, false},
        {{-1e-9f, 0.0f, 0.0f, 0.0f, 0.0f}, false},   {{0.0f, -1e-9f, 0.0f, 0.0f, 0.0f}, false},
        {{0.0f, 0.0f, q, q, q}, true},               {{0.0f, 0.0f, -q, -q, -q}, true},
        {{0.0f, 0.0f, 0.0f, -qup, 0.0f}, false},     {{0.0f, 0.0f, 0.0f, 0.0f, qup}, false},
        {{0.0f, 0.0f, 0.1f, 0.11f, 0.2f}, false},    {{0.0f, 0.0f, 0.21f, 0.1f, 0.2f}, false},
        {{0.0f, 0.0f, 0.0f, 0.1f, -0.1f}, false},    {{0.0f, 0.0f, 0.1f, 0.1f, 0.1f}, true},
        {{NAN, 0.0f, 0.0f, 0.0f, 0.0f}, false},      {{0.0f, INFINITY, 0.0f, 0.0f, 0.0f}, false},
        {{0.0f, 0.0f, NAN, -q, q}, false},           {{0.0f, 0.0f, 0.0f, -INFINITY, q}, false},
        {{0.0f, 0.0f, 0.0f, -q, NAN}, false},
    };
    for (const Edge &e : edges) CHECK((check_params(e.q) == nullptr) == e.ok);
    // the extremes of the derived constants
    const float ext[5] = {0.125f, 0.125f, 0.25f, -0.25f, 0.25f};
    const cm::Loop x = derive(ext);
    CHECK(x.aw == 0x1p29f && x.bw == 0x1p29f && x.f0 == (1 << 30) && x.fmin == -(1 << 30) && x.fmax == (1 << 30));
}

// steps 3 to 5 with the error held at e, 2^20 samples, in int64 beside the header's int32
static void check_no_overflow(const float *q, int32_t f_start, float e) {
    const cm::Loop k = derive(q);
    const int64_t lim = 1ll << 29;
    int32_t f = f_start;
    int64_t wide = f_start;
    uint32_t theta = 0;
    uint64_t theta_wide = 0;
    for (uint32_t n = 0; n < (1u << 20); n++) {
        const float pb = k.bw * e, pa = k.aw * e;
        CHECK(fabsf(pb) <= 0x1p29f && fabsf(pa) <= 0x1p29f);
        const int32_t df = cm::to_i32(pb), dth = cm::to_i32(pa);
        CHECK(df >= -lim && df <= lim && dth >= -lim && dth <= lim);
        int64_t w = wide + df;
        CHECK(w >= INT32_MIN && w <= INT32_MAX);
        w = w < k.fmin ? k.fmin : w;
        w = w > k.fmax ? k.fmax : w;
        wide = w;
        int32_t g = (int32_t)((uint32_t)f + (uint32_t)df);
        g = g < k.fmin ? k.fmin : g;
        g = g > k.fmax ? k.fmax : g;
        f = g;
        CHECK((int64_t)f == wide && f >= k.fmin && f <= k.fmax);
        theta = theta + (uint32_t)f + (uint32_t)dth;
        theta_wide = (theta_wide + (uint64_t)(int64_t)f + (uint64_t)(int64_t)dth) & 0xffffffffull;
        CHECK(theta == (uint32_t)theta_wide);
        if (failures) return;
    }
}

// car_step itself at the extreme sets: samples that keep the clipped error at +-1 whatever the phase (TONE: the sample
// turned a quarter ahead of or behind the oscillator, three times the unit), under the sanitizer
template <int MODE> static void check_step_extreme(const float *q, float sign) {
    const cm::Loop k = derive(q);
    cm::State s{0u, k.f0};
    for (uint32_t n = 0; n < (1u << 20); n++) {
        float c, sn;
        cm::car_unit(s.theta + (sign > 0 ? 0x40000000u : 0xc0000000u), &c, &sn);
        tn::c32 y;
        const float track = cm::car_step<MODE>(s, k, tn::c32{3.0f * c, 3.0f * sn}, &y);
        CHECK(s.f >= k.fmin && s.f <= k.fmax && track == (float)s.f * 0x1p-32f);
        if (MODE == cm::kTone) CHECK(sign > 0 ? y.im > 1.0f : y.im < -1.0f);
        if (failures) return;
    }
    if (MODE == cm::kTone) CHECK(s.f == (sign > 0 ? k.fmax : k.fmin));
}

int main() {
    static_assert(kMaxRows == 8192 && kLanes == 64 && kParams == 5 && kStateWords == 2, "the limits of include/hzsdr_carrier.h");
    static_assert(sizeof(cm::Loop) == 20, "five words per row on the device");
    std::set<uint32_t> done;
    size_t largest = 0;
    for (uint32_t R = 1; R <= kMaxRows; R++)
        for (int track = 0; track < 2; track++) {
            const Geom g = carrier_geom(R, track != 0);
            CHECK(g.G >= 1 && g.G <= kMaxGroup && g.G == (R + 1023) / 1024 && g.P >= g.G && (g.P & 1) && g.T == 256 && g.K == kSteps);
            CHECK(g.planes == 2 && g.lds_bytes == (size_t)(2 + track) * g.T * g.P * 4);
            CHECK(g.lds_bytes <= 3u * 256u * 9u * 4u && g.lds_bytes < kLdsBudget);
            if (g.lds_bytes > largest) largest = g.lds_bytes;
            check_rows(g, R);
            CHECK(state_words(R) == (size_t)R * 2);
            for (uint32_t r : {0u, R / 2, R - 1}) CHECK(state_index(r, 0) == (size_t)r * 2 && state_index(r, 1) == (size_t)r * 2 + 1);
            if (track && done.insert(g.G).second) check_geometry(g);
        }
    check_validation();
    const float widest[5] = {0.125f, 0.125f, 0.0f, -0.25f, 0.25f}, top[5] = {0.125f, 0.125f, 0.25f, 0.25f, 0.25f};
    const float bottom[5] = {0.125f, 0.125f, -0.25f, -0.25f, -0.25f}, narrow[5] = {0.125f, 0.125f, 0.25f, -0.25f, 0.25f};
    for (const float *q : {widest, top, bottom, narrow})
        for (float e : {1.0f, -1.0f, nextafterf(1.0f, 0.0f), -nextafterf(1.0f, 0.0f)}) {
            const cm::Loop k = derive(q);
            for (int32_t f0 : {k.f0, k.fmin, k.fmax}) check_no_overflow(q, f0, e);
        }
    for (const float *q : {widest, narrow}) {
        check_step_extreme<cm::kTone>(q, 1.0f);
        check_step_extreme<cm::kTone>(q, -1.0f);
        check_step_extreme<cm::kBpsk>(q, 1.0f);
        check_step_extreme<cm::kQpsk>(q, -1.0f);
    }
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("carrier_plan ok\n");
    return 0;
}
