// symsync_plan.cpp -- csrc/hz_symsync_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_symsync_plan.py (what it shares with the IIR bank, csrc/hz_rowwave_plan.h, by the checks of
// rowwave_check.h).  For every R = 1 ... 8192 and both kinds:
//   - the LDS request is (planes T P + planes (T / 2 + 1) P) * 4 bytes, under 28 KiB and so inside the family's budget;
//   - the waves' rows cover [0, R) exactly once, in order, 1 ... G rows each, G <= kMaxGroup;
//   - the state index is a bijection onto [0, state_floats), in the documented order;
// for every geometry that occurs (rows per wave, planes), from the maps the kernel itself uses:
//   - the loader's slots are a bijection onto the sample tile and the walk's slot of (row, sample) is the loader's; the
//     storer's slots are a bijection onto the symbol tile and the walk's slot of (row, symbol) is the storer's; the two
//     tiles do not overlap;
//   - the lanes per bank, bank = slot mod 32, in each 32-lane group of the four accesses (the loader's write: row fixed,
//     lane = sample; the walk's sample read: sample fixed, lane = row; the walk's symbol write: symbol fixed, lane =
//     row -- the rows in step, see hz_symsync_plan.h; the storer's read: row fixed, lane = symbol) are 1;
// the symbol tile's size: for every strobe pattern over T = 1 ... 16 samples that the invariants allow (any subset of
// the samples holds a strobe, at most one each; the flag alternates from either start) no row emits more than
// tile_symbols(T), and for T = 256 the densest pattern (a strobe in every sample) stays inside it;
// the bound: for every n = 0 ... 700 and a grid of smallest advances, a float32 counter that advances by the smallest
// advance at EVERY strobe (denser than any real row) from every start in a grid, the flag either way, emits at most
// max_symbols(n, amin), also when its first mid-symbol advance is the 1 that an exchange of parameters may leave in h;
// the validation of the parameters at its edges; and sync_idle of hz_symsync_math.h (the kernel's
// way through a sample in which no lane has a strobe) against sync_step, every state word.
// Prints "banks: G planes load walk emit store" per geometry, "largest lds: bytes", and "symsync_plan ok".
#include <cmath>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "hz_symsync_plan.h"
#include "rowwave_check.h"

using namespace hz::sp;

static void check_geometry(const Geom &g) {
    const uint32_t samples = g.planes * g.T * g.P, symbols = g.planes * g.Y * g.P;
    CHECK(g.sym_base == samples && g.lds_bytes == (size_t)(samples + symbols) * 4);
    std::vector<int> seen_y(symbols, 0);
    uint32_t load, walk, emit = 0, store = 0;
    check_tile(g, &load, &walk);
    const uint32_t steps = (g.Y + kLanes - 1) / kLanes;
    for (uint32_t p = 0; p < g.planes; p++) {
        for (uint32_t r = 0; r < g.G; r++)
            for (uint32_t j = 0; j < steps; j++) {
                std::vector<uint32_t> slots;
                for (uint32_t lane = 0; lane < kLanes && lane + kLanes * j < g.Y; lane++) {
                    const uint32_t s = store_slot(lane, j, r, p, g.P, g.Y);
                    CHECK(s < symbols);
                    if (s < symbols) seen_y[s]++;
                    CHECK(s == emit_slot(r, lane + kLanes * j, p, g.P, g.Y));
                    slots.push_back(s);
                }
                const uint32_t w = worst(slots);
                if (w > store) store = w;
            }
        for (uint32_t k = 0; k < g.Y; k++) {
            std::vector<uint32_t> slots;
            for (uint32_t lane = 0; lane < g.G; lane++) slots.push_back(emit_slot(lane, k, p, g.P, g.Y));
            const uint32_t w = worst(slots);
            if (w > emit) emit = w;
        }
    }
    uint32_t used_y = 0;
    for (uint32_t s = 0; s < symbols; s++) {
        CHECK(seen_y[s] <= 1);
        used_y += seen_y[s];
    }
    CHECK(used_y == g.planes * g.Y * g.G);
    CHECK(load == 1 && walk == 1 && emit == 1 && store == 1);
    printf("banks: %u %u %u %u %u %u\n", g.G, g.planes, load, walk, emit, store);
}

// the symbols of a tile of T samples whose sample t holds a strobe when bit t of `pattern` is set, from `flag`
static uint32_t emitted(uint32_t T, uint64_t pattern, uint32_t flag) {
    uint32_t k = 0;
    for (uint32_t t = 0; t < T; t++)
        if (pattern >> t & 1) {
            k += flag;
            flag ^= 1u;
        }
    return k;
}

static void check_tile_symbols() {
    for (uint32_t T = 1; T <= 16; T++) {
        uint32_t most = 0;
        for (uint64_t pattern = 0; pattern < (1ull << T); pattern++)
            for (uint32_t flag = 0; flag < 2; flag++) {
                const uint32_t k = emitted(T, pattern, flag);
                if (k > most) most = k;
            }
        CHECK(most == (T + 1) / 2 && most <= tile_symbols(T));
    }
    // T = 256 in four words of 64: a strobe in every sample, the flag set first
    uint32_t k = 0, flag = 1;
    for (int w = 0; w < 4; w++) {
        k += emitted(64, ~0ull, flag);  // (64 strobes leave the flag where it was)
    }
    CHECK(k == 128 && k < tile_symbols(kLanes * kSteps) && tile_symbols(kLanes * kSteps) == 129);
}

// symbols of n samples by a float32 counter that advances by `a` at every strobe, from the counter c0 and `flag`
static uint64_t densest(uint64_t n, float a, float c0, uint32_t flag, bool *below) {
    float c = c0;
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (c < 1.0f) {
            k += flag;
            flag ^= 1u;
            c = c + a;
        }
        c = c - 1.0f;
        if (c < 0.0f) *below = true;
    }
    return k;
}

// the same behind a parameter exchange: the FIRST mid-symbol advance is `old_h`, what the row still held (at least 1,
// the least any accepted h can be); every other advance is `a`
static uint64_t densest_after_exchange(uint64_t n, float a, float old_h, float c0, uint32_t flag) {
    float c = c0;
    uint64_t k = 0;
    bool old = true;
    for (uint64_t i = 0; i < n; i++) {
        if (c < 1.0f) {
            k += flag;
            c = c + (flag == 0 && old ? old_h : a);
            if (flag == 0) old = false;
            flag ^= 1u;
        }
        c = c - 1.0f;
    }
    return k;
}

static void check_bound() {
    const float advances[] = {1.0f, 1.0000001f, 1.025f, 1.125f, 1.5f, 2.0f, 2.4999f, 3.75f, 17.3f, 127.9f};
    CHECK(max_symbols(0, 1.0) == 0 && max_symbols(1, 1.0) == 2 && max_symbols(20000, 1.0) == 10002);
    for (float a : advances) {
        bool below = false;
        for (uint64_t n = 0; n <= 700; n++) {
            const uint64_t bound = max_symbols(n, (double)a);
            CHECK(bound <= n / 2 + 2);  // (never above what the structure allows, one strobe per sample, plus the edges)
            for (int s = 0; s < 16; s++)
                for (uint32_t flag = 0; flag < 2; flag++) {
                    CHECK(densest(n, a, (float)s / 16.0f, flag, &below) <= bound);
                    // (set_params from the densest loop there is, h = 1, to this one)
                    CHECK(densest_after_exchange(n, a, 1.0f, (float)s / 16.0f, flag) <= bound);
                }
        }
        CHECK(!below);
    }
}

static void check_validation() {
    const float good[4] = {5.0f, 0.01f, 0.1f, 0.002f};
    CHECK(check_params(good) == nullptr);
    const Derived d = derive(good);
    CHECK(d.h0 == 2.5f && d.loop.hmin == (float)(2.5 * (1.0 - (double)0.01f)) && d.loop.hmax == (float)(2.5 * (1.0 + (double)0.01f)));
    CHECK(d.loop.g_mu == 0.1f && d.loop.g_omega == 0.002f);
    struct Edge {
        float q[4];
        bool ok;
    };
    const Edge edges[] = {
        {{2.0f, 0.0f, 0.0f, 0.0f}, false},        {{nextafterf(2.0f, 3.0f), 0.0f, 0.0f, 0.0f}, true},
        {{256.0f, 0.0f, 0.0f, 0.0f}, true},       {{nextafterf(256.0f, 300.0f), 0.0f, 0.0f, 0.0f}, false},
        {{5.0f, 0.25f, 0.0f, 0.0f}, true},        {{5.0f, nextafterf(0.25f, 1.0f), 0.0f, 0.0f}, false},
        {{5.0f, -1e-9f, 0.0f, 0.0f}, false},      {{5.0f, 0.0f, -1e-9f, 0.0f}, false},
        {{5.0f, 0.0f, 0.0f, -1e-9f}, false},      {{5.0f, 0.0f, 1.5f, 0.0f}, true},
        {{5.0f, 0.0f, nextafterf(1.5f, 2.0f), 0.0f}, false}, {{2.25f, 0.0f, 0.125f, 0.0f}, true},
        // hmin - g_mu = 1 - 2^-24, one ulp under 1: refused; 1 - 2^-26 rounds to 1 in float32, as the kernel's own
        // fmaf(g_mu, -1, hmin) does: accepted
        {{2.25f, 0.0f, 0.125f + 0x1p-24f, 0.0f}, false}, {{2.25f, 0.0f, nextafterf(0.125f, 1.0f), 0.0f}, true},
        {{3.0f, 0.25f, 0.125f, 9.0f}, true},
        {{NAN, 0.0f, 0.0f, 0.0f}, false},         {{5.0f, INFINITY, 0.0f, 0.0f}, false},
        {{5.0f, 0.0f, 0.0f, INFINITY}, false},    {{5.0f, 0.0f, NAN, 0.0f}, false},
    };
    for (const Edge &e : edges) CHECK((check_params(e.q) == nullptr) == e.ok);
}

// sync_idle is sync_step where the sample holds no strobe: every state word equal, for counters from 1 up, a NaN and an
// infinite one, real and complex rows
template <int PL> static void check_idle() {
    const hz::sm::Loop loop{0.11f, 0.0017f, 2.475f, 2.525f};
    const float counters[] = {1.0f, 1.0000001f, 1.5f, 2.25f, 63.0f, NAN, INFINITY};
    uint32_t seed = 12345u + PL;
    auto next = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (float)(int32_t)(seed >> 8 & 0xffff) / 4096.0f - 8.0f;
    };
    for (float c : counters)
        for (uint32_t flag = 0; flag < 2; flag++)
            for (int trial = 0; trial < 50; trial++) {
                hz::sm::State<PL> a{};
                a.c = c, a.h = 2.5f, a.flag = flag;
                float x0[PL], y[PL];
                for (int p = 0; p < PL; p++) a.yp[p] = next(), a.ym[p] = next(), a.x1[p] = next(), a.x2[p] = next(), a.x3[p] = next(), x0[p] = next();
                hz::sm::State<PL> b = a;
                CHECK(!hz::sm::sync_step<PL>(a, loop, x0, y));
                hz::sm::sync_idle<PL>(b, x0);
                CHECK(memcmp(&a, &b, sizeof a) == 0);
            }
}

int main() {
    check_idle<1>();
    check_idle<2>();
    static_assert(kMaxRows == 8192 && kLanes == 64 && kParams == 4, "the limits of include/hzsdr_symsync.h");
    std::set<std::tuple<uint32_t, uint32_t>> done;
    size_t largest = 0;
    for (uint32_t R = 1; R <= kMaxRows; R++)
        for (int cplx = 0; cplx < 2; cplx++) {
            const Geom g = symsync_geom(R, cplx != 0);
            CHECK(g.G >= 1 && g.G <= kMaxGroup && g.G == (R + 1023) / 1024 && g.P >= g.G && (g.P & 1) && g.T == 256 && g.K == kSteps);
            CHECK(g.planes == (cplx ? 2u : 1u) && g.Y == g.T / 2 + 1);
            CHECK(g.lds_bytes == ((size_t)g.planes * g.T * g.P + (size_t)g.planes * g.Y * g.P) * 4);
            CHECK(g.lds_bytes < kLdsOwn && kLdsOwn <= kLdsBudget);
            if (g.lds_bytes > largest) largest = g.lds_bytes;
            check_rows(g, R);
            CHECK(state_floats(R, g.planes) == (size_t)R * (cplx ? 13 : 8) && state_row_floats(g.planes) == (cplx ? 13u : 8u));
            for (uint32_t r : {0u, R / 2, R - 1}) {
                size_t want = (size_t)r * state_row_floats(g.planes);
                for (uint32_t e = kStC; e <= kStX3; e++)
                    for (uint32_t p = 0; p < (e < 3 ? 1u : g.planes); p++) CHECK(state_index(r, e, p, g.planes) == want++);
            }
            if (done.insert({g.G, g.planes}).second) check_geometry(g);
        }
    check_tile_symbols();
    check_bound();
    check_validation();
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("symsync_plan ok\n");
    return 0;
}
