// equalizer_plan.cpp -- csrc/hz_equalizer_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_equalizer_plan.py.  For every N = 1 ... 64, both kinds and R at the edges of the rows-per-wave steps:
//   - Np is N rounded up to a power of two, G = min(8, 64 / Np, ceil(R / 1024)), the waves' rows cover [0, R) exactly
//     once, in order, 1 ... G rows each; the LDS request holds the segments, the output tiles and the scratch one behind
//     the other and stays inside the family's budget ("geom:" lines, which the test recomputes);
// for every (G, Np, N, kind) that occurs, from the maps the kernel itself uses:
//   - every slot lies inside its region; the loader's slot of symbol t is the walk's slot of tap 0; the history's slot of
//     entry j is the walk's slot of tap j + 1 at the tile's first symbol; a tile's last N - 1 symbols, moved to the
//     front, are the next tile's history;
//   - the DISTINCT addresses per bank in each 32-lane group (lanes that read one address are served by one read) of the
//     walk's reads, of the first lanes' output writes, of the loader's writes and of the storer's reads are 1;
// the state's layout is a bijection onto (2 N - 1) planes floats; the validation at its edges.
// Prints "geom: R N complex G Np S lds" per geometry, "banks: G Np N planes walk out load store" per shape, "largest lds:
// bytes" and "equalizer_plan ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "hz_equalizer_plan.h"

using namespace hz::ep;
namespace em = hz::em;

static int failures = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            if (failures++ < 20) printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                               \
    } while (0)

// the largest number of distinct addresses of one 32-lane group that share a bank; slots[l] < 0: lane l is off
static uint32_t worst(const std::vector<int64_t> &slots) {
    uint32_t w = 0;
    for (size_t base = 0; base < slots.size(); base += 32) {
        std::set<int64_t> per[32];
        for (size_t l = base; l < base + 32 && l < slots.size(); l++)
            if (slots[l] >= 0) per[slots[l] % 32].insert(slots[l]);
        for (const auto &s : per)
            if (s.size() > w) w = (uint32_t)s.size();
    }
    return w;
}

static void check_rows(const Geom &g, uint32_t R) {
    uint32_t next = 0;
    CHECK(g.waves == (R + g.G - 1) / g.G);
    for (uint32_t w = 0; w < g.waves; w++) {
        const uint32_t c = wave_row_count(w, g.G, R);
        CHECK(wave_first_row(w, g.G) == next && c >= 1 && c <= g.G);
        next += c;
    }
    CHECK(next == R && wave_row_count(g.waves, g.G, R) == 0);
}

static void check_maps(const Geom &g) {
    const uint32_t N = g.N, floats = (uint32_t)(g.lds_bytes / 4);
    uint32_t walk = 0, out = 0, load = 0, store = 0;
    CHECK(g.out_base == g.planes * g.G * g.S && g.xchg_base == g.out_base + (g.planes + 1) * g.G * kOutPitch && floats == g.xchg_base + g.planes * kLanes);
    CHECK(g.G * g.Np <= kLanes && g.S >= N - 1 + g.T && g.S % kLanes == g.Np % kLanes);
    for (uint32_t t = 0; t < g.T; t++) {
        CHECK(load_slot(t % kLanes, t / kLanes, N) == walk_slot(0, t, N));
        for (uint32_t p = 0; p < g.planes; p++) {
            std::vector<int64_t> reads(kLanes, -1), writes(kLanes, -1);
            for (uint32_t lane = 0; lane < g.G * g.Np; lane++) {
                const uint32_t r = lane_row(lane, g.Np), tap = lane_tap(lane, g.Np), s = walk_slot(tap, t, N);
                CHECK(r < g.G && tap < g.Np && s < N - 1 + g.T);
                reads[lane] = seg_slot(r, p, s, g.G, g.S);
                CHECK(reads[lane] < g.out_base);
                if (tap == 0) writes[lane] = out_slot(r, p, t, g.G, g.out_base);
            }
            const uint32_t a = worst(reads), b = worst(writes);
            walk = a > walk ? a : walk, out = b > out ? b : out;
        }
        std::vector<int64_t> writes(kLanes, -1);  // the track
        for (uint32_t r = 0; r < g.G; r++) {
            writes[r * g.Np] = out_slot(r, g.planes, t, g.G, g.out_base);
            CHECK(writes[r * g.Np] >= g.out_base && writes[r * g.Np] < g.xchg_base);
        }
        const uint32_t b = worst(writes);
        out = b > out ? b : out;
    }
    for (uint32_t j = 0; j + 1 < N; j++) {
        CHECK(history_slot(j, N) == walk_slot(j + 1, 0, N));
        // behind a tile of tn symbols slot s + tn moves to slot s: entry j of the new history is X[j] of the last symbol
        for (uint32_t tn : {1u, N - 1, g.T}) CHECK(history_slot(j, N) + tn == walk_slot(j, tn - 1, N));
    }
    std::set<uint32_t> seen;
    for (uint32_t p = 0; p <= g.planes; p++)
        for (uint32_t r = 0; r < g.G; r++)
            for (uint32_t k = 0; k < g.K; k++) {
                std::vector<int64_t> w(kLanes), s(kLanes);
                for (uint32_t lane = 0; lane < kLanes; lane++) {
                    w[lane] = p < g.planes ? (int64_t)seg_slot(r, p, load_slot(lane, k, N), g.G, g.S) : -1;
                    s[lane] = out_slot(r, p, lane + kLanes * k, g.G, g.out_base);
                    if (p < g.planes) CHECK(w[lane] < g.out_base && seen.insert((uint32_t)w[lane]).second);
                    CHECK(s[lane] >= g.out_base && s[lane] < g.xchg_base && seen.insert((uint32_t)s[lane]).second);
                }
                const uint32_t a = worst(w), b = worst(s);
                load = a > load ? a : load, store = b > store ? b : store;
            }
    // the state: taps, then the history, a bijection onto the row's floats
    std::set<uint32_t> words;
    for (uint32_t p = 0; p < g.planes; p++) {
        for (uint32_t i = 0; i < N; i++) CHECK(words.insert(state_tap(i, p, g.planes)).second && state_tap(i, p, g.planes) < N * g.planes);
        for (uint32_t j = 0; j + 1 < N; j++) CHECK(words.insert(state_history(j, p, N, g.planes)).second);
    }
    CHECK(words.size() == state_row_floats(N, g.planes) && *words.rbegin() == state_row_floats(N, g.planes) - 1);
    printf("banks: %u %u %u %u %u %u %u %u\n", g.G, g.Np, N, g.planes, walk, out, load, store);
}

static void check_validation() {
    const float lo = kLow, hi = kHigh, lo_dn = nextafterf(lo, 0.0f), hi_up = nextafterf(hi, INFINITY);
    struct Edge {
        float q[2];
        bool ok;
    };
    const Edge edges[] = {
        {{0.0f, lo}, true},   {{1.0f, hi}, true},         {{-0.0f, 1.0f}, true},   {{nextafterf(1.0f, 2.0f), 1.0f}, false}, {{-1e-45f, 1.0f}, false},
        {{0.5f, lo_dn}, false}, {{0.5f, hi_up}, false},   {{0.5f, 0.0f}, false},   {{0.5f, -1.0f}, false},                  {{NAN, 1.0f}, false},
        {{0.5f, NAN}, false}, {{INFINITY, 1.0f}, false}, {{0.5f, INFINITY}, false}, {{0.5f, -INFINITY}, false},
    };
    for (const Edge &e : edges) CHECK((check_params(e.q) == nullptr) == e.ok);
    const float q[2] = {0.25f, 3.0f};
    CHECK(derive(q).mu == 0.25f && derive(q).level == 3.0f);
    for (int cplx = 0; cplx < 2; cplx++) {
        CHECK(!check_geom(1, 0, em::kCma, cplx) && !check_geom(64, 63, em::kDdBpsk, cplx) && !check_geom(64, 0, em::kCma, cplx));
        CHECK(check_geom(0, 0, em::kCma, cplx) && check_geom(65, 0, em::kCma, cplx) && check_geom(8, 8, em::kCma, cplx) && check_geom(8, -1, em::kCma, cplx));
        CHECK(check_geom(8, 4, -1, cplx) && check_geom(8, 4, 3, cplx) && check_geom(-1, -1, em::kCma, cplx));
    }
    CHECK(!check_geom(8, 4, em::kDdQpsk, true) && check_geom(8, 4, em::kDdQpsk, false));
}

int main() {
    static_assert(kMaxRows == 8192 && kLanes == 64 && kParams == 2 && kRealF32 == 32 && kC64 == 1 && kMaxTaps == 64 && kTile == 256,
                  "the limits of include/hzsdr_equalizer.h");
    static_assert(sizeof(em::Loop) == 8, "two words per row on the device");
    std::set<std::tuple<uint32_t, uint32_t, uint32_t, int>> done;
    size_t largest = 0;
    std::vector<uint32_t> edges = {1, 2, 3, 64, 1000, kMaxRows - 1, kMaxRows};
    for (uint32_t k = 1; k < 8; k++)
        for (uint32_t d : {0u, 1u, 2u}) edges.push_back(1024 * k - 1 + d);
    for (uint32_t N = 1; N <= kMaxTaps; N++)
        for (int cplx = 0; cplx < 2; cplx++)
            for (uint32_t R : edges) {
                const Geom g = equalizer_geom(R, N, N / 2, cplx != 0);
                CHECK(g.N == N && g.c == N / 2 && g.Np >= N && (g.Np & (g.Np - 1)) == 0 && (g.Np == 1 || g.Np / 2 < N));
                CHECK(g.G >= 1 && g.G <= kMaxGroup && g.G * g.Np <= kLanes && g.T == 256 && g.K == kSteps && g.planes == 1u + cplx);
                CHECK(g.lds_bytes < kLdsBudget);
                if (g.lds_bytes > largest) largest = g.lds_bytes;
                check_rows(g, R);
                printf("geom: %u %u %d %u %u %u %zu\n", R, N, cplx, g.G, g.Np, g.S, g.lds_bytes);
                if (done.insert({g.G, g.Np, N, cplx}).second) check_maps(g);
            }
    check_validation();
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("equalizer_plan ok\n");
    return 0;
}
