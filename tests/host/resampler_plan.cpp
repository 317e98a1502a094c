// resampler_plan.cpp -- csrc/hz_resampler_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer, checked against
// expectations computed with Python's big integers (tests/test_resampler_plan.py writes them to the file named on the
// command line):
//   C U D Q L n m phi rel                  a stream position to start from
//   T t tile i0 phi lo hi                  tile `tile` of t outputs of the NEXT push: resampler_tile's i0 and phi, and
//                                          the first and last sample index (relative, lo offset by Q - 1 to stay
//                                          unsigned) its outputs read
//   P n_in ok count n m phi rel held flush a push: resampler_step's result and the flush count behind it
// Beside them, with no expectation needed: every output of a tile gets the (i, phi) that a 64-bit division gives from
// the kernel's lane arithmetic (reciprocal, then add-and-carry), and the reciprocal is exact on its whole range.
// A search of every (U, D, Q) a create accepts for the largest LDS request among the forms with a window prints
// "largest lds: U D Q window bytes" (the loops nest U, Q, D: the first shape in that order to reach the maximum), and
// the forms of the shapes named by "G U D Q" lines print as "form: U D Q T direct global uniform pad bytes".
// Prints "resampler_plan ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "hz_resampler_plan.h"

using namespace hz::rs;

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (failures++ < 20) {                            \
                printf("FAIL line %ld: %s: ", lineno, #cond); \
                printf(__VA_ARGS__);                          \
                printf("\n");                                 \
            }                                                 \
        }                                                     \
    } while (0)

// the kernel's lane arithmetic for every output of a tile against plain 64-bit division
static void lanes(long lineno, const State &s, uint32_t U, uint32_t D, uint32_t Q, const Geom &g, uint64_t tile) {
    const Tile t = resampler_tile(s.rel, s.phi, U, D, Q, g.T, tile);
    const uint64_t magic = hz::div_magic(U);
    const uint64_t base = (uint64_t)s.rel * U + s.phi + tile * ((uint64_t)g.T * D);
    for (uint32_t tid = 0; tid < (uint32_t)kThreads; tid++) {
        const uint32_t u = t.phi + tid * D;
        CHECK(u < kDivRange, "u=%u", u);
        uint32_t i = hz::div_by_magic(u, magic), phi = u - i * U;
        for (uint32_t r = 0; r < g.T / kThreads; r++) {
            const uint64_t tt = base + (uint64_t)(tid + r * kThreads) * D;
            CHECK(phi < U && tt / U == t.i0 + i && tt % U == phi, "U=%u D=%u tid=%u r=%u", U, D, tid, r);
            CHECK(g.direct || i + Q <= t.window, "window %u, index %u", t.window, i + Q - 1);
            i += g.step_i;
            phi += g.step_phi;
            if (phi >= U) {
                phi -= U;
                i++;
            }
        }
    }
}

int main(int argc, char **argv) {
    long lineno = 0;
    // the reciprocal: floor(u / U) can only first go wrong just below or at a multiple of U
    for (uint32_t U = 1; U <= kMaxRate; U++) {
        const uint64_t magic = hz::div_magic(U);
        for (uint32_t u = 0; u < kDivRange; u += U) {
            CHECK(hz::div_by_magic(u, magic) == u / U, "U=%u u=%u", U, u);
            if (u) CHECK(hz::div_by_magic(u - 1, magic) == (u - 1) / U, "U=%u u=%u", U, u - 1);
        }
        CHECK(hz::div_by_magic(kDivRange - 1, magic) == (kDivRange - 1) / U, "U=%u", U);
        // every shape's offsets stay inside that range, its LDS inside the budget
        for (uint32_t D = 1; D <= kMaxRate; D += (U % 7 == 0 ? 1 : 61))
            for (uint32_t Q : {1u, 2u, 7u, 64u, 256u}) {
                const Geom g = resampler_geom(U, D, Q);
                CHECK(U - 1 + (uint64_t)(g.T - 1) * D < kDivRange, "U=%u D=%u", U, D);
                CHECK((uint64_t)g.step_i * U + g.step_phi == (uint64_t)kThreads * D && g.step_phi < U, "U=%u D=%u", U, D);
                CHECK(g.pitch >= Q && g.pitch % 4 == 0 && (g.pitch / 4) % 2 == 1, "pitch %u", g.pitch);
                CHECK(g.lds_bytes <= (size_t)(kWindowMax + kWindowMax / 32 + 1) * 8 + (size_t)kTableMax * 4 && g.lds_bytes <= 80 * 1024, "lds %zu", g.lds_bytes);
                CHECK(g.pad == (!g.direct && D >= 2 * U), "pad");
                CHECK(g.taps_uniform == (!g.direct && !g.taps_global && D % U == 0), "uniform");
                if (g.window) CHECK(g.lds_bytes >= (size_t)(resampler_slot(g.window - 1, g.pad) + 1) * 8, "lds %zu", g.lds_bytes);
                CHECK(g.direct ? g.window == 0 : g.window == (U - 1 + (g.T - 1) * D) / U + Q && g.window <= kWindowMax, "window %u", g.window);
                CHECK(g.taps_global == ((uint64_t)U * g.pitch > kTableMax), "U=%u Q=%u", U, Q);
            }
    }
    // the largest LDS request of a form with a window, over every shape a create accepts (Q taps per phase need at
    // least (Q - 1) U + 1 taps in all): the GPU tests run the shape this prints
    {
        Geom best{};
        uint32_t bu = 0, bd = 0, bq = 0;
        for (uint32_t U = 1; U <= kMaxRate; U++)
            for (uint32_t Q = 1; Q <= kMaxPhaseTaps && (uint64_t)(Q - 1) * U + 1 <= kMaxTaps; Q++)
                for (uint32_t D = 1; D <= kMaxRate; D++) {
                    const Geom g = resampler_geom(U, D, Q);
                    if (!g.direct && g.lds_bytes > best.lds_bytes) best = g, bu = U, bd = D, bq = Q;
                }
        CHECK(best.lds_bytes <= (size_t)(kWindowMax + kWindowMax / 32 + 1) * 8 + (size_t)kTableMax * 4, "lds %zu", best.lds_bytes);
        printf("largest lds: %u %u %u %u %zu\n", bu, bd, bq, best.window, best.lds_bytes);
    }
    if (argc < 2) {
        printf("usage: resampler_plan CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char line[512];
    State s{};
    uint32_t U = 1, D = 1, Q = 1, L = 1;
    long pushes = 0, tiles = 0;
    while (fgets(line, sizeof line, f)) {
        lineno++;
        unsigned long long a[10] = {0};
        if (line[0] == 'C') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) == 8, "parse");
            U = (uint32_t)a[0], D = (uint32_t)a[1], Q = (uint32_t)a[2], L = (uint32_t)a[3];
            s.n = a[4], s.m = a[5], s.phi = (uint32_t)a[6], s.rel = (uint32_t)a[7];
        } else if (line[0] == 'G') {
            CHECK(sscanf(line + 1, "%llu %llu %llu", a, a + 1, a + 2) == 3, "parse");
            const Geom g = resampler_geom((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
            printf("form: %llu %llu %llu %u %d %d %d %d %zu\n", a[0], a[1], a[2], g.T, (int)g.direct, (int)g.taps_global, (int)g.taps_uniform,
                   (int)g.pad, g.lds_bytes);
        } else if (line[0] == 'T') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4, a + 5) == 6, "parse");
            const Tile t = resampler_tile(s.rel, s.phi, U, D, Q, (uint32_t)a[0], a[1]);
            CHECK(t.i0 == a[2] && t.phi == a[3], "tile %llu: i0 %" PRIu64 " phi %u", a[1], t.i0, t.phi);
            // the window covers exactly the samples the tile's outputs read: [i0 - (Q - 1), i0 - (Q - 1) + window)
            CHECK(t.i0 == a[4] && t.i0 + t.window - 1 == a[5], "tile %llu: window %u from %" PRIu64, a[1], t.window, t.i0);
            const Geom g = resampler_geom(U, D, Q);
            if (g.T == a[0]) lanes(lineno, s, U, D, Q, g, a[1]);
            tiles++;
        } else if (line[0] == 'P') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7, a + 8) == 9, "parse");
            const Step p = resampler_step(s, U, D, Q, a[0]);
            CHECK(p.ok == (a[1] != 0), "ok %d", (int)p.ok);
            if (p.ok && a[1]) {
                CHECK(p.count == a[2], "count %" PRIu64, p.count);
                CHECK(p.next.n == a[3] && p.next.m == a[4], "n %" PRIu64 " m %" PRIu64, p.next.n, p.next.m);
                CHECK(p.next.phi == a[5] && p.next.rel == a[6], "phi %u rel %u", p.next.phi, p.next.rel);
                CHECK(p.held == a[7], "held %zu", p.held);
                s = p.next;
                CHECK(resampler_flush_count(s, U, D, L) == a[8], "flush %" PRIu64, resampler_flush_count(s, U, D, L));
            }
            pushes++;
        }
    }
    fclose(f);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("resampler_plan ok: %ld pushes, %ld tiles\n", pushes, tiles);
    return 0;
}
