// demod_plan.cpp -- csrc/hz_demod_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer, checked against
// expectations computed with Python's big integers (tests/test_demod_plan.py writes them to the file named on the
// command line):
//   C D Q n m rel                          a stream position to start from
//   T t tile i0 lo hi                      tile `tile` of t outputs of the NEXT push: demod_tile's i0, and the first and
//                                          last detector index (relative, lo offset by Q - 1 to stay unsigned) its
//                                          outputs read
//   P n_in ok count n m rel held flush     a push: demod_step's result and the flush count behind it
//   G D Q                                  prints "form: D Q T half window J bytes"
// Beside them, with no expectation needed, for every D <= 64 and a spread of Q (every Q for the LDS request):
//   - the LDS request is inside the budget, the tile the largest that is, and the layout is a bijection of the window
//     into it;
//   - the reciprocal of D is exact on the window's range;
//   - the kernel's stepped slot (from tap to tap: one row up, or from row 0 to the last row of the column before) is
//     transposed_slot of the window index, for every tap, the first and the last lane and chain;
//   - the lanes per bank of each 32-lane half of a read, for EVERY window base (every tap of every chain): the table
//     "banks: D worst" is printed, one line per D, and the condition is 1 for odd D and at most 2 for even D.
// Prints "demod_plan ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "hz_demod_plan.h"

using namespace hz::dp;

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

// the most lanes on one of the 32 banks (4 bytes wide) in a 32-lane half of a read at window base c
static int worst_bank(const Geom &g, uint32_t D, uint32_t c, uint32_t lanes) {
    int worst = 0;
    for (uint32_t half = 0; half < 64; half += 32) {
        int n[32] = {0};
        for (uint32_t l = half; l < half + 32 && l < lanes; l++) {
            const int v = ++n[hz::transposed_slot(l * D + c, D, g.J) % 32];
            if (v > worst) worst = v;
        }
    }
    return worst;
}

int main(int argc, char **argv) {
    long lineno = 0;
    size_t largest = 0;
    uint32_t ld = 0, lq = 0;
    for (uint32_t D = 1; D <= kMaxDown; D++) {
        const uint64_t magic = hz::div_magic(D);
        for (uint32_t w = 0; w < kDivRange; w += D) {
            CHECK(hz::div_by_magic(w, magic) == w / D, "D=%u w=%u", D, w);
            if (w) CHECK(hz::div_by_magic(w - 1, magic) == (w - 1) / D, "D=%u w=%u", D, w - 1);
        }
        int banks = 0;
        for (uint32_t Q = 1; Q <= kMaxTaps; Q++) {
            const Geom g = demod_geom(D, Q);
            CHECK(g.T == 1024 || g.T == 512 || g.T == 256 || g.T == 128, "T %u", g.T);
            CHECK(g.half == (g.T == 128), "half");
            CHECK(g.window == (g.T - 1) * D + Q && g.window < kDivRange, "window %u", g.window);
            CHECK(g.J % 2 == 1 && (uint64_t)g.J * D >= g.window, "J %u", g.J);
            CHECK(g.lds_bytes == (size_t)D * g.J * 4 && g.lds_bytes <= (size_t)kWindowMax * 4 && g.lds_bytes <= 66 * 1024, "D=%u Q=%u lds %zu", D,
                  Q, g.lds_bytes);
            if (g.T < 1024) {  // the next larger tile does not fit
                const uint32_t w2 = (2 * g.T - 1) * D + Q, j2 = ((w2 + D - 1) / D) | 1u;
                CHECK(D * j2 > kWindowMax, "D=%u Q=%u: T %u though %u fits", D, Q, g.T, 2 * g.T);
            }
            CHECK(g.row0 == (Q - 1) % D && g.slot0 == hz::transposed_slot(Q - 1, D, g.J), "slot0");
            if (g.lds_bytes > largest) largest = g.lds_bytes, ld = D, lq = Q;
            if (!(Q <= 9 || Q % 97 == 0 || Q == kMaxTaps || Q == 129 || Q == 513 || Q == 757)) continue;
            // a bijection into the request
            std::vector<unsigned char> seen((size_t)D * g.J, 0);
            for (uint32_t w = 0; w < g.window; w++) {
                const uint32_t s = hz::transposed_slot(w, D, g.J);
                CHECK(s < D * g.J && !seen[s], "D=%u Q=%u w=%u slot %u", D, Q, w, s);
                if (s < D * g.J) seen[s] = 1;
                const uint32_t j = hz::div_by_magic(w, magic);  // the kernel's store
                CHECK((w - j * D) * g.J + j == s, "store w=%u", w);
            }
            // the stepped slot, and the banks of every read
            const uint32_t lanes = g.half ? g.T : (uint32_t)kThreads, chains = g.half ? 1 : g.T / kThreads;
            uint32_t row = g.row0, off = g.slot0;
            const uint32_t up = (D - 1) * g.J - 1;
            for (uint32_t q = 0; q < Q; q++) {
                for (uint32_t r = 0; r < chains; r++)
                    for (uint32_t tid : {0u, 31u, 32u, lanes - 1}) {
                        const uint32_t w = (tid + r * kThreads) * D + (Q - 1 - q);
                        CHECK(w < g.window && off + tid + r * kThreads == hz::transposed_slot(w, D, g.J), "D=%u Q=%u q=%u tid=%u r=%u", D, Q, q, tid, r);
                    }
                // (a wave's 64 lanes from any wave of any chain: the base c = wave's first output * D + Q - 1 - q)
                for (uint32_t first = 0; first < g.T; first += 64) {
                    const int b = worst_bank(g, D, first * D + (Q - 1 - q), 64);
                    if (b > banks) banks = b;
                }
                if (row == 0) {
                    row = D - 1;
                    off += up;
                } else {
                    row--;
                    off -= g.J;
                }
            }
        }
        printf("banks: %u %d\n", D, banks);
        CHECK(banks == 1 || (D % 2 == 0 && banks <= 2), "D=%u: %d lanes on a bank", D, banks);
    }
    printf("largest lds: %u %u %zu\n", ld, lq, largest);
    if (argc < 2) {
        printf("usage: demod_plan CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char line[512];
    State s{};
    uint32_t D = 1, Q = 1;
    long pushes = 0, tiles = 0;
    while (fgets(line, sizeof line, f)) {
        lineno++;
        unsigned long long a[10] = {0};
        if (line[0] == 'C') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4) == 5, "parse");
            D = (uint32_t)a[0], Q = (uint32_t)a[1];
            s.n = a[2], s.m = a[3], s.rel = (uint32_t)a[4];
        } else if (line[0] == 'G') {
            CHECK(sscanf(line + 1, "%llu %llu", a, a + 1) == 2, "parse");
            const Geom g = demod_geom((uint32_t)a[0], (uint32_t)a[1]);
            printf("form: %llu %llu %u %d %u %u %zu\n", a[0], a[1], g.T, (int)g.half, g.window, g.J, g.lds_bytes);
        } else if (line[0] == 'T') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4) == 5, "parse");
            const Tile t = demod_tile(s.rel, D, Q, (uint32_t)a[0], a[1]);
            CHECK(t.i0 == a[2], "tile %llu: i0 %" PRIu64, a[1], t.i0);
            // the window covers exactly the values the tile's outputs read: [i0 - (Q - 1), i0 - (Q - 1) + window)
            CHECK(t.i0 == a[3] && t.i0 + t.window - 1 == a[4], "tile %llu: window %u from %" PRIu64, a[1], t.window, t.i0);
            tiles++;
        } else if (line[0] == 'P') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) == 8, "parse");
            const Step p = demod_step(s, D, Q, a[0]);
            CHECK(p.ok == (a[1] != 0), "ok %d", (int)p.ok);
            if (p.ok && a[1]) {
                CHECK(p.count == a[2], "count %" PRIu64, p.count);
                CHECK(p.next.n == a[3] && p.next.m == a[4], "n %" PRIu64 " m %" PRIu64, p.next.n, p.next.m);
                CHECK(p.next.rel == a[5], "rel %u", p.next.rel);
                CHECK(p.held == a[6], "held %zu", p.held);
                s = p.next;
                CHECK(demod_flush_count(s, D, Q) == a[7], "flush %" PRIu64, demod_flush_count(s, D, Q));
            }
            pushes++;
        }
    }
    fclose(f);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demod_plan ok: %ld pushes, %ld tiles\n", pushes, tiles);
    return 0;
}
