// tuner_plan.cpp -- csrc/hz_tuner_plan.h under AddressSanitizer + UndefinedBehaviorSanitizer, checked against
// expectations computed with Python's big integers (tests/test_tuner_plan.py writes them to the file named on the
// command line):
//   C D Q n m rel                          a stream position to start from
//   P n_in ok count n m rel held flush     a push: the step's result, the held samples and the flush count behind it
//   W w D                                  a tuner: its phase step; the running word starts from the position's m
//   A count word                           the running word behind a push of `count` outputs
//   B T cq tile chunk lo                   the window base of a tile's chunk (offset by 2^62 to stay unsigned)
//   G K D Q                                prints "form: K D Q T tile_rows cq chunks window J plane bytes row_tiles"
// Beside them, with no expectation needed:
//   - for every D <= 256 and every Q <= 1024: the geometry's identities, the LDS request inside the budget, the tile the
//     largest that is, the chunk the largest that is, chunks * cq covering Qp; the plane pitch 16 modulo 32;
//   - for every D and a spread of Q: the reciprocal of D exact on the window's range; the layout a bijection of the
//     window into a plane; the kernel's stepped slot (two samples down per k-step) equal to transposed_slot for every lane
//     and both column tiles; the banks of every B-operand read (32 lanes: 16 of the re plane, 16 of the im plane) all
//     distinct;
//   - for a spread of K and Q: tuner_a_index a bijection of (row, j) onto [0, a_floats), and the 64 values of one row
//     tile and k-step in lane order.
// Prints "largest lds: D Q bytes", "chunked: <count of (D, Q)>" and "tuner_plan ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "hz_tuner_plan.h"

using namespace hz::tp;

static int failures = 0;
static long lineno = 0;
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

static void check_layout(uint32_t D, uint32_t Q) {
    const Geom g = tuner_geom(1, D, Q);
    const uint64_t magic = hz::div_magic(D);
    std::vector<unsigned char> seen((size_t)D * g.J, 0);
    for (uint32_t w = 0; w < g.window; w++) {
        const uint32_t s = hz::transposed_slot(w, D, g.J);
        CHECK(s < D * g.J && s < g.plane && !seen[s], "D=%u Q=%u w=%u slot %u", D, Q, w, s);
        if (s < D * g.J) seen[s] = 1;
        const uint32_t j = hz::div_by_magic(w, magic);  // the kernel's store
        CHECK(j == w / D && (w - j * D) * g.J + j == s, "store w=%u", w);
    }
    // the kernel's walk: lane (n, kk) of the wave at outputs wo * 32, both column tiles, every k-step of a chunk
    const uint32_t dec = 2u % D, cdec = 2u / D, down = dec * g.J + cdec, wrap = D * g.J - 1u;
    for (uint32_t wo = 0; wo < g.waves_out; wo++) {
        uint32_t row[64], off[64];
        for (uint32_t l = 0; l < 64; l++) {
            const uint32_t w0 = (wo * 32 + (l & 15)) * D + (g.cq - 1) - (l >> 5);
            const uint32_t col = hz::div_by_magic(w0, magic);
            row[l] = w0 - col * D;
            off[l] = row[l] * g.J + col;
        }
        for (uint32_t s = 0; s < g.cq / 2; s++) {
            for (uint32_t half = 0; half < 64; half += 32) {
                for (uint32_t ct = 0; ct < 2; ct++) {
                    int banks[32] = {0};
                    for (uint32_t l = half; l < half + 32; l++) {
                        const uint32_t ml = wo * 32 + ct * 16 + (l & 15), q = 2 * s + (l >> 5);
                        const uint32_t w = ml * D + (g.cq - 1 - q);
                        CHECK(w < g.window && off[l] + 16 * ct == hz::transposed_slot(w, D, g.J), "D=%u Q=%u s=%u lane %u", D, Q, s, l);
                        const uint32_t addr = ((l >> 4) & 1u) * g.plane + off[l] + 16 * ct;
                        CHECK(addr < 2 * g.plane, "address %u", addr);
                        CHECK(++banks[addr % 32] == 1, "D=%u Q=%u s=%u: two lanes of a read on bank %u", D, Q, s, addr % 32);
                    }
                }
            }
            for (uint32_t l = 0; l < 64; l++) {
                if (row[l] < dec) row[l] += D, off[l] += wrap;
                row[l] -= dec, off[l] -= down;
            }
        }
    }
}

static void check_a(uint32_t K, uint32_t Q) {
    const Geom g = tuner_geom(K, 3, Q);
    CHECK(g.row_tiles % 2 == 0 && g.row_tiles * 16 >= 2 * K && g.row_tiles * 16 < 2 * K + 32, "row tiles %u", g.row_tiles);
    CHECK(g.a_floats == (size_t)g.row_tiles * g.steps * 64 && g.a_floats * 4 <= (4u << 20), "A of %zu floats", g.a_floats);
    std::vector<unsigned char> seen(g.a_floats, 0);
    for (uint32_t row = 0; row < g.row_tiles * 16; row++)
        for (uint32_t j = 0; j < 2 * g.Qp; j++) {
            const size_t i = tuner_a_index(row, j, g.steps);
            CHECK(i < g.a_floats && !seen[i], "K=%u Q=%u row %u j %u", K, Q, row, j);
            if (i < g.a_floats) seen[i] = 1;
            // lane l of the step's 64 holds A[l & 15][l >> 4] of the 16 x 4 block
            const size_t lane = i % 64, block = i / 64;
            CHECK(lane % 16 == row % 16 && lane / 16 == j % 4 && block == (size_t)(row / 16) * g.steps + j / 4, "lane order");
        }
    for (size_t i = 0; i < g.a_floats; i++) CHECK(seen[i], "A index %zu is not reached", i);
}

int main(int argc, char **argv) {
    size_t largest = 0;
    uint32_t ld = 0, lq = 0;
    long chunked = 0;
    for (uint32_t D = 1; D <= kMaxDown; D++) {
        const uint64_t magic = hz::div_magic(D);
        for (uint32_t w = 0; w < kDivRange; w += D) {
            CHECK(hz::div_by_magic(w, magic) == w / D, "D=%u w=%u", D, w);
            if (w) CHECK(hz::div_by_magic(w - 1, magic) == (w - 1) / D, "D=%u w=%u", D, w - 1);
        }
        for (uint32_t Q = 1; Q <= kMaxTaps; Q++) {
            const Geom g = tuner_geom(7, D, Q);
            CHECK(g.Qp == Q + Q % 2 && g.steps * 2 == g.Qp, "Qp %u", g.Qp);
            CHECK(g.T == 128 || g.T == 64 || g.T == 32, "T %u", g.T);
            CHECK(g.waves_out * 32 == g.T && g.tile_rows * g.waves_out == 128, "waves %u rows %u", g.waves_out, g.tile_rows);
            CHECK(g.cq >= 2 && g.cq % 2 == 0 && g.cq <= g.Qp && g.chunks == (g.Qp + g.cq - 1) / g.cq, "cq %u chunks %u", g.cq, g.chunks);
            CHECK(g.chunks == 1 ? g.cq == g.Qp : g.T == 32, "D=%u Q=%u: chunked at T %u", D, Q, g.T);
            CHECK(g.window == (g.T - 1) * D + g.cq && g.window < kDivRange, "window %u", g.window);
            CHECK((uint64_t)g.J * D >= g.window && g.plane >= D * g.J && g.plane < D * g.J + 32 && g.plane % 32 == 16, "J %u plane %u", g.J,
                  g.plane);
            CHECK(g.lds_bytes == (size_t)g.plane * 8 && g.lds_bytes <= (size_t)kLdsFloats * 4 && g.lds_bytes <= 66 * 1024, "D=%u Q=%u lds %zu", D,
                  Q, g.lds_bytes);
            CHECK(g.J == tuner_columns(D, g.window), "J");
            if (g.T < 128) CHECK(tuner_columns(D, (2 * g.T - 1) * D + g.Qp) == 0, "D=%u Q=%u: T %u though %u fits", D, Q, g.T, 2 * g.T);
            if (g.chunks > 1) {
                CHECK(tuner_columns(D, (g.T - 1) * D + g.cq + 2) == 0, "D=%u Q=%u: cq %u though %u fits", D, Q, g.cq, g.cq + 2);
                chunked++;
            }
            if (g.lds_bytes > largest) largest = g.lds_bytes, ld = D, lq = Q;
            if (Q <= 2 || Q == kMaxTaps || Q == 129 || Q == 513 || Q == 1023) check_layout(D, Q);
        }
    }
    for (uint32_t K : {1u, 2u, 8u, 9u, 16u, 17u, 255u, 256u})
        for (uint32_t Q : {1u, 2u, 7u, 129u, 1023u, 1024u}) check_a(K, Q);
    printf("largest lds: %u %u %zu\n", ld, lq, largest);
    printf("chunked: %ld\n", chunked);
    if (argc < 2) {
        printf("usage: tuner_plan CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char line[512];
    State s{};
    uint32_t D = 1, Q = 1, step = 0, word = 0;
    long pushes = 0, words = 0, bases = 0;
    while (fgets(line, sizeof line, f)) {
        lineno++;
        unsigned long long a[10] = {0};
        if (line[0] == 'C') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4) == 5, "parse");
            D = (uint32_t)a[0], Q = (uint32_t)a[1];
            s.n = a[2], s.m = a[3], s.rel = (uint32_t)a[4];
        } else if (line[0] == 'G') {
            CHECK(sscanf(line + 1, "%llu %llu %llu", a, a + 1, a + 2) == 3, "parse");
            const Geom g = tuner_geom((uint32_t)a[0], (uint32_t)a[1], (uint32_t)a[2]);
            printf("form: %llu %llu %llu %u %u %u %u %u %u %u %zu %u\n", a[0], a[1], a[2], g.T, g.tile_rows, g.cq, g.chunks, g.window, g.J, g.plane,
                   g.lds_bytes, g.row_tiles);
        } else if (line[0] == 'W') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu", a, a + 1, a + 2, a + 3) == 4, "parse");
            CHECK((uint32_t)a[1] == D, "the tuner's D");
            step = phase_step((uint32_t)a[0], D);
            word = phase_at(step, s.m);
            CHECK(step == a[2] && word == a[3], "step %u word %u", step, word);
        } else if (line[0] == 'A') {
            CHECK(sscanf(line + 1, "%llu %llu", a, a + 1) == 2, "parse");
            word = phase_advance(word, step, a[0]);
            CHECK(word == a[1], "word %u", word);
            words++;
        } else if (line[0] == 'B') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4) == 5, "parse");
            const int64_t b = tuner_window_base(s.rel, D, (uint32_t)a[0], (uint32_t)a[1], a[2], (uint32_t)a[3]);
            CHECK((uint64_t)(b + ((int64_t)1 << 62)) == a[4], "base %" PRId64, b);
            bases++;
        } else if (line[0] == 'P') {
            CHECK(sscanf(line + 1, "%llu %llu %llu %llu %llu %llu %llu %llu", a, a + 1, a + 2, a + 3, a + 4, a + 5, a + 6, a + 7) == 8, "parse");
            const Step p = hz::dp::demod_step(s, D, Q, a[0]);
            CHECK(p.ok == (a[1] != 0), "ok %d", (int)p.ok);
            if (p.ok && a[1]) {
                CHECK(p.count == a[2], "count %" PRIu64, p.count);
                CHECK(p.next.n == a[3] && p.next.m == a[4], "n %" PRIu64 " m %" PRIu64, p.next.n, p.next.m);
                CHECK(p.next.rel == a[5], "rel %u", p.next.rel);
                const uint64_t held = p.next.n < tuner_held(Q) ? p.next.n : tuner_held(Q);
                CHECK(held == a[6], "held %" PRIu64, held);
                s = p.next;
                CHECK(hz::dp::demod_flush_count(s, D, Q) == a[7], "flush %" PRIu64, hz::dp::demod_flush_count(s, D, Q));
            }
            pushes++;
        }
    }
    fclose(f);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("tuner_plan ok: %ld pushes, %ld words, %ld bases\n", pushes, words, bases);
    return 0;
}
