// chanbank_plan.cpp -- the host arithmetic of the channel bank (csrc/hz_chanbank_plan.h) as a stand-alone program for
// the sanitizers (tests/test_chanbank_plan.py builds it with -fsanitize=address,undefined).
//
//   chanbank_plan SEED STREAMS
//
// For EVERY M in 2 .. 255: the tile against the stated LDS budget; both operand layouts as bijections onto their
// ranges; the fold's dealing of (frame, r) to (wave, lane, trip), the product's dealing of row tiles to waves and both
// register-to-output maps of the kernel, each covering every frame and channel of a tile exactly once; the position map
// as a permutation with position 0 at -floor(M / 2); the division by multiplication over its whole range.  For STREAMS
// random streams of random (M, P, D) from random positions (pushes up to 2^62 samples among them): the counts of every
// push against the closed form in 128-bit integers, and the first and last sample a tile's fold loads against the
// virtual buffer.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_chanbank_plan.h"

using namespace hz;
typedef unsigned __int128 u128;

static int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            if (fails++ < 20) {                  \
                fprintf(stdout, "FAIL %s: ", #cond); \
                fprintf(stdout, __VA_ARGS__);    \
                fprintf(stdout, "\n");           \
            }                                    \
        }                                        \
    } while (0)

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static void check_geometry(uint32_t M, size_t *largest, uint32_t *largest_m, int *a_lds_count, int tiles_seen[2]) {
    const cp::Geom g = cp::chanbank_geom(M);
    CHECK(g.M == M && g.Mp == M + M % 2 && g.steps * 4 == 2 * g.Mp, "M=%u", M);
    CHECK(g.T == 64 || g.T == 32, "M=%u T=%u", M, g.T);
    tiles_seen[g.T == 64 ? 0 : 1]++;
    CHECK(g.col_tiles * 16 == g.T && g.pitch == g.T + 1, "M=%u", M);
    CHECK(g.groups * cp::kGroupTiles == g.row_tiles, "M=%u", M);
    CHECK(g.row_tiles * 16 >= 2 * M && (g.row_tiles - cp::kGroupTiles) * 16 < 2 * M, "M=%u row_tiles=%u", M, g.row_tiles);
    CHECK(g.b_floats == 2 * g.Mp * g.pitch && g.a_floats == (size_t)g.row_tiles * 16 * 2 * g.Mp, "M=%u", M);
    // the budget: B always, A beside it where the form says so; the largest T that fits was taken
    CHECK(g.lds_bytes == (g.b_floats + (g.a_lds ? g.a_floats : 0)) * 4 && g.lds_bytes <= cp::kLdsFloats * 4, "M=%u lds=%zu", M, g.lds_bytes);
    CHECK(g.a_lds == (g.b_floats + g.a_floats <= cp::kLdsFloats), "M=%u", M);
    if (g.T < 64) CHECK(cp::chanbank_b_floats(g.Mp, 2 * g.T) > cp::kLdsFloats, "M=%u: a larger tile fits", M);
    if (g.lds_bytes > *largest) *largest = g.lds_bytes, *largest_m = M;
    *a_lds_count += g.a_lds;
    CHECK((1u << g.fold_shift) <= 64 && ((1u << g.fold_shift) >= g.Mp || g.fold_shift == 6) && (g.fold_shift == 1 || (1u << (g.fold_shift - 1)) < g.Mp),
          "M=%u fold_shift=%u", M, g.fold_shift);

    // A: a bijection of (row, j) onto [0, a_floats); the 64 lanes of one (row tile, k-step) contiguous
    std::vector<uint8_t> seen(g.a_floats, 0);
    for (uint32_t row = 0; row < g.row_tiles * 16; row++)
        for (uint32_t j = 0; j < 2 * g.Mp; j++) {
            const size_t i = cp::chanbank_a_index(row, j, g.steps);
            CHECK(i < g.a_floats, "M=%u A(%u, %u) at %zu", M, row, j, i);
            if (i < g.a_floats) seen[i]++;
            const uint32_t lane = (j % 4) * 16 + row % 16;
            CHECK(i == ((size_t)(row / 16) * g.steps + j / 4) * 64 + lane, "M=%u A lane order", M);
        }
    for (size_t i = 0; i < g.a_floats; i++) CHECK(seen[i] == 1, "M=%u A slot %zu taken %d times", M, i, seen[i]);
    // B: injective into [0, b_floats); (re, im) side by side; a half wave's read is 32 consecutive floats
    std::vector<uint8_t> bseen(g.b_floats, 0);
    for (uint32_t j = 0; j < 2 * g.Mp; j++)
        for (uint32_t f = 0; f < g.T; f++) {
            const uint32_t i = cp::chanbank_b_index(j, f, g.pitch);
            CHECK(i < g.b_floats, "M=%u B(%u, %u) at %u", M, j, f, i);
            if (i < g.b_floats) bseen[i]++;
            if (j % 2 == 0) CHECK(cp::chanbank_b_index(j + 1, f, g.pitch) == i + 1 && i % 2 == 0, "M=%u B pair", M);
        }
    size_t used = 0;
    for (uint32_t i = 0; i < g.b_floats; i++) {
        CHECK(bseen[i] <= 1, "M=%u B slot %u taken %d times", M, i, bseen[i]);
        used += bseen[i];
    }
    CHECK(used == (size_t)2 * g.Mp * g.T, "M=%u", M);
    for (uint32_t s = 0; s < g.steps; s++)
        for (uint32_t ct = 0; ct < g.col_tiles; ct++)
            for (uint32_t half = 0; half < 2; half++) {
                uint32_t banks[32] = {};
                for (uint32_t l = half * 32; l < half * 32 + 32; l++) banks[cp::chanbank_b_index(4 * s + (l >> 4), ct * 16 + (l & 15), g.pitch) % 32]++;
                for (uint32_t b = 0; b < 32; b++) CHECK(banks[b] == 1, "M=%u: a B read with a bank conflict", M);
            }

    // the fold's dealing: (wave, lane, trips) -> (fl, r), every pair of the tile exactly once
    std::vector<uint8_t> fseen((size_t)g.T * g.Mp, 0);
    const uint32_t fold_lanes = 1u << g.fold_shift, fold_frames = 64u >> g.fold_shift;
    for (uint32_t wave = 0; wave < cp::kWaves; wave++)
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t fl = wave * fold_frames + (lane >> g.fold_shift); fl < g.T; fl += cp::kWaves * fold_frames)
                for (uint32_t r = lane & (fold_lanes - 1); r < g.Mp; r += fold_lanes) fseen[(size_t)fl * g.Mp + r]++;
    for (size_t i = 0; i < fseen.size(); i++) CHECK(fseen[i] == 1, "M=%u: fold output %zu computed %d times", M, i, fseen[i]);

    // the product's dealing and both register-to-output maps: every (channel, frame) of the tile exactly once
    for (int layout = 0; layout < 2; layout++) {
        std::vector<uint8_t> oseen((size_t)M * g.T * 2, 0);
        std::vector<uint8_t> rows(g.row_tiles, 0);
        for (uint32_t wave = 0; wave < cp::kWaves; wave++)
            for (uint32_t grp = wave; grp < g.groups; grp += cp::kWaves)
                for (uint32_t i = 0; i < cp::kGroupTiles; i++) {
                    const uint32_t rt = grp * cp::kGroupTiles + i;
                    rows[rt]++;
                    for (uint32_t lane = 0; lane < 64; lane++)
                        for (uint32_t j = 0; j < g.col_tiles; j++)
                            for (uint32_t q = 0; q < 4; q++) {
                                const uint32_t n = lane & 15, kk = lane >> 4;
                                uint32_t k, f, c;
                                if (layout == 1) {  // channel-major: rows of D are rows of A, columns are frames
                                    k = rt * 8 + kk * 2 + q / 2, c = q % 2, f = j * 16 + n;
                                } else {  // frame-major: columns of D are rows of A, rows are frames
                                    k = rt * 8 + n / 2, c = n % 2, f = j * 16 + kk * 4 + q;
                                }
                                if (k < M) oseen[((size_t)k * g.T + f) * 2 + c]++;
                            }
                }
        for (uint32_t rt = 0; rt < g.row_tiles; rt++) CHECK(rows[rt] == 1, "M=%u: row tile %u dealt %d times", M, rt, rows[rt]);
        for (size_t i = 0; i < oseen.size(); i++) CHECK(oseen[i] == 1, "M=%u layout %d: output %zu written %d times", M, layout, i, oseen[i]);
    }

    // the position map
    std::vector<uint8_t> pseen(M, 0);
    for (uint32_t k = 0; k < M; k++) {
        CHECK(cp::chanbank_pos(k, M, false) == k, "M=%u", M);
        const uint32_t p = cp::chanbank_pos(k, M, true);
        CHECK(p < M && p == (k + M / 2) % M, "M=%u pos(%u) = %u", M, k, p);
        if (p < M) pseen[p]++;
        // ascending signed frequency: position p holds the signed channel p - floor(M / 2)
        const int signed_k = k > (M - 1) / 2 ? (int)k - (int)M : (int)k;
        CHECK((int)p - (int)(M / 2) == signed_k, "M=%u: channel %u at position %u", M, k, p);
    }
    for (uint32_t k = 0; k < M; k++) CHECK(pseen[k] == 1, "M=%u", M);

    // the division by multiplication, the rotation of a tile's frames and the load offsets
    const uint64_t magic = div_magic(M);
    for (uint32_t w = 0; w <= 254 + 63 * 255; w++) CHECK(div_by_magic(w, magic) == w / M, "M=%u w=%u", M, w);
    for (uint32_t s = 0; s < M; s++)
        for (uint32_t r = 0; r < M; r++) {
            const uint32_t o = cp::chanbank_offset(r, s, M);
            CHECK(o < M && (o + s) % M == r, "M=%u offset(%u, %u) = %u", M, r, s, o);
        }
}

static u128 frames_after(u128 n, uint32_t L, uint32_t D) { return n >= L ? (n - L) / D + 1 : 0; }

static void check_stream(int index) {
    const uint32_t M = 2 + (uint32_t)below(254);
    const uint32_t pick_p[] = {1, 2, 32, 1 + (uint32_t)below(32)}, P = pick_p[below(4)];
    const uint32_t pick_d[] = {1, M, 1 + (uint32_t)below(M)}, D = pick_d[below(3)];
    const uint32_t L = P * M;
    const cp::Geom g = cp::chanbank_geom(M);
    cp::State st{};
    u128 N = 0;  // samples pushed so far
    for (int push = 0; push < 16; push++) {
        const uint64_t pick_n[] = {0, 1, below(10), below(3 * (uint64_t)L + 1), below(100000), below((uint64_t)1 << 33), below((uint64_t)1 << 52),
                                   ((uint64_t)1 << 62) - below(3), ((uint64_t)1 << 62) + 1 + below(1000), ~(uint64_t)0 - below(3)};
        const uint64_t n = pick_n[index % 4 == 0 ? below(10) : below(5)];
        const cp::Step p = cp::chanbank_step(st, M, L, D, n);
        CHECK(p.ok == (n <= cp::kPushMax), "push of %llu", (unsigned long long)n);
        if (!p.ok) continue;
        const u128 f0 = frames_after(N, L, D), f1 = frames_after(N + n, L, D);
        CHECK((u128)p.F == f1 - f0 && (u128)p.V == (u128)st.held + n, "M=%u P=%u D=%u: frames of a push", M, P, D);
        CHECK((u128)p.next.held == N + n - f1 * D && p.next.held < L, "M=%u P=%u D=%u: held %llu", M, P, D, (unsigned long long)p.next.held);
        CHECK((u128)p.next.rot == f1 * D % M, "M=%u P=%u D=%u: rotation", M, P, D);
        CHECK((u128)p.next.frame == (f1 & (u128) ~(uint64_t)0), "M=%u P=%u D=%u: frame index", M, P, D);
        // the loads of the fold of a live frame: inside held ++ in
        if (p.F) {
            const uint64_t tiles = (p.F + g.T - 1) / g.T;
            const uint64_t pick_t[] = {0, tiles - 1, below(tiles)};
            for (uint64_t tile : pick_t) {
                const uint64_t fa = tile * g.T, fb = fa + g.T <= p.F ? fa + g.T - 1 : p.F - 1;
                CHECK(cp::chanbank_rot(st.rot, fa, D, M) == (uint32_t)((u128)(st.rot + (u128)fa * D) % M), "rotation of tile %llu", (unsigned long long)tile);
                CHECK((u128)cp::chanbank_rot(st.rot, fa, D, M) == (f0 + fa) * D % M, "rotation against the stream position");
                const u128 last = (u128)fb * D + (M - 1) + (u128)(P - 1) * M;
                CHECK(last < p.V && last < ((u128)1 << 63), "the last sample of tile %llu", (unsigned long long)tile);
            }
        }
        st = p.next;
        N += n;
    }
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: chanbank_plan SEED STREAMS\n");
        return 64;
    }
    rng_state = strtoull(argv[1], nullptr, 10);
    const int streams = atoi(argv[2]);
    size_t largest = 0;
    uint32_t largest_m = 0;
    int a_lds = 0, tiles_seen[2] = {0, 0};
    for (uint32_t M = cp::kMinChannels; M <= cp::kMaxChannels; M++) check_geometry(M, &largest, &largest_m, &a_lds, tiles_seen);
    for (int i = 0; i < streams; i++) check_stream(i);
    printf("largest lds: %u %zu\n", largest_m, largest);
    printf("a in lds: %d\n", a_lds);
    printf("tiles: %d %d\n", tiles_seen[0], tiles_seen[1]);
    for (uint32_t M : {2u, 3u, 7u, 8u, 12u, 16u, 17u, 64u, 100u, 128u, 255u}) {
        const cp::Geom g = cp::chanbank_geom(M);
        printf("form: %u %u %u %d %zu\n", M, g.T, g.row_tiles, (int)g.a_lds, g.lds_bytes);
    }
    if (fails) {
        printf("chanbank_plan: %d check(s) failed\n", fails);
        return 1;
    }
    printf("chanbank_plan ok\n");
    return 0;
}
