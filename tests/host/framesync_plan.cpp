// framesync_plan.cpp -- the host arithmetic of the frame sync bank (csrc/hz_framesync_plan.h, csrc/hz_framesync_math.h)
// as a stand-alone program, built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_framesync_plan.py:
//   - the geometry for every (W, P) at the bounds and for every shift c = 0 ... 63: K, HW, c, the ring a power of two that
//     holds the history, a chunk and one word more, the LDS request inside the family's budget;
//   - the ring walked as the kernel walks it -- the history in front, chunks of tile words written into their slots, the
//     window and the payload words of every completing bit read back by funnel shifts, the history re-aligned behind
//     every push -- against a bit-by-bit loop over the plain bit array, with pushes of every length modulo 64;
//   - the word forms against the bit forms: reverse_bits, diff_word, map_word, out_word, distance;
//   - the history's bytes there and back.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_framesync_math.h"
#include "hz_framesync_plan.h"

using namespace hz;

#define REQUIRE(c)                                                  \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                \
        }                                                           \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static size_t largest_lds = 0;
static bool shift_seen[64], pay_shift_seen[64];

// the stream `bits` (0 / 1 per entry) in pushes of `cut` bits through the ring; every window and payload against the array
static void walk(uint32_t W, uint32_t P, const std::vector<uint8_t> &bits, uint32_t cut) {
    const fp::Geom g = fp::geom(1, W, P);
    REQUIRE(g.K == W + P - 1 && g.HW == (g.K + 63) / 64 && g.c == 64 * g.HW - g.K && g.c < 64);
    REQUIRE((g.RW & (g.RW - 1)) == 0 && g.RW >= g.HW + fp::kChunk + 1 && g.RW < 2 * (g.HW + fp::kChunk + 1));
    REQUIRE(g.lds_bytes == (size_t)g.RW * 8 && g.lds_bytes <= fp::kLdsBudget && g.FB == (P + 7) / 8 && g.PW == (P + 63) / 64 && g.per == 3 + g.HW);
    if (g.lds_bytes > largest_lds) largest_lds = g.lds_bytes;
    std::vector<uint64_t> ring(g.RW, 0xdeadbeefdeadbeefull), hist(g.HW, 0);
    uint64_t bits0 = 0;
    while (bits0 < bits.size()) {
        const uint32_t m = (uint32_t)(bits.size() - bits0 < cut ? bits.size() - bits0 : cut), tiles = (m + 63) / 64;
        for (uint32_t j = 0; j < g.HW; j++) ring[fp::ring_slot(j, g.RW)] = hist[j];
        for (uint32_t t0 = 0; t0 < tiles; t0 += fp::kChunk) {
            for (uint32_t t = t0; t < t0 + fp::kChunk && t < tiles; t++) {
                uint64_t w = rng() << 1;  // (bits behind a partial tile's end are garbage)
                for (uint32_t l = 0; l < 64 && t * 64 + l < m; l++) w = (w & ~(1ull << l)) | ((uint64_t)bits[bits0 + t * 64 + l] << l);
                ring[fp::ring_slot(fp::tile_word(t, g.HW), g.RW)] = w;
            }
            for (uint32_t t = t0; t < t0 + fp::kChunk && t < tiles; t++) {
                for (uint32_t l = 0; l < 64 && t * 64 + l < m; l++) {
                    const uint64_t done = bits0 + (uint64_t)t * 64 + l;
                    if (done < g.K) continue;
                    const uint64_t at = fp::window_bit(t, l, g.c);
                    shift_seen[at & 63] = true;
                    const uint64_t x = fm::funnel(ring[fp::ring_slot((uint32_t)(at >> 6), g.RW)], ring[fp::ring_slot((uint32_t)(at >> 6) + 1, g.RW)], at & 63);
                    for (uint32_t k = 0; k < W; k++) REQUIRE(((x >> k) & 1) == bits[done - g.K + k]);
                    for (uint32_t j = 0; j < g.PW; j++) {
                        const uint64_t pa = at + W + 64ull * j;
                        pay_shift_seen[pa & 63] = true;
                        const uint64_t p = fm::funnel(ring[fp::ring_slot((uint32_t)(pa >> 6), g.RW)], ring[fp::ring_slot((uint32_t)(pa >> 6) + 1, g.RW)], pa & 63);
                        const uint32_t nb = P - 64 * j < 64 ? P - 64 * j : 64;
                        for (uint32_t k = 0; k < nb; k++) REQUIRE(((p >> k) & 1) == bits[done - P + 1 + 64 * j + k]);
                    }
                }
            }
        }
        if (m) {
            std::vector<uint64_t> next(g.HW);
            for (uint32_t j = 0; j < g.HW; j++) {
                const uint64_t at = 64ull * j + m;
                next[j] = fm::funnel(ring[fp::ring_slot((uint32_t)(at >> 6), g.RW)], ring[fp::ring_slot((uint32_t)(at >> 6) + 1, g.RW)], at & 63);
            }
            hist = next;
        }
        bits0 += m;
        // the history: the last 64 HW bits, the newest in bit 63 of the last word, zeros where the stream had not begun
        for (uint32_t k = 0; k < 64 * g.HW; k++) {
            const int64_t src = (int64_t)bits0 - 64 * (int64_t)g.HW + k;
            REQUIRE(((hist[k >> 6] >> (k & 63)) & 1) == (src < 0 ? 0u : bits[src]));
        }
        std::vector<uint8_t> bytes(fp::history_bytes(g.K) + 1, 0xa5);
        std::vector<uint64_t> back(g.HW, ~0ull);
        fp::history_to_bytes(hist.data(), g, bytes.data());
        REQUIRE(bytes.back() == 0xa5);
        for (uint32_t k = 0; k < g.K; k++) {
            const int64_t src = (int64_t)bits0 - (int64_t)g.K + k;
            REQUIRE((uint32_t)((bytes[k >> 3] >> (7 - (k & 7))) & 1) == (src < 0 ? 0u : bits[src]));
        }
        fp::history_from_bytes(bytes.data(), g, back.data());
        for (uint32_t j = 0; j < g.HW; j++) REQUIRE(back[j] == (j == 0 ? hist[0] & ~fm::low_mask(g.c) : hist[j]));
    }
}

static void word_forms() {
    for (uint32_t W = 1; W <= 64; W++) {
        const uint64_t v = rng() & fm::low_mask(W), r = fm::reverse_bits(v, W);
        for (uint32_t k = 0; k < W; k++) REQUIRE(((r >> k) & 1) == ((v >> (W - 1 - k)) & 1));
        REQUIRE(fm::reverse_bits(r, W) == v && (r & ~fm::low_mask(W)) == 0);
    }
    REQUIRE(fm::reverse_bits(1, 64) == 1ull << 63 && fm::low_mask(0) == 0 && fm::low_mask(64) == ~0ull && fm::low_mask(63) == ~0ull >> 1);
    for (int trial = 0; trial < 200; trial++) {
        const uint64_t raw = rng(), other = rng(), mask = rng() & rng();
        const uint32_t carry = (uint32_t)rng() & 1u;
        for (int diff = 0; diff < 3; diff++) {
            const uint64_t w = fm::diff_word(raw, carry, diff);
            for (uint32_t k = 0; k < 64; k++)
                REQUIRE(((w >> k) & 1) == fm::diff_bit((uint32_t)(raw >> k) & 1u, k ? (uint32_t)(raw >> (k - 1)) & 1u : carry, diff));
        }
        for (int map = 0; map < 2; map++) {
            const uint64_t y = fm::map_word(raw, map, false);
            for (uint32_t k = 0; k < 64; k++) REQUIRE(((y >> k) & 1) == fm::map_bit((uint32_t)(raw >> k) & 1u, map));
        }
        for (int q = 0; q < 4; q++) {
            const uint64_t y = fm::map_word(raw, q, true);
            for (uint32_t k = 0; k < 64; k += 2) REQUIRE(((y >> k) & 3) == fm::map_dibit((uint32_t)(raw >> k) & 3u, q));
        }
        const uint64_t y = fm::out_word(raw);
        for (uint32_t k = 0; k < 64; k++) REQUIRE(((y >> (8 * (k / 8) + 7 - k % 8)) & 1) == ((raw >> k) & 1));
        uint32_t dist = 0;
        for (uint32_t k = 0; k < 64; k++) dist += (uint32_t)((mask >> k) & ((raw ^ other) >> k) & 1);
        REQUIRE(fm::distance(raw, other, mask) == dist);
    }
    // four quarter turns are a full one; map q undoes a rotation by i^q: (b0, b1) of x i is (!b1, b0)
    for (uint32_t d = 0; d < 4; d++) {
        uint32_t turned = d;
        for (int q = 0; q < 4; q++) {
            REQUIRE(fm::map_dibit(turned, q) == d);
            const uint32_t b0 = turned & 1u, b1 = turned >> 1;
            turned = (b1 ^ 1u) | (b0 << 1);
        }
        REQUIRE(turned == d);
    }
    REQUIRE(fm::decide(0x00000000u) == 1 && fm::decide(0x80000000u) == 0 && fm::decide(0x7fc00000u) == 1 && fm::decide(0xffc00000u) == 0 &&
            fm::decide(0x7f800000u) == 1 && fm::decide(0xff800000u) == 0);
}

int main() {
    word_forms();
    const uint32_t Ws[] = {1, 2, 7, 8, 24, 32, 63, 64}, Ps[] = {1, 2, 8, 13, 63, 64, 65, 127, 128, 129, 168, 1000};
    for (uint32_t W : Ws)
        for (uint32_t P : Ps) {
            std::vector<uint8_t> bits(3 * (W + P) + 700);
            for (auto &b : bits) b = (uint8_t)(rng() & 1);
            const uint32_t cuts[] = {1, 63, 64, 65, 300, (uint32_t)bits.size(), 64 * fp::kChunk, 64 * fp::kChunk + 1};
            for (uint32_t cut : cuts)
                if (cut > 1 || P < 100) walk(W, P, bits, cut);
        }
    for (uint32_t P = 1; P <= 130; P++) {  // every shift c
        std::vector<uint8_t> bits(900);
        for (auto &b : bits) b = (uint8_t)(rng() & 1);
        walk(32, P, bits, 257);
    }
    for (uint32_t W : {1u, 64u})
        for (uint32_t P : {8191u, 8192u}) {
            if (W == 1 && P == 8191) continue;
            std::vector<uint8_t> bits(2 * 8300);
            for (auto &b : bits) b = (uint8_t)(rng() & 1);
            walk(W, P, bits, 5000);
        }
    for (int k = 0; k < 64; k++) REQUIRE(shift_seen[k] && pay_shift_seen[k]);
    // validation at the bounds (the rest is restated in Python against the program of framesync_ref.cpp)
    fp::Config q{fp::kC64, 2, 64, ~0ull, 63, 4, {1, 2, 3, 4}, {0, 1, 2, 3}, 8192, 0, fp::kMaxHoldoff};
    REQUIRE(fp::check_config(q) == nullptr);
    q.thr = 64;
    REQUIRE(fp::check_config(q) != nullptr);
    const fp::Geom big = fp::geom(8192, 64, 8192);
    REQUIRE(big.G == 1 && big.waves == 8192 && big.HW == 129 && big.RW == 256);
    printf("largest lds: %zu\n", largest_lds);
    printf("framesync_plan ok\n");
    return 0;
}
