// bitring_plan.cpp -- the host arithmetic that the bit-ring banks share (csrc/hz_bitring_plan.h) as a stand-alone program,
// built with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_bitring_plan.py.  For every K from 1 to
// 8192 + 63:
//   - the ring: HW = ceil(K / 64), RW the smallest power of two that holds HW + kChunk + 1 words and at most 256,
//     c = 64 HW - K;
//   - the history's bytes there and back, from random words (the bits below c clear) and from random bytes (the pad bits
//     clear);
//   - the re-alignment: HW words of history, then m new bits written into the ring's slots tile by tile and chunk by
//     chunk as the kernels write them (a push's last word masked), then new history word j = the 64 ring bits from
//     64 j + m on, read through the slots by funnel shifts -- for m at every word and chunk edge against the
//     concatenation as a plain word array, which has no slots and overwrites nothing, and for one m in turn (every m up
//     to K = 256) through the ABI's bytes against the last K bits of the plain bit array.
// The dealing of rows to waves is one row per wave.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_bitring_plan.h"
#include "hz_framesync_math.h"

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

// bits (0 / 1 per entry), oldest first -> the ABI's bytes: bit k in byte k / 8, bit 7 - k % 8, pad bits 0
static std::vector<uint8_t> pack(const uint8_t *bits, uint32_t K) {
    std::vector<uint8_t> bytes((K + 7) / 8, 0);
    for (uint32_t k = 0; k < K; k++)
        if (bits[k]) bytes[k >> 3] |= (uint8_t)(0x80u >> (k & 7));
    return bytes;
}

// 64 bits from bit `at` of the plain word array `flat` on (words behind its end are 0)
static uint64_t plain_bits(const std::vector<uint64_t> &flat, uint64_t at) {
    const size_t w = (size_t)(at >> 6);
    const uint32_t sh = (uint32_t)at & 63u;
    const uint64_t lo = w < flat.size() ? flat[w] : 0, hi = w + 1 < flat.size() ? flat[w + 1] : 0;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// bits: K bits of history, then at least m new ones; hist: the history's words.  The ring against the concatenation as
// a plain word array, which has neither slots nor a chunk that overwrites the oldest words; bitwise: and the K bits of
// the new history, through the ABI's bytes, against the bit array itself.
static void realign(const br::Ring &g, const std::vector<uint8_t> &bits, const std::vector<uint64_t> &hist, uint32_t m, bool bitwise) {
    std::vector<uint64_t> ring(g.RW, 0xdeadbeefdeadbeefull), next(g.HW), flat(hist);
    for (uint32_t j = 0; j < g.HW; j++) ring[br::ring_slot(j, g.RW)] = hist[j];
    const uint32_t tiles = (m + 63) / 64;
    for (uint32_t t0 = 0; t0 < tiles; t0 += br::kChunk) {
        for (uint32_t t = t0; t < t0 + br::kChunk && t < tiles; t++) {
            const uint32_t tn = m - 64 * t < 64 ? m - 64 * t : 64;
            uint64_t w = 0;
            for (uint32_t l = 0; l < tn; l++) w |= (uint64_t)bits[g.K + 64 * t + l] << l;
            const uint32_t slot = br::ring_slot(br::tile_word(t, g.HW), g.RW);
            REQUIRE(slot < g.RW);
            ring[slot] = w;
            flat.push_back(w);
        }
    }
    for (uint32_t j = 0; j < g.HW; j++) {
        const uint64_t at = 64ull * j + m;
        const uint32_t w = (uint32_t)(at >> 6);
        next[j] = m ? fm::funnel(ring[br::ring_slot(w, g.RW)], ring[br::ring_slot(w + 1, g.RW)], (uint32_t)at & 63u) : hist[j];
        REQUIRE(next[j] == plain_bits(flat, at));
    }
    if (!bitwise) return;
    std::vector<uint8_t> got(br::history_bytes(g.K) + 1, 0xa5);
    br::history_to_bytes(next.data(), g, got.data());
    REQUIRE(got.back() == 0xa5);
    got.pop_back();
    REQUIRE(got == pack(bits.data() + m, g.K));  // the last K bits of the K + m
}

int main() {
    REQUIRE(br::kTileBits == 64 && br::kChunk == 16 && br::kMaxPush == 0x7ffffff0u && br::kRealF32 == 32 && br::kC64 == 1);
    for (uint32_t rows : {1u, 2u, 1024u, 1025u, 8192u}) {
        const br::Deal d = br::deal(rows);
        REQUIRE(d.G == 1 && d.waves == rows);
    }
    const uint32_t ms[] = {0, 1, 63, 64, 65, 64 * br::kChunk - 1, 64 * br::kChunk, 64 * br::kChunk + 1};
    uint32_t widest = 0;
    for (uint32_t K = 1; K <= 8192 + 63; K++) {
        const br::Ring g = br::ring(K);
        REQUIRE(g.K == K && g.HW == (K + 63) / 64 && g.c == 64 * g.HW - K && g.c < 64);
        REQUIRE((g.RW & (g.RW - 1)) == 0 && g.RW >= g.HW + br::kChunk + 1 && g.RW / 2 < g.HW + br::kChunk + 1 && g.RW <= 256);
        if (g.RW > widest) widest = g.RW;
        // words -> bytes -> words, the bits below c clear
        std::vector<uint64_t> x(g.HW), back(g.HW, ~0ull);
        for (auto &w : x) w = rng();
        x[0] &= ~fm::low_mask(g.c);
        std::vector<uint8_t> bytes(br::history_bytes(K) + 1, 0xa5);
        REQUIRE(br::history_bytes(K) == (K + 7) / 8);
        br::history_to_bytes(x.data(), g, bytes.data());
        REQUIRE(bytes.back() == 0xa5);
        if (K % 8) REQUIRE((bytes[bytes.size() - 2] & (0xffu >> (K % 8))) == 0);
        br::history_from_bytes(bytes.data(), g, back.data());
        REQUIRE(back == x);
        // bytes -> words -> bytes, the pad bits clear
        std::vector<uint8_t> y(br::history_bytes(K)), again(br::history_bytes(K), 0xa5);
        for (auto &b : y) b = (uint8_t)rng();
        if (K % 8) y.back() &= (uint8_t)~(0xffu >> (K % 8));
        br::history_from_bytes(y.data(), g, back.data());
        REQUIRE((back[0] & fm::low_mask(g.c)) == 0);
        br::history_to_bytes(back.data(), g, again.data());
        REQUIRE(again == y);
        // the re-alignment: every m against the plain word array, and one of them in turn bit by bit
        std::vector<uint8_t> bits(K + 64 * br::kChunk + 1);
        for (auto &b : bits) b = (uint8_t)(rng() & 1);
        br::history_from_bytes(pack(bits.data(), K).data(), g, back.data());
        for (uint32_t i = 0; i < 8; i++) realign(g, bits, back, ms[i], i == K % 8 || K <= 256);
    }
    REQUIRE(widest == 256);
    printf("widest ring: %u\n", widest);
    printf("bitring_plan ok\n");
    return 0;
}
