// hdlc_plan.cpp -- the HDLC deframer bank's host arithmetic (csrc/hz_hdlc_plan.h, csrc/hz_hdlc_math.h) as a stand-alone
// program for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_hdlc_plan.py builds and runs it):
//   1. the validation over every combination of values at and around the bounds, against the bounds written out;
//   2. the geometry for every max_bytes: Lmax, K, the ring a power of two that holds the history, a chunk and one more
//      word, the frame buffer, the largest LDS request;
//   3. the word forms against the bit forms: stuffed_mask, delete_bits, fcs_word, the powers table and mulmod;
//   4. the state's history through history_to_bytes / history_from_bytes and back;
//   5. the WALK: random streams (noise, encoded traffic with aborts, shared zeros and long frames) pushed in random cuts
//      through a ring laid out and read exactly as the kernel does it, lane by lane -- windows and spans by funnel shifts,
//      stuffed masks across the word boundary, the scan of the kept counts, the pieces ORed into the frame buffer, the
//      FCS walked through the byte table (short frames) or combined from per-word registers through the powers table
//      (long ones), the history re-aligned behind each push -- with every slot
//      index checked against the ring's size, against a bit-serial decoder that keeps the whole stream.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_hdlc_math.h"
#include "hz_hdlc_plan.h"

using namespace hz;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                                      \
        }                                                                 \
    } while (0)

struct Frame {
    uint64_t from;
    uint32_t good;
    std::vector<uint8_t> bits;
    bool operator==(const Frame &o) const { return from == o.from && good == o.good && bits == o.bits; }
};

// ---- the bit-serial decoder over the whole stream ----
static std::vector<Frame> serial(const std::vector<uint8_t> &b, const hp::Config &q) {
    std::vector<Frame> out;
    uint64_t evend = 0;
    uint32_t evkind = hp::kEvAbort;
    for (size_t i = 0; i < b.size(); i++) {
        uint32_t window = 0;
        for (uint32_t k = 0; k < 8; k++) window |= (i + k >= 7 ? (uint32_t)b[i + k - 7] : 0u) << k;
        const bool flag = hm::is_flag(window), ab = hm::is_abort(window);
        if (!flag && !ab) continue;
        const uint64_t from = evend, end = i + 1;
        const bool pair = flag && evkind == hp::kEvFlag;
        evkind = flag ? hp::kEvFlag : hp::kEvAbort, evend = end;
        if (!pair || end - from <= 8) continue;
        Frame f{from, 1, {}};
        for (uint64_t k = from; k < end - 8; k++) {
            uint32_t before = 0;
            for (uint32_t s = 0; s < 5; s++) before |= (k + s >= from + 5 ? (uint32_t)b[k + s - 5] : 0u) << s;
            if (!hm::is_stuffed(b[k], before)) f.bits.push_back(b[k]);
        }
        if (!hp::well_formed((uint32_t)f.bits.size(), q.min_bytes, q.max_bytes)) continue;
        if (q.fcs) {
            uint32_t c = hm::fcs_init(q.fcs);
            for (uint8_t bit : f.bits) c = hm::fcs_step(c, bit, hm::fcs_poly(q.fcs));
            f.good = c == hm::fcs_good(q.fcs);
        }
        if (f.good || q.keep_bad) out.push_back(f);
    }
    return out;
}

// ---- the kernel's walk, lane by lane ----
struct Walker {
    hp::Config q;
    hp::Geom g;
    std::vector<uint64_t> z, ring, obuf;  // the row's state words, the ring, the frame buffer
    uint32_t tab[hp::kPowers], btab[256];
    std::vector<Frame> out;

    explicit Walker(const hp::Config &c) : q(c), g(hp::geom(1, c.max_bytes)), z(g.per, 0), ring(g.RW, 0), obuf(g.OW, 0) {
        hp::fcs_powers(q.fcs, tab);
        for (uint32_t e = 0; e < 256; e++) btab[e] = hm::fcs_table_entry(e, hm::fcs_poly(q.fcs));
    }
    uint64_t &slot(uint32_t word) {
        const uint32_t s = hp::ring_slot(word, g.RW);
        CHECK(s < g.RW);
        return ring[s];
    }
    uint64_t ring_bits(uint64_t bit) {
        const uint32_t w = (uint32_t)(bit >> 6);
        return fm::funnel(slot(w), slot(w + 1), (uint32_t)bit & 63u);
    }
    void push(const uint8_t *b, uint32_t m) {
        const uint32_t tiles = m / 64 + (m % 64 ? 1 : 0), poly = hm::fcs_poly(q.fcs);
        const uint64_t bits0 = z[hp::kStBits];
        uint64_t evend = z[hp::kStEvEnd];
        uint32_t evkind = (uint32_t)z[hp::kStEvKind];
        for (auto &w : ring) w = rnd();  // (what another row left there)
        for (uint32_t j = 0; j < g.HW; j++) slot(j) = z[hp::kStHist + j];
        for (uint32_t t0 = 0; t0 < tiles; t0 += hp::kChunk) {
            for (uint32_t t = t0; t < t0 + hp::kChunk && t < tiles; t++) {
                const uint32_t tn = m - 64 * t < 64 ? m - 64 * t : 64;
                uint64_t w = 0;
                for (uint32_t l = 0; l < tn; l++) w |= (uint64_t)b[64 * t + l] << l;
                slot(hp::tile_word(t, g.HW)) = w;
            }
            for (uint32_t t = t0; t < t0 + hp::kChunk && t < tiles; t++) {
                const uint32_t tn = m - 64 * t < 64 ? m - 64 * t : 64;
                uint64_t flags = 0, aborts = 0;
                for (uint32_t l = 0; l < tn; l++) {
                    const uint32_t x = (uint32_t)ring_bits(hp::window_bit(t, l, g.HW)) & 0xFFu;
                    if (hm::is_flag(x)) flags |= 1ull << l;
                    if (hm::is_abort(x)) aborts |= 1ull << l;
                }
                uint64_t ev = flags | aborts;
                while (ev) {
                    const uint32_t l = (uint32_t)__builtin_ctzll(ev);
                    ev &= ev - 1;
                    const uint64_t end = bits0 + 64ull * t + l + 1, d = end - evend, from = evend;
                    const uint32_t kind = (uint32_t)(flags >> l) & 1u;
                    const bool pair = kind == hp::kEvFlag && evkind == hp::kEvFlag && d > 8 && hp::span_fits(d - 8, q.min_bytes, g.Lmax);
                    evkind = kind, evend = end;
                    if (!pair) continue;
                    const uint32_t L = (uint32_t)d - 8, NW = (L + 63) / 64;
                    CHECK(NW <= 64 * hp::kMaxPass);
                    const uint64_t start = hp::span_bit(t, l, g.HW, (uint32_t)d);
                    CHECK(start >= g.c && (start >> 6) + g.RW > hp::tile_word(t0 + hp::kChunk - 1, g.HW));  // (still in the ring)
                    std::vector<uint64_t> w(NW), sm(NW);
                    std::vector<uint32_t> val(NW);
                    uint32_t stuffed = 0;
                    for (uint32_t j = 0; j < NW; j++) {
                        val[j] = L - 64 * j < 64 ? L - 64 * j : 64;
                        w[j] = ring_bits(start + 64ull * j) & fm::low_mask(val[j]);
                        const uint32_t b5 = j ? (uint32_t)ring_bits(start + 64ull * j - 5) & 31u : 0u;
                        sm[j] = hm::stuffed_mask(w[j], b5) & fm::low_mask(val[j]);
                        stuffed += (uint32_t)__builtin_popcountll(sm[j]);
                    }
                    const uint32_t u = L - stuffed;
                    if (!hp::well_formed(u, q.min_bytes, q.max_bytes)) continue;
                    const uint32_t NO = (u + 63) / 64;
                    CHECK(NO < g.OW);
                    for (auto &o : obuf) o = rnd();
                    for (uint32_t k = 0; k < NO; k++) obuf[k] = 0;
                    uint32_t o = 0;
                    for (uint32_t j = 0; j < NW; j++) {
                        const uint32_t k = val[j] - (uint32_t)__builtin_popcountll(sm[j]), sh = o & 63u;
                        const uint64_t c = hm::delete_bits(w[j], sm[j]);
                        if (k) {
                            CHECK((o >> 6) < NO);
                            obuf[o >> 6] |= c << sh;
                            if (sh + k > 64) {
                                CHECK((o >> 6) + 1 < NO);
                                obuf[(o >> 6) + 1] |= c >> (64 - sh);
                            }
                        }
                        o += k;
                    }
                    CHECK(o == u);
                    uint32_t good = 1;
                    if (q.fcs && u / 8 <= hp::kWalkBytes) {
                        uint32_t c = hm::fcs_init(q.fcs);
                        for (uint32_t k = 0; k < u / 8; k++) c = hm::fcs_byte(c, (uint32_t)(obuf[k >> 3] >> (8 * (k & 7))), btab);
                        good = c == hm::fcs_good(q.fcs);
                    } else if (q.fcs) {
                        uint32_t acc = NO == 1 ? hm::fcs_init(q.fcs) : 0u;
                        for (uint32_t k = 0; k + 1 < NO; k++) {  // the whole words in front of the last, each by the words between
                            CHECK(NO - 2 - k < hp::kPowers);
                            acc ^= hm::fcs_mulmod(tab[NO - 2 - k], hm::fcs_word(k == 0 ? hm::fcs_init(q.fcs) : 0u, obuf[k], 64, poly), q.fcs, poly);
                        }
                        good = hm::fcs_word(acc, obuf[NO - 1], u - 64 * (NO - 1), poly) == hm::fcs_good(q.fcs);
                    }
                    if (!q.keep_bad && !good) continue;
                    Frame f{from, good, {}};
                    for (uint32_t k = 0; k < u; k++) f.bits.push_back((uint8_t)((obuf[k >> 6] >> (k & 63)) & 1u));
                    out.push_back(f);
                }
            }
        }
        if (m) {
            std::vector<uint64_t> h(g.HW);
            for (uint32_t j = 0; j < g.HW; j++) h[j] = ring_bits(64ull * j + m);
            for (uint32_t j = 0; j < g.HW; j++) z[hp::kStHist + j] = h[j];
        }
        z[hp::kStBits] = bits0 + m, z[hp::kStEvEnd] = evend, z[hp::kStEvKind] = evkind;
    }
};

static void append_frame(std::vector<uint8_t> &b, uint32_t bytes, uint32_t fcs, int fill) {
    std::vector<uint8_t> bits;
    for (uint32_t k = 0; k < 8 * bytes; k++) bits.push_back(fill == 0 ? 0 : (fill == 1 ? 1 : (uint8_t)(rnd() & 1)));
    if (fcs) {
        uint32_t c = hm::fcs_init(fcs);
        for (uint8_t bit : bits) c = hm::fcs_step(c, bit, hm::fcs_poly(fcs));
        c = ~c;
        for (uint32_t k = 0; k < fcs; k++) bits.push_back((uint8_t)((c >> k) & 1u));
    }
    uint32_t ones = 0;
    for (uint8_t bit : bits) {
        b.push_back(bit);
        ones = bit ? ones + 1 : 0;
        if (ones == 5) b.push_back(0), ones = 0;
    }
}
static void append_flag(std::vector<uint8_t> &b, bool shared) {
    static const uint8_t f[8] = {0, 1, 1, 1, 1, 1, 1, 0};
    for (int k = shared && !b.empty() && b.back() == 0 ? 1 : 0; k < 8; k++) b.push_back(f[k]);
}

static std::vector<uint8_t> traffic(const hp::Config &q, uint32_t frames) {
    std::vector<uint8_t> b;
    for (uint32_t k = rnd() % 70; k; k--) b.push_back((uint8_t)(rnd() & 1));
    append_flag(b, false);
    for (uint32_t f = 0; f < frames; f++) {
        const uint32_t lo = q.min_bytes - q.fcs / 8, hi = q.max_bytes - q.fcs / 8;
        uint32_t bytes = lo + (uint32_t)(rnd() % (hi - lo + 1));
        const uint32_t pick = (uint32_t)(rnd() % 8);
        if (pick == 0) bytes = hi;
        if (pick == 1) bytes = lo;
        if (pick == 2) bytes = hi + 1;  // (too long: dropped)
        append_frame(b, bytes, q.fcs, (int)(rnd() % 4));
        if (rnd() % 8 == 0) b[b.size() - 1 - rnd() % (b.size() < 40 ? b.size() : 40)] ^= 1;  // (a bit error)
        if (rnd() % 6 == 0)
            for (int k = 0; k < 9; k++) b.push_back(1);  // (an abort)
        for (uint32_t k = 1 + rnd() % 3; k; k--) append_flag(b, rnd() & 1);
        if (rnd() % 4 == 0)
            for (uint32_t k = rnd() % 20; k; k--) b.push_back(1);  // (mark idle)
    }
    return b;
}

int main() {
    // 1. the validation
    const uint32_t fcss[] = {0, 8, 15, 16, 17, 32, 33, 64}, sizes[] = {0, 1, 2, 3, 4, 5, 6, 1023, 1024, 1025, 0xFFFFFFFFu}, flags[] = {0, 1, 2};
    size_t accepted = 0;
    for (int kind : {0, hp::kC64, 31, hp::kRealF32, 33})
        for (uint32_t diff : {0u, 1u, 2u, 3u})
            for (uint32_t fcs : fcss)
                for (uint32_t lo : sizes)
                    for (uint32_t hi : sizes)
                        for (uint32_t msb : flags)
                            for (uint32_t keep : flags) {
                                const hp::Config q{kind, diff, fcs, lo, hi, msb, keep};
                                const bool want = (kind == hp::kC64 || kind == hp::kRealF32) && diff <= 2 && (fcs == 0 || fcs == 16 || fcs == 32) && lo >= 1 &&
                                                  lo <= hi && hi <= 1024 && lo > fcs / 8 && msb <= 1 && keep <= 1;
                                CHECK((hp::check_config(q) == nullptr) == want);
                                accepted += want;
                            }
    CHECK(accepted > 1000);
    // 2. the geometry
    size_t largest = 0;
    for (uint32_t mb = 1; mb <= hp::kMaxBytes; mb++) {
        const hp::Geom g = hp::geom(1 + (uint32_t)(rnd() % hp::kMaxRows), mb);
        CHECK(g.Lmax == 8 * mb + 8 * mb / 5 && g.K == g.Lmax + 8 && g.HW == (g.K + 63) / 64 && g.c == 64 * g.HW - g.K && g.c < 64);
        CHECK((g.RW & (g.RW - 1)) == 0 && g.RW >= g.HW + hp::kChunk + 1 && g.RW <= 256 && g.RW < 2 * (g.HW + hp::kChunk + 1));
        CHECK(g.OW == (mb + 7) / 8 + 1 && g.per == hp::kStHist + g.HW && g.lds_bytes == (size_t)(g.RW + g.OW) * 8 + 1024 && g.G == 1);
        CHECK((g.Lmax + 63) / 64 <= 64u * hp::kMaxPass);  // (a span's words over the lanes)
        if (g.lds_bytes > largest) largest = g.lds_bytes;
    }
    printf("largest lds:%zu\n", largest);
    // 3. the word forms against the bit forms
    for (int it = 0; it < 20000; it++) {
        uint64_t w = rnd();
        if (it & 1) w |= rnd(), w |= rnd();  // (longer runs)
        const uint32_t b5 = (uint32_t)rnd() & 31u;
        const uint64_t m = hm::stuffed_mask(w, b5);
        std::vector<uint8_t> kept;
        for (uint32_t i = 0; i < 64; i++) {
            uint32_t before = 0;
            for (uint32_t s = 0; s < 5; s++) before |= (i + s >= 5 ? (uint32_t)(w >> (i + s - 5)) & 1u : (b5 >> (i + s)) & 1u) << s;
            const bool st = hm::is_stuffed((uint32_t)(w >> i) & 1u, before);
            CHECK(st == (((m >> i) & 1ull) != 0));
            if (!st) kept.push_back((uint8_t)((w >> i) & 1u));
        }
        const uint64_t mm = it % 3 ? m : rnd() & rnd();  // (delete_bits: any mask)
        kept.clear();
        for (uint32_t i = 0; i < 64; i++)
            if (!((mm >> i) & 1ull)) kept.push_back((uint8_t)((w >> i) & 1u));
        const uint64_t c = hm::delete_bits(w, mm);
        for (uint32_t i = 0; i < 64; i++) CHECK(((c >> i) & 1ull) == (i < kept.size() ? kept[i] : 0u));
        for (uint32_t fcs : {16u, 32u}) {
            const uint32_t poly = hm::fcs_poly(fcs), bits = (uint32_t)(rnd() % 65), c0 = (uint32_t)rnd() & (fcs == 16 ? 0xFFFFu : 0xFFFFFFFFu);
            uint32_t a = c0;
            for (uint32_t k = 0; k < bits; k++) a = hm::fcs_step(a, (uint32_t)(w >> k) & 1u, poly);
            CHECK(a == hm::fcs_word(c0, w, bits, poly));
        }
    }
    for (uint32_t fcs : {16u, 32u}) {
        uint32_t tab[hp::kPowers];
        hp::fcs_powers(fcs, tab);
        const uint32_t poly = hm::fcs_poly(fcs), full = fcs == 16 ? 0xFFFFu : 0xFFFFFFFFu;
        CHECK(tab[0] == 1u << (fcs - 1));
        for (int it = 0; it < 300; it++) {
            const uint32_t k = (uint32_t)(rnd() % hp::kPowers), c0 = (uint32_t)rnd() & full;
            uint32_t a = c0;
            for (uint32_t s = 0; s < 64 * k; s++) a = hm::fcs_step(a, 0, poly);  // 64 k zero bits
            CHECK(a == hm::fcs_mulmod(tab[k], c0, fcs, poly) && a == hm::fcs_mulmod(c0, tab[k], fcs, poly) && a <= full);
        }
    }
    // 4. the history's bytes
    for (uint32_t mb : {1u, 2u, 7u, 8u, 33u, 1024u}) {
        const hp::Geom g = hp::geom(1, mb);
        std::vector<uint64_t> w(g.HW), back(g.HW);
        for (auto &x : w) x = rnd();
        std::vector<uint8_t> bytes(hp::history_bytes(g.K)), again(hp::history_bytes(g.K));
        hp::history_to_bytes(w.data(), g, bytes.data());
        hp::history_from_bytes(bytes.data(), g, back.data());
        hp::history_to_bytes(back.data(), g, again.data());
        CHECK(bytes == again && (back[0] & fm::low_mask(g.c)) == 0);
        for (uint32_t k = 0; k < g.K; k++) CHECK(((back[(g.c + k) >> 6] >> ((g.c + k) & 63)) & 1ull) == ((w[(g.c + k) >> 6] >> ((g.c + k) & 63)) & 1ull));
        if (g.K % 8) CHECK((bytes.back() & (0xFFu >> (g.K % 8))) == 0);
    }
    // 5. the walk
    size_t frames = 0, bad = 0, longest = 0;
    for (int it = 0; it < 400; it++) {
        const uint32_t fcs3[] = {0, 16, 32};
        const uint32_t fcs = fcs3[rnd() % 3];
        const uint32_t mbs[] = {1, 2, 5, 8, 9, 31, 32, 64, 100, 256, 1024};
        uint32_t mb = mbs[rnd() % 11];
        if (mb <= fcs / 8) mb = fcs / 8 + 1 + (uint32_t)(rnd() % 8);
        const uint32_t lo = fcs / 8 + 1 + (uint32_t)(rnd() % (mb - fcs / 8));
        const hp::Config q{hp::kRealF32, 0, fcs, lo, mb, 0, (uint32_t)(rnd() & 1)};
        CHECK(hp::check_config(q) == nullptr);
        std::vector<uint8_t> b;
        if (it % 4 == 0) {
            for (uint32_t k = 3000 + rnd() % 2000; k; k--) b.push_back((uint8_t)(rnd() % 8 != 0));  // (noise rich in flags)
        } else {
            b = traffic(q, mb >= 256 ? 4 : 12);
        }
        const std::vector<Frame> want = serial(b, q);
        Walker wk(q);
        size_t at = 0;
        while (at < b.size()) {
            const uint32_t mode = (uint32_t)(rnd() % 4);
            size_t n = mode == 0 ? rnd() % 3 : (mode == 1 ? 60 + rnd() % 10 : (mode == 2 ? rnd() % 700 : 64 * hp::kChunk - 3 + rnd() % 7));
            if (n > b.size() - at) n = b.size() - at;
            wk.push(b.data() + at, (uint32_t)n);
            at += n;
        }
        CHECK(wk.out.size() == want.size());
        for (size_t k = 0; k < want.size(); k++) {
            if (!(wk.out[k] == want[k]))
                fprintf(stderr, "stream %d frame %zu: good %u / %u, %zu / %zu bits, fcs %u, max_bytes %u\n", it, k, wk.out[k].good, want[k].good,
                        wk.out[k].bits.size(), want[k].bits.size(), q.fcs, q.max_bytes);
            CHECK(wk.out[k] == want[k]);
            bad += !want[k].good;
            if (want[k].bits.size() > longest) longest = want[k].bits.size();
        }
        frames += want.size();
        // the state behind the stream: the last K bits, the event
        std::vector<uint8_t> bytes(hp::history_bytes(wk.g.K));
        hp::history_to_bytes(wk.z.data() + hp::kStHist, wk.g, bytes.data());
        for (uint32_t k = 0; k < wk.g.K; k++) {
            const size_t age = wk.g.K - 1 - k;
            const uint8_t bit = age < b.size() ? b[b.size() - 1 - age] : 0;
            CHECK(((bytes[k >> 3] >> (7 - (k & 7))) & 1u) == bit);
        }
        CHECK(wk.z[hp::kStBits] == b.size());
    }
    printf("walk: %zu frames, %zu of them bad, the longest %zu bits\n", frames, bad, longest);
    CHECK(frames > 1000 && bad > 10 && longest == 8192);
    printf("hdlc_plan ok\n");
    return 0;
}
