// viterbi_plan.cpp -- the host arithmetic of the Viterbi decoder bank (csrc/hz_viterbi_plan.h, csrc/hz_viterbi_math.h) as
// a stand-alone program for the sanitizers:
//   1. the plan for every (K, n, termination) with D at its bounds and around the edge between the two decision forms:
//      frames per wave times states is a wave, the LDS regions follow each other without overlap, the request stays inside
//      the family's budget and FORM_LDS is chosen exactly where the whole frame fits;
//   2. the puncture index table against a bit-by-bit walk, for every pattern length and many patterns of each;
//   3. a wave, emulated lane by lane with the kernel's own maps (which lane and register hold a state, where its
//      predecessors live, the decision word and bit, the tile's words, the decoded words, the chunks of the scratch form)
//      over buffers of exactly the planned sizes, against a plain state-array decoder: decoded words, metric, end state;
//   4. the CRC's byte table against the bit steps, and the largest LDS request.
// Prints "viterbi_plan ok" and "largest lds: N".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hz_viterbi_math.h"
#include "hz_viterbi_plan.h"

using namespace hz;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            if (++failures > 20) exit(1);                          \
        }                                                          \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static const uint32_t kGens[10][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {5, 7, 7, 5}, {015, 017, 013, 011}, {023, 035, 027, 033},
                                      {053, 075, 047, 067}, {0171, 0133, 0165, 0117}, {0247, 0371, 0225, 0331}, {0557, 0663, 0711, 0745}};

static vp::Config config(uint32_t K, uint32_t n, int term, uint32_t D, uint32_t C = 0) {
    vp::Config q{vp::kBits, K, n, {0, 0, 0, 0}, 0, (1ull << n) - 1, n, term, D, 1.0f, C, C ? 0x07u : 0u, 0, 0};
    for (uint32_t j = 0; j < n; j++) q.gens[j] = kGens[K][j];
    return q;
}

static size_t largest = 0;

static void plan_of(const vp::Config &q) {
    CHECK(vp::check_config(q) == nullptr);
    const vp::Geom g = vp::geom(q);
    CHECK(g.S == 1u << (q.K - 1) && g.G * g.S == (g.S < 64 ? 64 : g.S));
    CHECK(g.G * g.gsz == 64 || (g.G == 1 && g.gsz == 64));
    CHECK(g.SPL * 64 == (g.S > 64 ? g.S : 64) && g.gsz == (g.S < 64 ? g.S : 64));
    CHECK(g.off_tb == g.G * 256 && g.off_crc == g.off_tb + g.G * g.DW * 8 && g.off_dec == g.off_crc + (q.C ? 1024 : 0) && g.off_dec % 8 == 0);
    const size_t whole = (size_t)g.off_dec + (size_t)g.T * g.SPL * 8;
    CHECK((g.form == vp::kFormLds) == (whole <= vp::kLdsBudget));
    CHECK(g.lds_bytes == g.off_dec + (size_t)g.chunk * g.SPL * 8 && g.lds_bytes <= vp::kLdsBudget);
    CHECK(g.form == vp::kFormLds ? (g.chunk == g.T && g.scratch_words == 0) : (g.chunk == vp::kChunkSteps && g.scratch_words == (size_t)g.max_waves * g.T * g.SPL));
    CHECK(g.decision_bytes == (size_t)g.T * g.S / 8 && g.tiles * 64 >= g.T && (g.tiles - 1) * 64 < g.T);
    CHECK(vp::waves_for(g, 1) == 1 && vp::waves_for(g, g.G) == 1 && vp::waves_for(g, g.G + 1) == 2 && vp::waves_for(g, vp::kMaxFrames) == g.max_waves);
    if (g.lds_bytes > largest) largest = g.lds_bytes;
}

static void plans() {
    for (uint32_t K = vp::kMinK; K <= vp::kMaxK; K++)
        for (uint32_t n = 2; n <= 4; n++)
            for (int term = 0; term < 2; term++) {
                const uint32_t tail = term == vp::kTail ? K - 1 : 0;
                const uint32_t Dmax = (vp::kMaxBits / n) - tail;  // N = T n <= 8192
                for (uint32_t D : {1u, 2u, 63u, 64u, 65u, Dmax - 1, Dmax}) plan_of(config(K, n, term, D));
                for (uint32_t C : {8u, 32u}) plan_of(config(K, n, term, Dmax, C));
                CHECK(vp::check_config(config(K, n, term, Dmax + 1)) != nullptr);
            }
    // T up to 8192 needs a pattern that sends one bit per step: the form's edge for every K
    for (uint32_t K = vp::kMinK; K <= vp::kMaxK; K++) {
        int forms = 0;
        for (uint32_t D = 1000; D <= vp::kMaxBits - (K - 1); D += (D < 8000 ? 97 : 1)) {
            vp::Config q = config(K, 2, vp::kTail, D, 16);
            q.pattern = 0b10;
            q.poly = 0x1021;
            plan_of(q);
            forms |= vp::geom(q).form;
        }
        CHECK(forms == (vp::kFormLds | vp::kFormScratch));  // both forms are reached for every K
    }
}

static void index_tables() {
    for (uint32_t n = 2; n <= 4; n++)
        for (uint32_t Lp = n; Lp <= 64; Lp += n)
            for (int trial = 0; trial < 12; trial++) {
                vp::Config q = config(7, n, trial & 1, 50 + (uint32_t)(rng() % 300));
                uint64_t pat = trial == 0 ? ~0ull : rng() | (trial == 1 ? 0 : rng());
                for (uint32_t m = 0; m < Lp; m += n) pat |= 1ull << (Lp - 1 - m - rng() % n);  // a 1 in every group
                q.pattern = Lp < 64 ? pat & ((1ull << Lp) - 1) : pat, q.Lp = Lp;
                CHECK(vp::check_config(q) == nullptr);
                const vp::Geom g = vp::geom(q);
                std::vector<uint16_t> idx;
                vp::build_index(q, g, idx);
                CHECK(idx.size() == (size_t)g.T * n);
                uint32_t at = 0;
                for (uint32_t m = 0; m < g.T * n; m++) {
                    const bool sent = (q.pattern >> (Lp - 1 - m % Lp)) & 1ull;
                    CHECK(idx[m] == (sent ? at : vm::kPunctured));
                    at += sent;
                }
                CHECK(at == g.N && g.N <= vp::kMaxBits && g.FB == (g.N + 7) / 8);
            }
}

// a plain decoder over state arrays -> end state, metric, the decoded bits
static void plain(const vp::Config &c, const vp::Geom &g, const std::vector<uint32_t> &qw, uint32_t &end, uint32_t &fin, std::vector<uint8_t> &u) {
    const uint32_t S = g.S;
    std::vector<uint32_t> metric(S, vm::kInf), next(S);
    std::vector<uint8_t> dec((size_t)g.T * S);
    metric[0] = 0;
    for (uint32_t t = 0; t < g.T; t++) {
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t e0 = vm::expected(vm::branch_reg(s, 0, c.K), c.gens, c.n, c.inv), e1 = vm::expected(vm::branch_reg(s, 1, c.K), c.gens, c.n, c.inv);
            dec[(size_t)t * S + s] = (uint8_t)vm::acs(metric[vm::predecessor(s, 0, S)], vm::branch_cost(qw[t], e0), metric[vm::predecessor(s, 1, S)],
                                                      vm::branch_cost(qw[t], e1), &next[s]);
        }
        metric.swap(next);
    }
    end = 0;
    if (c.term == vp::kTruncated)
        for (uint32_t k = 1; k < S; k++)
            if (metric[k] < metric[end]) end = k;
    fin = metric[end];
    u.assign(g.T, 0);
    uint32_t s = end;
    for (uint32_t t = g.T; t-- > 0;) u[t] = (uint8_t)vm::input_of(s, c.K), s = vm::predecessor(s, dec[(size_t)t * S + s], S);
}

// one wave over G frames, lane by lane, with the kernel's maps and buffers of the planned sizes
static void wave(const vp::Config &c) {
    CHECK(vp::check_config(c) == nullptr);
    const vp::Geom g = vp::geom(c);
    const uint32_t SPL = g.SPL, H = SPL > 1 ? SPL / 2 : 1, wave_id = g.max_waves - 1;  // the last wave's part of the scratch
    std::vector<uint32_t> qs(g.off_tb / 4);
    std::vector<uint64_t> tb((g.off_crc - g.off_tb) / 8), dl((g.lds_bytes - g.off_dec) / 8), scratch(g.scratch_words);
    uint64_t *sc = g.form == vp::kFormScratch ? scratch.data() + (size_t)wave_id * g.T * SPL : nullptr;
    // the frames' values: random q with many zeros and equal magnitudes, so that ties are frequent
    std::vector<std::vector<uint32_t>> qw(g.G, std::vector<uint32_t>(g.T));
    for (auto &fr : qw)
        for (auto &w : fr) {
            w = 0;
            for (uint32_t j = 0; j < c.n; j++) w |= vm::pack_q((int)(rng() % 5) - 2, j);
        }
    std::vector<uint32_t> m(SPL * 64), nm(SPL * 64);
    for (uint32_t lane = 0; lane < 64; lane++)
        for (uint32_t k = 0; k < SPL; k++) m[k * 64 + lane] = (k == 0 && lane % g.gsz == 0) ? 0 : vm::kInf;
    for (uint32_t tile = 0; tile < g.tiles; tile++) {
        const uint32_t t0 = tile * 64, tn = g.T - t0 < 64 ? g.T - t0 : 64;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t gi = lane / g.gsz, sl = lane % g.gsz;
            for (uint32_t tl = sl; tl < 64; tl += g.gsz) qs.at(gi * 64 + tl) = t0 + tl < g.T ? qw[gi][t0 + tl] : 0;
        }
        for (uint32_t tl = 0; tl < tn; tl++) {
            uint64_t words[4] = {0, 0, 0, 0};
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t gi = lane / g.gsz, gbase = gi * g.gsz, sl = lane - gbase;
                const uint32_t w = qs.at(gi * 64 + tl);
                for (uint32_t k = 0; k < SPL; k++) {
                    const uint32_t s = vp::lane_state(k, sl), h = vp::pair_of(k, SPL);
                    CHECK(vp::state_lane(gbase, s) == lane && vp::state_reg(s) == k && h < H);
                    uint32_t pm[2];
                    for (uint32_t b = 0; b < 2; b++) {
                        const uint32_t pl = vp::pred_lane(gbase, sl, b, g.S, SPL), pr = vp::pred_reg(h, sl, SPL);
                        const uint32_t p = vm::predecessor(s, b, g.S);
                        CHECK(pl == vp::state_lane(gbase, p) && pr == vp::state_reg(p));  // the exchange fetches the predecessor
                        pm[b] = m.at(pr * 64 + pl);
                    }
                    const uint32_t e0 = vm::expected(vm::branch_reg(s, 0, c.K), c.gens, c.n, c.inv), e1 = vm::expected(vm::branch_reg(s, 1, c.K), c.gens, c.n, c.inv);
                    const uint32_t d = vm::acs(pm[0], vm::branch_cost(w, e0), pm[1], vm::branch_cost(w, e1), &nm.at(k * 64 + lane));
                    words[k] |= (uint64_t)d << lane;
                }
            }
            m = nm;
            for (uint32_t k = 0; k < SPL; k++) {
                const size_t at = (size_t)(t0 + tl) * SPL + k;
                if (sc)
                    scratch.at((size_t)wave_id * g.T * SPL + at) = words[k];
                else
                    dl.at(at) = words[k];
            }
        }
    }
    for (uint32_t gi = 0; gi < g.G; gi++) {
        uint32_t end, fin;
        std::vector<uint8_t> u;
        plain(c, g, qw[gi], end, fin, u);
        const uint32_t gbase = gi * g.gsz;
        // the end state as the kernel finds it: the smallest metric << 16 | state
        uint64_t key = ~0ull;
        for (uint32_t s = 0; s < g.S; s++) {
            const uint64_t mine = ((uint64_t)m[vp::state_reg(s) * 64 + vp::state_lane(gbase, s)] << 16) | s;
            if (mine < key) key = mine;
        }
        const uint32_t es = c.term == vp::kTail ? 0 : (uint32_t)key & 0xffffu;
        CHECK(es == end && m[vp::state_reg(es) * 64 + vp::state_lane(gbase, es)] == fin && fin < (1u << 23));
        uint32_t s = es;
        uint64_t acc = 0;
        for (int32_t c0 = (int32_t)(((g.T - 1) / g.chunk) * g.chunk); c0 >= 0; c0 -= (int32_t)g.chunk) {
            const uint32_t cn = g.T - (uint32_t)c0 < g.chunk ? g.T - (uint32_t)c0 : g.chunk;
            if (sc)
                for (uint32_t i = 0; i < cn * SPL; i++) dl.at(i) = sc[(size_t)c0 * SPL + i];
            for (int32_t t = c0 + (int32_t)cn - 1; t >= c0; t--) {
                if ((uint32_t)t < c.D) {
                    acc |= (uint64_t)vm::input_of(s, c.K) << (t & 63);
                    if ((t & 63) == 0) tb.at(gi * g.DW + ((uint32_t)t >> 6)) = acc, acc = 0;
                }
                const uint32_t d = (uint32_t)(dl.at(vp::dec_word((uint32_t)t, (uint32_t)c0, s, SPL)) >> vp::dec_bit(gbase, s)) & 1u;
                s = vm::predecessor(s, d, g.S);
            }
        }
        for (uint32_t t = 0; t < c.D; t++) CHECK(((tb[gi * g.DW + (t >> 6)] >> (t & 63)) & 1u) == u[t]);
        for (uint32_t t = (uint32_t)c.D; t < g.DW * 64; t++) CHECK(((tb[gi * g.DW + (t >> 6)] >> (t & 63)) & 1u) == 0);
    }
}

static void waves() {
    for (uint32_t K = vp::kMinK; K <= vp::kMaxK; K++)
        for (uint32_t n = 2; n <= 4; n++)
            for (int term = 0; term < 2; term++)
                for (uint32_t D : {1u, K - 2, K - 1, K, 63u, 64u, 65u, 78u, 200u}) wave(config(K, n, term, D));
    for (uint32_t K = vp::kMinK; K <= vp::kMaxK; K++) {  // the scratch form: chunks of the traceback, T no multiple of a chunk
        vp::Config q = config(K, 2, vp::kTail, vp::kMaxBits - (K - 1) - 3, 8);
        q.pattern = 0b10;
        CHECK(vp::geom(q).form == vp::kFormScratch);
        wave(q);
    }
}

static void crc_tables() {
    for (uint32_t C : {8u, 16u, 24u, 32u})
        for (int trial = 0; trial < 8; trial++) {
            const uint32_t poly = (uint32_t)rng() & vm::crc_mask(C), init = (uint32_t)rng() & vm::crc_mask(C);
            uint32_t table[256];
            for (uint32_t b = 0; b < 256; b++) table[b] = vm::crc_table_entry(b, C, poly);
            uint32_t a = init, b = init;
            for (int k = 0; k < 40; k++) {
                const uint32_t byte = (uint32_t)rng() & 0xffu;
                a = vm::crc_byte(a, byte, C, table);
                for (int i = 7; i >= 0; i--) b = vm::crc_step(b, (byte >> i) & 1u, C, poly);
                CHECK(a == b && a <= vm::crc_mask(C));
            }
        }
    // a word of the stream (the earliest bit lowest) as its bytes, most significant bit first
    const uint64_t w = 0x8001ull | (1ull << 63);  // stream bits 0, 15, 63
    CHECK(vm::stream_byte(fm::out_word(w), 0) == 0x80 && vm::stream_byte(fm::out_word(w), 1) == 0x01 && vm::stream_byte(fm::out_word(w), 7) == 0x01);
}

int main() {
    plans();
    index_tables();
    waves();
    crc_tables();
    printf("largest lds: %zu\n", largest);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("viterbi_plan ok\n");
    return 0;
}
