// rs_plan.cpp -- the host arithmetic of the Reed-Solomon decoder bank (csrc/hz_rs_plan.h, csrc/hz_rs_math.h) as a
// stand-alone program, built by tests/test_rs_plan.py with AddressSanitizer and UndefinedBehaviorSanitizer:
//   1. the plan at every bound: every (nroots, n, interleave) at the edges of its range, the LDS layout's regions in
//      order, disjoint and inside the request, the request inside the family's budget, the occupancy it states;
//   2. the validation of a configuration (every primitive polynomial found by an independent order count) and of a call;
//   3. a workgroup emulated wave by wave and lane by lane with the kernel's own index maps (rsp::frame_index,
//      chien_position, bm_syndrome, the table block's offsets, the LDS offsets) over heap buffers of EXACTLY the planned
//      sizes -- the table block, the LDS, the input and the output spans -- against rsm::decode_word: clean words, 1 ... t
//      and more errors, all 0x00, all 0xFF, and random words far from any codeword.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_rs_math.h"
#include "hz_rs_plan.h"

using namespace hz;

static void check_failed(int line, const char *what) {
    printf("rs_plan: line %d: %s\n", line, what);
    exit(1);
}
#define CHECK(c) ((c) ? (void)0 : check_failed(__LINE__, #c))

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

static size_t largest_lds = 0;

static void plan_bounds() {
    for (uint32_t nroots : {2u, 3u, 16u, 32u, 63u, 64u})
        for (uint32_t n : {nroots + 1, nroots + 2, 204u, 254u, 255u})
            for (uint32_t I = 1; I <= rsp::kMaxInterleave; I++) {
                if (n <= nroots) continue;
                const rsp::Config q{0x187, 112, 11, nroots, n, I, 0};
                CHECK(rsp::check_config(q) == nullptr);
                const rsp::Geom g = rsp::geom(q);
                CHECK(g.k == n - nroots && g.t == nroots / 2 && g.F == I * n && g.IK == I * g.k && g.waves == I && g.threads == 64 * I);
                CHECK(g.off_frame == rsp::kTabBytes && g.off_frame % 16 == 0 && g.off_wave >= g.off_frame + g.F && g.off_wave % 16 == 0);
                CHECK(g.off_res == g.off_wave + I * rsp::kWaveBytes && g.off_res % 4 == 0 && g.lds_bytes == g.off_res + 4 * I);
                CHECK(g.lds_bytes <= rsp::kLdsBudget && g.table_bytes == rsp::kTabBytes + g.F);
                CHECK(g.groups_per_cu == 32 / I);  // the wave slots set it, never the LDS
                CHECK(g.t <= 32 && rsp::kWaveLam - rsp::kWaveSyn >= 64 && rsp::kWaveOmg - rsp::kWaveLam >= 64 && rsp::kWaveBytes - rsp::kWaveOmg >= 64);
                if (g.lds_bytes > largest_lds) largest_lds = g.lds_bytes;
            }
    CHECK(rsp::kPasses * 64 >= rsp::kMaxN);
    CHECK(rsp::groups_for(1) == 1 && rsp::groups_for(rsp::kMaxGroups) == rsp::kMaxGroups && rsp::groups_for(rsp::kMaxFrames) == rsp::kMaxGroups);
}

static void validation() {
    uint32_t primitive = 0;
    for (uint32_t p = 0; p < 0x400; p++) {
        // independently: the order of x modulo p, by repeated doubling
        bool want = false;
        if ((p >> 8) == 1) {
            uint32_t x = 1, order = 0;
            do {
                x <<= 1;
                if (x & 0x100) x ^= p;
                order++;
            } while (x != 1 && x != 0 && order < 300);
            want = x == 1 && order == 255;
        }
        CHECK(rsp::primitive(p) == want);
        uint8_t exp[rsm::kExpSize], log[rsm::kLogSize];
        if ((p >> 8) == 1) CHECK(rsm::build_tables(p, exp, log) == want);
        primitive += want;
    }
    CHECK(primitive == 16);
    const rsp::Config ok{0x187, 112, 11, 32, 255, 4, 255};
    CHECK(!rsp::check_config(ok));
    for (uint32_t prim = 0; prim < 300; prim++) {
        rsp::Config q = ok;
        q.prim = prim;
        CHECK((rsp::check_config(q) == nullptr) == (prim >= 1 && prim <= 254 && prim % 3 && prim % 5 && prim % 17));
    }
    rsp::Config q = ok;
    q.fcr = 255, CHECK(rsp::check_config(q)), q = ok;
    q.nroots = 1, CHECK(rsp::check_config(q)), q.nroots = 65, CHECK(rsp::check_config(q)), q = ok;
    q.n = 32, CHECK(rsp::check_config(q)), q.n = 256, CHECK(rsp::check_config(q)), q = ok;
    q.interleave = 0, CHECK(rsp::check_config(q)), q.interleave = 9, CHECK(rsp::check_config(q)), q = ok;
    q.scramble_len = 2041, CHECK(rsp::check_config(q)), q.scramble_len = 2040, CHECK(!rsp::check_config(q));

    const rsp::Geom g = rsp::geom(ok);  // F = 1020, I k = 892
    const char *why;
    const uintptr_t A = 1 << 20;
    auto call = [&](uintptr_t in, uintptr_t out, size_t is, size_t ip, size_t os, size_t op, size_t cap, size_t rows, bool info = true) {
        return rsp::check_call(g, rsp::Call{in, out, is, ip, os, op, cap, rows, info}, &why);
    };
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kOk);
    CHECK(call(A, 2 * A, 0, 1020, 0, 892, 3, 1) == rsp::kOk);  // one row: no strides
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 0, 2) == rsp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, (rsp::kMaxFrames / 2) + 1, 2) == rsp::kInvalid);
    CHECK(call(0, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid && call(A, 0, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 892, 3, 2, false) == rsp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1019, 3 * 892, 892, 3, 2) == rsp::kInvalid && call(A, 2 * A, 3 * 1020, 1020, 3 * 892, 891, 3, 2) == rsp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020 - 1, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid);
    CHECK(call(A, 2 * A, 3 * 1020, 1020, 3 * 892 - 1, 892, 3, 2) == rsp::kDstTooSmall);
    CHECK(call(A, A, 3 * 1020, 1020, 3 * 1020, 1020, 3, 2) == rsp::kOk);  // in place
    CHECK(call(A, A, 3 * 1020, 1020, 3 * 1024, 1020, 3, 2) == rsp::kInvalid && call(A, A, 3 * 1024, 1024, 3 * 1024, 1020, 3, 2) == rsp::kInvalid);
    const size_t ispan = 3 * 1020 + 2 * 1020 + 1020, ospan = 3 * 892 + 2 * 892 + 892;
    CHECK(call(A, A + ispan, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kOk && call(A, A + ispan - 1, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid);
    CHECK(call(A + ospan, A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kOk && call(A + ospan - 1, A, 3 * 1020, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid);
    CHECK(call(A, A + 1, 3 * 1020, 1020, 3 * 1020, 1020, 3, 2) == rsp::kInvalid);
    CHECK(call(A, 2 * A, (size_t)1 << 41, 1020, 3 * 892, 892, 3, 2) == rsp::kInvalid && call(A, 2 * A, 0, ~(size_t)0, 0, 892, 3, 1) == rsp::kInvalid);
}

// ---- the workgroup, lane by lane ----
// one frame at src (F bytes exactly) -> dst (I k bytes exactly) and info, as hz_rs.hip's kernel goes about it
static uint32_t emulate(const rsp::Config &q, const rsp::Geom &g, const std::vector<uint8_t> &block, const uint8_t *src, uint8_t *dst) {
    std::vector<uint8_t> lds_v(g.lds_bytes);
    uint8_t *lds = lds_v.data();
    const uint32_t nthr = g.threads, I = q.interleave;
    const rsm::Code c{q.gfpoly, q.fcr, q.prim, q.nroots, q.n};
    for (uint32_t tid = 0; tid < nthr; tid++)
        for (uint32_t i = tid; i < rsp::kTabBytes / 4; i += nthr) memcpy(lds + 4 * i, block.data() + 4 * i, 4);
    const uint8_t *exp = lds + rsp::kTabExp, *log = lds + rsp::kTabLog, *imap = lds + rsp::kTabIn, *omap = lds + rsp::kTabOut;
    const uint8_t *scr = block.data() + rsp::kTabBytes;
    uint8_t *frame = lds + g.off_frame;
    int32_t res[rsp::kMaxInterleave];
    uint32_t whole = ((uintptr_t)src & 3u) == 0 ? g.F >> 2 : 0;
    for (uint32_t tid = 0; tid < nthr; tid++) {
        for (uint32_t w = tid; w < whole; w += nthr) {
            uint8_t x[4], s[4];
            memcpy(x, src + 4 * w, 4), memcpy(s, scr + 4 * w, 4);
            for (int b = 0; b < 4; b++) x[b] = imap[x[b] ^ s[b]];
            memcpy(frame + 4 * w, x, 4);
        }
        for (uint32_t m = 4 * whole + tid; m < g.F; m += nthr) frame[m] = imap[src[m] ^ scr[m]];
    }
    for (uint32_t wave = 0; wave < I; wave++) {
        uint8_t *wl = lds + g.off_wave + wave * rsp::kWaveBytes;
        uint8_t *syn = wl + rsp::kWaveSyn, *lamA = wl + rsp::kWaveLam, *omgA = wl + rsp::kWaveOmg;
        uint32_t s[64], any = 0;
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint32_t lroot = rsm::root_log(c, lane < c.nroots ? lane : 0);
            uint32_t P[8], a = 0, b = 0;
            rsm::products(exp[lroot], c.poly, P);
            for (uint32_t p = 0; p < c.n; p++) {
                const uint32_t v = frame[rsp::frame_index(wave, p, I)];
                a = rsm::mul_products(a, P) ^ v, b = rsm::mul_log(b, lroot, exp, log) ^ v;
            }
            CHECK(a == b);  // the two forms of the multiply
            s[lane] = lane < c.nroots ? a : 0, any |= s[lane];
        }
        int32_t e = 0;
        if (any) {
            for (uint32_t lane = 0; lane < 64; lane++) syn[lane] = (uint8_t)s[lane];
            uint32_t lam[64] = {1}, B[64] = {1}, L = 0;
            for (uint32_t it = 0; it < c.nroots; it++) {
                uint32_t d = 0, bs[64], nl[64];
                for (uint32_t lane = 0; lane < 64; lane++) d ^= rsm::bm_term(lam[lane], lane <= it ? syn[rsp::bm_syndrome(it, lane)] : 0u, c.poly);
                for (uint32_t lane = 0; lane < 64; lane++) bs[lane] = lane ? B[lane - 1] : 0;
                for (uint32_t lane = 0; lane < 64; lane++) {
                    if (d) {
                        nl[lane] = rsm::bm_lambda(lam[lane], d, bs[lane], c.poly);
                        B[lane] = 2 * L <= it ? rsm::bm_b(lam[lane], rsm::inv(d, exp, log), c.poly) : bs[lane];
                        lam[lane] = nl[lane];
                    } else {
                        B[lane] = bs[lane];
                    }
                }
                if (d && 2 * L <= it) L = it + 1 - L;
                if (L > g.t) break;
            }
            if (L > g.t || L == 0) {
                e = rsm::kFailed;
            } else {
                for (uint32_t lane = 0; lane < 64; lane++) lamA[lane] = (uint8_t)lam[lane];
                for (uint32_t lane = 0; lane < 64; lane++) omgA[lane] = lane < L ? (uint8_t)rsm::omega_coeff(lamA, syn, lane, c.poly) : 0;
                uint32_t roots = 0, ev[rsp::kPasses][64];
                bool hit[rsp::kPasses][64];
                for (uint32_t ps = 0; ps < rsp::kPasses; ps++)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        const uint32_t p = rsp::chien_position(ps, lane);
                        const bool valid = p < c.n;
                        const uint32_t xl = valid ? rsm::locator_log(c, p) : 0u;
                        hit[ps][lane] = valid && rsm::poly_eval(lamA, L, exp[rsm::neg_log(xl)], c.poly) == 0;
                        roots += hit[ps][lane];
                        ev[ps][lane] = hit[ps][lane] ? rsm::forney(lamA, omgA, L, xl, c, exp, log) : 0u;
                    }
                if (roots == L) {
                    for (uint32_t ps = 0; ps < rsp::kPasses; ps++)
                        for (uint32_t lane = 0; lane < 64; lane++)
                            if (hit[ps][lane]) frame[rsp::frame_index(wave, rsp::chien_position(ps, lane), I)] ^= (uint8_t)ev[ps][lane];
                    e = (int32_t)L;
                } else {
                    e = rsm::kFailed;
                }
            }
        }
        memcpy(lds + g.off_res + 4 * wave, &e, 4);
    }
    whole = ((uintptr_t)dst & 3u) == 0 ? g.IK >> 2 : 0;
    for (uint32_t tid = 0; tid < nthr; tid++) {
        for (uint32_t w = tid; w < whole; w += nthr)
            for (int b = 0; b < 4; b++) dst[4 * w + b] = omap[frame[4 * w + b]];
        for (uint32_t m = 4 * whole + tid; m < g.IK; m += nthr) dst[m] = omap[frame[m]];
    }
    uint32_t E = 0, nfail = 0;
    memcpy(res, lds + g.off_res, 4 * I);
    for (uint32_t i = 0; i < I; i++) {
        if (res[i] < 0)
            nfail++;
        else
            E += (uint32_t)res[i];
    }
    return E | nfail << 16 | (nfail ? 0u : 1u << 31);
}

static uint32_t frames_run = 0, failed_words = 0, corrected_words = 0;

static void one_frame(const rsp::Config &q, const uint8_t *imap, const uint8_t *omap, const std::vector<uint8_t> &scramble, const std::vector<uint8_t> &sent,
                      size_t misalign) {
    const rsp::Geom g = rsp::geom(q);
    std::vector<uint8_t> block;
    CHECK(rsp::build_block(q, g, imap, omap, scramble.empty() ? nullptr : scramble.data(), block));
    CHECK(block.size() == g.table_bytes);
    std::vector<uint8_t> in(g.F + misalign), out(g.IK + misalign, 0xA5);
    memcpy(in.data() + misalign, sent.data(), g.F);
    const uint32_t info = emulate(q, g, block, in.data() + misalign, out.data() + misalign);
    // the plain statement
    uint8_t exp[rsm::kExpSize], log[rsm::kLogSize];
    CHECK(rsm::build_tables(q.gfpoly, exp, log));
    std::vector<uint8_t> v(g.F);
    for (uint32_t m = 0; m < g.F; m++) {
        const uint8_t b = sent[m] ^ (q.scramble_len ? scramble[m % q.scramble_len] : 0);
        v[m] = imap ? imap[b] : b;
    }
    const rsm::Code c{q.gfpoly, q.fcr, q.prim, q.nroots, q.n};
    uint32_t E = 0, nfail = 0;
    for (uint32_t i = 0; i < q.interleave; i++) {
        const int e = rsm::decode_word(c, exp, log, v.data() + i, q.interleave);
        if (e < 0)
            nfail++, failed_words++;
        else
            E += (uint32_t)e, corrected_words += e > 0;
    }
    CHECK(info == (E | nfail << 16 | (nfail ? 0u : 1u << 31)));
    for (uint32_t m = 0; m < g.IK; m++) CHECK(out[misalign + m] == (omap ? omap[v[m]] : v[m]));
    for (size_t m = 0; m < misalign; m++) CHECK(out[m] == 0xA5);
    frames_run++;
}

// (this program has no encoder: the errors are planted into the frame that prepares to all-zero codewords, which under
// a scramble sequence and a map is as arbitrary a byte string as any)
static void workgroups() {
    const uint32_t codes[][5] = {{0x187, 112, 11, 32, 255}, {0x11D, 0, 1, 16, 204}, {0x11D, 3, 7, 2, 3}, {0x187, 112, 11, 5, 6}, {0x11D, 1, 2, 64, 65},
                                 {0x187, 0, 1, 64, 255}, {0x11D, 200, 254, 3, 255}};
    uint8_t perm[256], back[256];
    for (uint32_t b = 0; b < 256; b++) perm[b] = (uint8_t)(b * 167u + 13u);  // odd multiplier: a permutation
    for (uint32_t b = 0; b < 256; b++) back[perm[b]] = (uint8_t)b;
    for (const auto &cd : codes) {
        for (uint32_t I : {1u, 2u, 3u, 8u}) {
            for (uint32_t variant = 0; variant < 2; variant++) {
                const uint32_t slen = variant ? I * cd[4] + 1 : 0;
                const rsp::Config q{cd[0], cd[1], cd[2], cd[3], cd[4], I, slen > rsp::kMaxScramble ? 255u : slen};
                CHECK(!rsp::check_config(q));
                const rsp::Geom g = rsp::geom(q);
                std::vector<uint8_t> scramble(q.scramble_len);
                for (auto &b : scramble) b = (uint8_t)rnd();
                const uint8_t *imap = variant ? perm : nullptr, *omap = variant ? back : nullptr;
                // the frame that prepares to the all-zero codewords
                std::vector<uint8_t> zero(g.F);
                for (uint32_t m = 0; m < g.F; m++) zero[m] = (imap ? back[0] : 0) ^ (q.scramble_len ? scramble[m % q.scramble_len] : 0);
                for (uint32_t errs : {0u, 1u, g.t - (g.t > 1), g.t, g.t + 1, q.nroots}) {
                    std::vector<uint8_t> f = zero;
                    for (uint32_t i = 0; i < I; i++) {
                        std::vector<uint32_t> pos(q.n);
                        for (uint32_t p = 0; p < q.n; p++) pos[p] = p;
                        for (uint32_t j = 0; j < errs && j < q.n; j++) {
                            const uint32_t o = j + rnd() % (q.n - j);
                            const uint32_t tmp = pos[j];
                            pos[j] = pos[o], pos[o] = tmp;
                            f[rsp::frame_index(i, pos[j], I)] ^= (uint8_t)(1 + rnd() % 255);  // (a change before the maps: still a change behind them)
                        }
                    }
                    one_frame(q, imap, omap, scramble, f, errs % 4);
                }
                one_frame(q, imap, omap, scramble, std::vector<uint8_t>(g.F, 0x00), 0);
                one_frame(q, imap, omap, scramble, std::vector<uint8_t>(g.F, 0xFF), 1);
                for (int k = 0; k < 3; k++) {
                    std::vector<uint8_t> f(g.F);
                    for (auto &b : f) b = (uint8_t)rnd();
                    one_frame(q, imap, omap, scramble, f, (size_t)k);
                }
            }
        }
    }
    CHECK(failed_words > 100 && corrected_words > 100);
}

int main() {
    plan_bounds();
    validation();
    workgroups();
    printf("frames: %u, corrected words: %u, failed words: %u\n", frames_run, corrected_words, failed_words);
    printf("largest lds:%zu\n", largest_lds);
    printf("rs_plan ok\n");
    return 0;
}
