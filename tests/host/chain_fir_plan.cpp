// chain_fir_plan.cpp -- csrc/hz_chain_fir_plan.h as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_chain_fir_plan.py: the overlap-save geometry of hzsdr_chain_fir_decimate and the list of reference-order
// blocks (slow_blocks_plan) that fir_decimate_kernel16 dispatches first.
//   - argv: seed, rounds.  Random geometries, calls and clock runs: the list against a walk over EVERY block (a span
//     that leaves [0, n - off], touches a run without a filter, or has the boundary of a run with a filter at
//     p0 ... p0 + N), ascending, without repeats, at most kMaxSlowBlocks entries, empty only when the walk finds none
//     or the host's count (a block once per stream edge and per run that lists it) passes kMaxSlowBlocks; the kernel's "c-th block not in the list" by both of its formulas against the walk.
//   - stdin: the cases of tests/test_fir_ref_cpu.py, one per line, answered on stdout for the Python restatement
//     (tests/fir_ref.py) to be compared with:
//         G ntaps D nfft_min                                     ->  G nfft off hop ok
//         S N hop off n nblocks nruns first[0..) has[0..)        ->  S count idx[0..)
// Prints "chain_fir_plan ok" at the end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "hz_chain_fir_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures++ < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                                 \
    } while (0)

using hz::SlowBlocks;

static bool walk_slow(int64_t N, int64_t hop, int64_t off, int64_t n, const std::vector<uint64_t> &first, const std::vector<char> &has, int64_t b) {
    const int64_t p0 = b * hop - off;
    if (p0 < 0 || b * hop > n - N) return true;
    const size_t nr = first.size();
    for (size_t r = 0; r < nr; r++) {
        const int64_t f = (int64_t)first[r], e = r + 1 < nr ? (int64_t)first[r + 1] : n;
        if (!has[r] && e > f && f <= p0 + N - 1 && e - 1 >= p0) return true;
        if (has[r] && r > 0 && p0 <= f && f <= p0 + N) return true;
    }
    return false;
}

static void fuzz(unsigned seed, int rounds) {
    std::mt19937_64 rng(seed);
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (int it = 0; it < rounds; it++) {
        const unsigned factors[] = {1, 2, 3, 4, 5, 8, 10, 16};
        const unsigned D = factors[rng() % 8];
        const unsigned nmins[] = {0, 1024, 2048, 4096, 8192};
        const size_t ntaps = (rng() & 3) == 0 ? pick(6000, 8185) : pick(1, 2100);
        const hz::FirGeom g = hz::fir_geometry(ntaps, D, nmins[rng() % 5]);
        if (!g.ok) continue;
        CHECK(g.nfft >= 1024 && g.nfft <= 8192 && (g.nfft & (g.nfft - 1)) == 0 && (g.nfft >= 4 * ntaps || g.nfft == 8192));
        CHECK(g.off % D == 0 && g.off >= ntaps - 1 && g.off < ntaps - 1 + D && g.hop % D == 0 && g.hop > 0 && g.off + g.hop <= g.nfft &&
              g.off + g.hop + D > g.nfft);
        const int64_t N = g.nfft, hop = g.hop, off = g.off;
        const size_t nblocks = pick(1, 300);
        const int64_t n = (int64_t)((nblocks - 1) * hop + pick(1, hop));
        CHECK((size_t)((n + hop - 1) / hop) == nblocks);
        const int nruns = (int)pick(0, 6);
        std::vector<uint64_t> first;
        std::vector<char> has;
        bool hb[32];
        for (int r = 0; r < nruns; r++) {
            // boundaries at a block's ends, one off, or anywhere
            uint64_t f = r == 0 ? 0 : first.back() + 1 + pick(0, 3 * N);
            if (r > 0 && (rng() & 1)) {
                const int64_t b = (int64_t)pick(0, nblocks - 1), cand = b * hop - off + (int64_t)pick(0, 2) - 1 + ((rng() & 1) ? N : 0);
                if (cand > (int64_t)first.back()) f = (uint64_t)cand;
            }
            if ((int64_t)f >= n) break;
            first.push_back(f);
        }
        for (size_t r = 0; r < first.size(); r++) {
            const int64_t e = r + 1 < first.size() ? (int64_t)first[r + 1] : n;
            has.push_back(e - (int64_t)first[r] >= 2 * N || (rng() % 5 == 0));
            hb[r] = has.back();
        }
        if (first.empty()) {
            has.push_back(1);
            hb[0] = true;
        }
        SlowBlocks s;
        memset(&s, 0xff, sizeof s);
        hz::slow_blocks_plan(N, hop, off, (size_t)n, nblocks, (int)first.size(), first.data(), hb, &s);
        std::vector<uint64_t> f1 = first.empty() ? std::vector<uint64_t>{0} : first;
        std::vector<unsigned> want;
        for (size_t b = 0; b < nblocks; b++)
            if (walk_slow(N, hop, off, n, f1, has, (int64_t)b)) want.push_back((unsigned)b);
        CHECK(s.n >= 0 && s.n <= hz::kMaxSlowBlocks);
        if (want.size() <= (size_t)hz::kMaxSlowBlocks && s.n > 0) {
            CHECK((size_t)s.n == want.size());
            for (int i = 0; i < s.n && (size_t)i < want.size(); i++) CHECK(s.idx[i] == want[i]);
        } else if (s.n == 0) {
            // given up: the host counts a block once per stream edge and per run that lists it, and gives up on THAT
            // count -- the walk (without repeats) may still fit, but not by more than that factor
            CHECK(want.empty() || want.size() * (f1.size() + 2) > (size_t)hz::kMaxSlowBlocks);
        } else {
            CHECK(false);
        }
        // the c-th block not in the list: the scalar scan and the ballot's count against the walk
        std::vector<unsigned> freeb;
        for (size_t b = 0, i = 0; b < nblocks; b++) {
            if (i < (size_t)s.n && s.idx[i] == b) i++;
            else freeb.push_back((unsigned)b);
        }
        for (size_t c = 0; c < freeb.size(); c++) {
            size_t scan = c, ballot = c;
            for (int i = 0; i < s.n; i++) {
                if ((size_t)s.idx[i] <= scan) scan++;
                if ((size_t)(s.idx[i] - (unsigned)i) <= c) ballot++;
            }
            CHECK(scan == freeb[c] && ballot == freeb[c]);
        }
    }
}

int main(int argc, char **argv) {
    static_assert(hz::kMaxSlowBlocks == 96 && hz::kMaxSlowBlocks <= 128, "two entries per lane of one wave");
    fuzz(argc > 1 ? (unsigned)atoi(argv[1]) : 1, argc > 2 ? atoi(argv[2]) : 1000);
    // the refusal and the smallest hop
    CHECK(hz::fir_geometry(8185, 8, 0).ok && hz::fir_geometry(8185, 8, 0).hop == 8 && !hz::fir_geometry(8186, 8, 0).ok);
    CHECK(hz::fir_geometry(8192, 1, 0).hop == 1 && !hz::fir_geometry(8193, 1, 0).ok && !hz::fir_geometry((size_t)1 << 40, 3, 0).ok);
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'G') {
            unsigned long long ntaps;
            unsigned D, nmin;
            if (scanf("%llu %u %u", &ntaps, &D, &nmin) != 3) return 2;
            const hz::FirGeom g = hz::fir_geometry((size_t)ntaps, D, nmin);
            printf("G %u %u %u %d\n", g.nfft, g.off, g.hop, g.ok ? 1 : 0);
        } else if (kind == 'S') {
            long long N, hop, off, n, nblocks;
            int nruns;
            if (scanf("%lld %lld %lld %lld %lld %d", &N, &hop, &off, &n, &nblocks, &nruns) != 6 || nruns < 0 || nruns > 32) return 2;
            std::vector<uint64_t> first((size_t)(nruns ? nruns : 1), 0);
            bool hb[32] = {false};
            for (int r = 0; r < nruns; r++) {
                unsigned long long f;
                if (scanf("%llu", &f) != 1) return 2;
                first[(size_t)r] = f;
            }
            for (int r = 0; r < (nruns ? nruns : 1); r++) {
                int h;
                if (scanf("%d", &h) != 1) return 2;
                hb[r] = h != 0;
            }
            SlowBlocks s;
            hz::slow_blocks_plan(N, hop, off, (size_t)n, (size_t)nblocks, nruns, first.data(), hb, &s);
            printf("S %d", s.n);
            for (int i = 0; i < s.n; i++) printf(" %u", s.idx[i]);
            printf("\n");
        } else {
            return 2;
        }
    }
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("chain_fir_plan ok\n");
    return 0;
}
