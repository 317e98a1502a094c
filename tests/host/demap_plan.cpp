// demap_plan.cpp -- the demapper bank's host arithmetic (csrc/hz_demap_plan.h, csrc/hz_demap_math.h) as a stand-alone
// program for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_demap_plan.py):
//   1. forged perm entries at and above S m, non-finite points and gains, over heap arrays of exactly the stated lengths:
//      every one refused with no access outside the arrays;
//   2. the plan at the bounds (S = 8192 with m = 2, S = 2048 with m = 8, N = 1, N = 8192) and over random admissible
//      shapes: threads in whole waves, at most 1024 per workgroup, the LDS request inside the budget, every slot of a
//      call visited exactly once by the kernel's walk;
//   3. a call walked as the kernel walks it -- frames side by side in a buffer of exactly the planned LDS bytes, inputs
//      and outputs in buffers of exactly the call's spans, the values written symbol by symbol and gathered in output
//      order -- against a plain loop, with both forms of the minima, for every m;
//   4. the check of a call at its edges.
// Prints "largest lds: N" and "demap_plan ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "hz_demap_math.h"
#include "hz_demap_plan.h"
#include "hz_received.h"

using namespace hz;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static float unit() { return (float)((double)(rnd() >> 11) / (double)(1ull << 53) * 2.0 - 1.0); }

// heap arrays of exactly n elements: one past the end is the sanitizer's
template <class T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

static dmp::Config config(int kind, uint64_t m, uint64_t S, uint64_t N, bool perm, uint64_t n_gains = 1, uint64_t rows = 1) {
    return dmp::Config{kind, m, S, N, kind != dmp::kLlrF32, perm, n_gains, rows};
}

static void forged_arrays() {
    const uint64_t m = 3, S = 11, N = 20, L = S * m;
    const dmp::Config q = config(dmp::kC64, m, S, N, true, 2, 2);
    CHECK(!dmp::check_config(q));
    auto pts = exact<float>(2u << m);
    auto perm = exact<uint32_t>(N);
    auto gains = exact<float>(2);
    for (uint32_t i = 0; i < (2u << m); i++) pts[i] = unit();
    for (uint32_t k = 0; k < N; k++) perm[k] = (uint32_t)(rnd() % L);
    gains[0] = 1.0f, gains[1] = 0.25f;
    CHECK(!dmp::check_arrays(q, pts.get(), perm.get(), gains.get()));
    perm[N - 1] = dm::kErased, perm[0] = (uint32_t)L - 1;
    CHECK(!dmp::check_arrays(q, pts.get(), perm.get(), gains.get()));
    for (uint32_t bad : {(uint32_t)L, (uint32_t)L + 1, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu}) {
        for (uint32_t at : {0u, 7u, (uint32_t)N - 1}) {
            const uint32_t keep = perm[at];
            perm[at] = bad;
            CHECK(dmp::check_arrays(q, pts.get(), perm.get(), gains.get()) != nullptr);
            perm[at] = keep;
        }
    }
    for (float bad : {INFINITY, -INFINITY, NAN}) {
        const float keep = pts[(2u << m) - 1];
        pts[(2u << m) - 1] = bad;
        CHECK(dmp::check_arrays(q, pts.get(), perm.get(), gains.get()) != nullptr);
        pts[(2u << m) - 1] = keep;
    }
    for (float bad : {0.0f, -0.0f, -1.0f, INFINITY, NAN}) {
        gains[1] = bad;
        CHECK(dmp::check_arrays(q, pts.get(), perm.get(), gains.get()) != nullptr);
    }
    gains[1] = 1e-45f;  // the least denormal is positive and finite
    CHECK(!dmp::check_arrays(q, pts.get(), perm.get(), gains.get()));
    CHECK(dmp::check_arrays(q, pts.get(), perm.get(), nullptr) != nullptr);
    // the scalars
    CHECK(dmp::check_config(config(dmp::kC64, 0, 8, 8, true)) && dmp::check_config(config(dmp::kC64, 9, 8, 8, true)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 0, 8, true)) && dmp::check_config(config(dmp::kC64, 1, 8193, 8, true)));
    CHECK(dmp::check_config(config(dmp::kC64, 8, 2049, 8, true)) && !dmp::check_config(config(dmp::kC64, 8, 2048, 8, true)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 8, 0, true)) && dmp::check_config(config(dmp::kC64, 2, 8, 8193, true)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 8, 15, false)) && !dmp::check_config(config(dmp::kC64, 2, 8, 16, false)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 8, 16, false, 2, 3)) && !dmp::check_config(config(dmp::kC64, 2, 8, 16, false, 3, 3)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 8, 16, false, 1, 0)) && dmp::check_config(config(dmp::kC64, 2, 8, 16, false, 1, 8193)));
    CHECK(dmp::check_config(config(dmp::kC64, 2, 8, 16, false, 0, 1)) && dmp::check_config(config(dmp::kC64, 2, ~0ull, 16, true)));
    CHECK(!dmp::check_config(config(dmp::kLlrF32, 1, 8, 8, false)) && dmp::check_config(config(dmp::kLlrF32, 2, 8, 16, false)));
    dmp::Config llr_points = config(dmp::kLlrF32, 1, 8, 8, false);
    llr_points.has_points = true;
    CHECK(dmp::check_config(llr_points) != nullptr);
    dmp::Config no_points = config(dmp::kRealF32, 1, 8, 8, false);
    no_points.has_points = false;
    CHECK(dmp::check_config(no_points) != nullptr);
    CHECK(dmp::known(1) && dmp::known(32) && dmp::known(33) && !dmp::known(0) && !dmp::known(2) && !dmp::known(34));
}

static size_t largest_lds = 0;

static void plan_of(const dmp::Config &q) {
    CHECK(!dmp::check_config(q));
    const dmp::Geom g = dmp::geom(q);
    CHECK(g.T % dmp::kLanes == 0 && g.T >= dmp::kLanes && g.T <= dmp::kMaxThreads && (g.T >= g.S || g.T == dmp::kMaxThreads));
    CHECK(g.G >= 1 && g.G <= dmp::kMaxGroup && g.G * g.T <= dmp::kMaxThreads);
    CHECK(g.frame_floats >= g.L && g.frame_floats % 4 == 0 && g.lds_bytes == (size_t)g.G * g.frame_floats * 4);
    CHECK(g.lds_bytes <= dmp::kLdsBudget && g.lds_bytes <= 160 * 1024);
    CHECK(g.W == (q.kind == dmp::kC64 ? 2 * g.S : g.S) && g.L == g.S * g.m);
    CHECK(((g.form & dmp::kFormGrouped) != 0) == (g.G > 1) && ((g.form & dmp::kFormPerm) != 0) == q.has_perm);
    CHECK(((g.form & dmp::kFormTree) != 0) == (q.kind != dmp::kLlrF32 && g.m >= dmp::kTreeFrom));
    if (g.lds_bytes > largest_lds) largest_lds = g.lds_bytes;
    // the kernel's walk over a call's slots: every slot once, whatever the grid
    for (uint32_t slots : {1u, g.G - 1 ? g.G - 1 : 1u, g.G, g.G + 1, 5 * g.G + 3}) {
        const uint32_t grid = dmp::groups_for(g, slots);
        CHECK(grid >= 1 && grid <= dmp::kMaxGrid);
        std::vector<uint8_t> seen(slots, 0);
        for (uint32_t w = 0; w < grid; w++)
            for (uint32_t base = w * g.G; base < slots; base += grid * g.G)
                for (uint32_t k = 0; k < g.G && base + k < slots; k++) seen[base + k]++;
        for (uint32_t s = 0; s < slots; s++) CHECK(seen[s] == 1);
    }
}

static void plans() {
    plan_of(config(dmp::kC64, 2, 8192, 8192, true));
    plan_of(config(dmp::kC64, 8, 2048, 8192, true));
    plan_of(config(dmp::kC64, 8, 2048, 1, true));
    plan_of(config(dmp::kC64, 1, 1, 1, false));
    plan_of(config(dmp::kRealF32, 2, 4096, 8192, false));
    plan_of(config(dmp::kLlrF32, 1, 8192, 8192, false));
    plan_of(config(dmp::kLlrF32, 1, 1, 8192, true));
    for (uint32_t S : {1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 1023u, 1024u, 1025u}) plan_of(config(dmp::kC64, 4, S, 4 * S, false));
    for (int i = 0; i < 300; i++) {
        const uint64_t m = 1 + rnd() % 8, S = 1 + rnd() % (dmp::kMaxLlrs / m < dmp::kMaxSymbols ? dmp::kMaxLlrs / m : dmp::kMaxSymbols);
        const bool perm = S * m > dmp::kMaxOut || (rnd() & 1);
        plan_of(config(rnd() & 1 ? dmp::kC64 : dmp::kRealF32, m, S, perm ? 1 + rnd() % dmp::kMaxOut : S * m, perm));
    }
    const dmp::Geom big = dmp::geom(config(dmp::kC64, 8, 2048, 8192, true));
    CHECK(big.T == 1024 && big.G == 1 && big.lds_bytes == 65536);
    const dmp::Geom small = dmp::geom(config(dmp::kC64, 4, 64, 256, false));
    CHECK(small.T == 64 && small.G == 8 && small.lds_bytes == 8 * 1024);
}

// ---- a call, as the kernel walks it ----
template <int m, bool CPLX, bool TREE> static void symbol(float xr, float xi, const float *pts, float *d0, float *d1) {
    if (TREE)
        dm::symbol_tree<m, CPLX>(xr, xi, pts, d0, d1);
    else
        dm::symbol_naive<m, CPLX>(xr, xi, pts, d0, d1);
}

template <int m, bool CPLX> static void walk(uint32_t S, uint32_t N, bool has_perm, bool has_flip, uint32_t R, uint32_t cap) {
    const int kind = CPLX ? dmp::kC64 : dmp::kRealF32;
    const dmp::Config q = config(kind, m, S, N, has_perm, R, R);
    CHECK(!dmp::check_config(q));
    const dmp::Geom g = dmp::geom(q);
    const uint32_t M = 1u << m, pf = CPLX ? 2 * M : M;
    auto pts = exact<float>(pf);
    auto perm = exact<uint32_t>(has_perm ? N : 0);
    auto flip = exact<uint8_t>(has_flip ? dbp::packed_bytes(N) : 0);
    auto gains = exact<float>(R);
    auto counts = exact<uint32_t>(R);
    for (uint32_t i = 0; i < pf; i++) pts[i] = unit();
    for (uint32_t k = 0; has_perm && k < N; k++) perm[k] = rnd() % 7 == 0 ? dm::kErased : (uint32_t)(rnd() % g.L);
    for (uint32_t k = 0; has_flip && k < dbp::packed_bytes(N); k++) flip[k] = (uint8_t)rnd();
    for (uint32_t r = 0; r < R; r++) gains[r] = 0.5f + (float)r, counts[r] = (uint32_t)(rnd() % (cap + 2));
    CHECK(!dmp::check_arrays(q, pts.get(), perm.get(), gains.get()));
    const size_t in_stride = (size_t)cap * g.W + 3, out_stride = (size_t)cap * g.N + 5;
    const size_t in_len = (size_t)(R - 1) * in_stride + (size_t)cap * g.W, out_len = (size_t)(R - 1) * out_stride + (size_t)cap * g.N;
    auto in = exact<float>(in_len);
    auto out = exact<uint32_t>(out_len);
    auto want = exact<uint32_t>(out_len);
    for (size_t i = 0; i < in_len; i++) in[i] = 1.5f * unit();
    in[0] = NAN, in[in_len - 1] = INFINITY;
    for (size_t i = 0; i < out_len; i++) out[i] = want[i] = 0xA5A5A5A5u;
    const dbp::Call c{(uintptr_t)in.get(), (uintptr_t)out.get(), in_stride, g.W, out_stride, g.N, cap, R, true};
    const char *why = nullptr;
    CHECK(dmp::check_run(g, c, &why) == dbp::kOk);

    // the plain loop
    std::vector<float> L(g.L);
    for (uint32_t r = 0; r < R; r++)
        for (uint32_t f = 0; f < cap && f < counts[r]; f++) {
            const float *x = in.get() + r * in_stride + (size_t)f * g.W;
            for (uint32_t s = 0; s < S; s++) {
                const float xr = CPLX ? x[2 * s] : x[s], xi = CPLX ? x[2 * s + 1] : 0.0f;
                for (uint32_t j = 0; j < (uint32_t)m; j++) {
                    float d0 = INFINITY, d1 = INFINITY;
                    for (uint32_t p = 0; p < M; p++) {
                        const float d = dm::point_dist<CPLX>(xr, xi, (const float *)pts.get(), p);
                        float &side = dm::bit_of(p, m, j) ? d1 : d0;
                        if (d < side) side = d;
                    }
                    L[s * m + j] = (xr != xr || xi != xi) ? NAN : dm::llr(d0, d1, gains[r]);
                }
            }
            for (uint32_t k = 0; k < N; k++) {
                const uint32_t at = has_perm ? perm[k] : k;
                want[r * out_stride + (size_t)f * g.N + k] = dm::stored(at == dm::kErased ? NAN : L[at], has_flip ? rx::packed_bit(flip.get(), k) : 0u);
            }
        }

    // the kernel's walk, both forms of the minima
    for (int tree = 0; tree < 2; tree++) {
        auto lds = exact<float>(g.lds_bytes / 4);
        const uint32_t slots = R * cap, grid = dmp::groups_for(g, slots);
        for (uint32_t w = 0; w < grid; w++)
            for (uint32_t base = w * g.G; base < slots; base += grid * g.G) {
                for (int pass = 0; pass < 2; pass++)  // (the barrier between the two passes)
                    for (uint32_t tid = 0; tid < g.G * g.T; tid++) {
                        const uint32_t gi = tid / g.T, t = tid - gi * g.T, slot = base + gi;
                        uint32_t row, f;
                        if (slot >= slots || !dbp::slot_frame(slot, cap, counts.get(), &row, &f)) continue;
                        float *Lf = lds.get() + (size_t)gi * g.frame_floats;
                        if (pass == 0) {
                            const float *x = in.get() + row * in_stride + (size_t)f * g.W;
                            for (uint32_t s = t; s < S; s += g.T) {
                                const float xr = CPLX ? x[2 * s] : x[s], xi = CPLX ? x[2 * s + 1] : 0.0f;
                                float d0[m], d1[m];
                                if (tree)
                                    symbol<m, CPLX, true>(xr, xi, pts.get(), d0, d1);
                                else
                                    symbol<m, CPLX, false>(xr, xi, pts.get(), d0, d1);
                                for (int j = 0; j < m; j++) Lf[(size_t)s * m + j] = (xr != xr || xi != xi) ? NAN : dm::llr(d0[j], d1[j], gains[row]);
                            }
                        } else {
                            for (uint32_t k = t; k < N; k += g.T) {
                                const uint32_t at = has_perm ? perm[k] : k;
                                out[row * out_stride + (size_t)f * g.N + k] = dm::stored(at == dm::kErased ? NAN : Lf[at], has_flip ? rx::packed_bit(flip.get(), k) : 0u);
                            }
                        }
                    }
            }
        CHECK(memcmp(out.get(), want.get(), out_len * 4) == 0);
        for (size_t i = 0; i < out_len; i++) out[i] = 0xA5A5A5A5u;
    }
}

template <int m> static void walks() {
    walk<m, true>(37, 37 * m + 9, true, true, 3, 2);
    walk<m, true>(65, 65 * m, false, false, 1, 9);
    walk<m, false>(130, 77, true, false, 2, 3);
    walk<m, false>(1, m, false, true, 2, 9);
}

static void calls() {
    const dmp::Geom g = dmp::geom(config(dmp::kC64, 4, 10, 40, false, 1, 3));  // W = 20, N = 40
    const char *why;
    const uintptr_t A = 1u << 20;
    auto rc = [&](uintptr_t in, uintptr_t out, size_t is, size_t os, size_t cap, size_t rows) {
        return dmp::check_run(g, dbp::Call{in, out, is, g.W, os, g.N, cap, rows, true}, &why);
    };
    CHECK(rc(A, A + 65536, 60, 120, 3, 3) == dbp::kOk && rc(A, A + 65536, 59, 120, 3, 3) == dbp::kInvalid && rc(A, A + 65536, 60, 119, 3, 3) == dbp::kDstTooSmall);
    CHECK(rc(A, A + 65536, 60, 120, 0, 3) == dbp::kInvalid && rc(0, A, 60, 120, 3, 3) == dbp::kInvalid && rc(A, 0, 60, 120, 3, 3) == dbp::kInvalid);
    CHECK(rc(A, A + 240, 0, 0, 3, 1) == dbp::kOk && rc(A, A + 236, 0, 0, 3, 1) == dbp::kInvalid && rc(A, A, 0, 0, 3, 1) == dbp::kInvalid);
    CHECK(rc(A + 480, A, 0, 0, 3, 1) == dbp::kOk && rc(A + 476, A, 0, 0, 3, 1) == dbp::kInvalid);
    CHECK(rc(A, A + 65536, ~(size_t)0, 120, 3, 2) == dbp::kInvalid && rc(A, (uintptr_t)1 << 44, 60, ~(size_t)0 / 2, 3, 2) == dbp::kInvalid);
    CHECK(rc(A, (uintptr_t)1 << 44, (size_t)1 << 30, (size_t)1 << 30, dbp::kMaxFrames / 3, 3) == dbp::kOk);
    CHECK(rc(A, (uintptr_t)1 << 44, (size_t)1 << 30, (size_t)1 << 30, dbp::kMaxFrames / 3 + 1, 3) == dbp::kInvalid);
}

int main() {
    forged_arrays();
    plans();
    walks<1>(), walks<2>(), walks<3>(), walks<4>(), walks<5>(), walks<6>(), walks<7>(), walks<8>();
    calls();
    static_assert(dm::naive_minima(8) == 2048 && dm::tree_minima(8) == 768 && dm::tree_minima(6) == 188 && dm::tree_minima(7) == 380, "the counts of the header");
    static_assert(dm::tree_minima(1) == 1 * (3 * 2 - 3) && dm::tree_minima(5) == 93, "one block");
    printf("largest lds: %zu\n", largest_lds);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demap_plan ok\n");
    return 0;
}
