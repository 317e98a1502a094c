// ldpc_plan.cpp -- the host arithmetic of the LDPC decoder bank (csrc/hz_ldpc_plan.h, csrc/hz_ldpc_math.h) as a
// stand-alone program for the sanitizers:
//   1. forged codes -- row pointers that start above 0, descend, run past the edges or disagree with them, columns at
//      and above n, repeated and descending columns, checks of degree 0, 1 and 65, variables of degree 0 and 65, E above
//      its bound, head + N above n, every scalar one step outside -- over arrays of EXACTLY the stated lengths: every one
//      is refused, and the sanitizers see no access outside the arrays;
//   2. random admissible codes and the codes at the bounds: the plan's threads and frames per workgroup, the LDS regions
//      one behind the other without overlap, the request inside the 160 KiB it reports against, the form chosen exactly
//      where the tables fit beside one frame; the tables by variable against the tables by check;
//   3. a workgroup's frame emulated with the kernel's own passes and layout (the check pass over P and the messages'
//      bytes, the variable pass through the tables by variable) inside a buffer of exactly the planned LDS bytes, in the
//      LAST frame slot, against a plain decoder with a message per edge and two generations of P: hard bits and info.
// Prints "ldpc_plan ok" and "largest lds: N".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_ldpc_math.h"
#include "hz_ldpc_plan.h"

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

struct Code {
    uint32_t n;
    std::vector<uint32_t> row_ptr, col;  // exactly m + 1 and E entries: the sanitizer guards their ends
};

// dv bands of n / dc checks, each band a permutation of the variables cut into checks (n a multiple of dc)
static Code banded(uint32_t n, uint32_t dv, uint32_t dc) {
    Code c{n, {0}, {}};
    std::vector<uint32_t> perm(n);
    for (uint32_t b = 0; b < dv; b++) {
        for (uint32_t i = 0; i < n; i++) perm[i] = i;
        if (b)
            for (uint32_t i = n - 1; i > 0; i--) std::swap(perm[i], perm[rng() % (i + 1)]);
        for (uint32_t k = 0; k < n / dc; k++) {
            std::vector<uint32_t> vs(perm.begin() + k * dc, perm.begin() + (k + 1) * dc);
            for (size_t i = 1; i < vs.size(); i++)
                for (size_t j = i; j > 0 && vs[j] < vs[j - 1]; j--) std::swap(vs[j], vs[j - 1]);
            c.col.insert(c.col.end(), vs.begin(), vs.end());
            c.row_ptr.push_back((uint32_t)c.col.size());
        }
    }
    return c;
}

static lp::Config config(const Code &c, uint32_t head = 0, uint32_t N = 0, uint32_t D = 0) {
    const uint32_t n = c.n;
    if (!N) N = n - head > lp::kMaxBits ? lp::kMaxBits : n - head;
    return lp::Config{lp::kSoftF32, c.row_ptr.size() - 1, n, c.col.size(), head, N, D ? D : n, 1.0f, 1, 20, 12, 0};
}

static bool accepted(const lp::Config &q, const Code &c) {
    if (lp::check_config(q)) return false;
    // (the entry's caller states the lengths; the program hands over arrays of exactly those)
    if (c.row_ptr.size() != q.m + 1 || c.col.size() != q.E) return false;
    return lp::check_code(q, c.row_ptr.data(), c.col.data()) == nullptr;
}

// ---- 1. forged codes ----
static void forged() {
    const Code good = banded(96, 3, 6);
    CHECK(accepted(config(good), good));
    {  // scalars one step outside
        lp::Config q = config(good);
        auto bad = [&](lp::Config v) { CHECK(lp::check_config(v) != nullptr); };
        lp::Config v = q;
        v.m = 0, bad(v), v = q, v.m = 16385, bad(v), v = q, v.n = 1, bad(v), v = q, v.n = 16385, bad(v);
        v = q, v.E = 0, bad(v), v = q, v.E = 65537, bad(v), v = q, v.N = 0, bad(v), v = q, v.N = 8193, bad(v);
        v = q, v.head = 1, bad(v), v = q, v.head = 97, v.N = 1, bad(v), v = q, v.head = ~0ull, v.N = 2, bad(v);
        v = q, v.D = 0, bad(v), v = q, v.D = 97, bad(v), v = q, v.max_iters = 0, bad(v), v = q, v.max_iters = 256, bad(v);
        v = q, v.a = 0, bad(v), v = q, v.a = 17, bad(v), v = q, v.beta = 127, bad(v);
        v = q, v.scale = 0.0f, bad(v), v = q, v.scale = -1.0f, bad(v), v = q, v.scale = INFINITY, bad(v), v = q, v.scale = NAN, bad(v);
        v = q, v.kind = lp::kBits, v.level = 0, bad(v), v.level = 128, bad(v);
        v.level = 127;
        CHECK(lp::check_config(v) == nullptr);
        v = q, v.head = 95, v.N = 1;
        CHECK(lp::check_config(v) == nullptr);
        v = q, v.E = 287;  // fewer edges than row_ptr says
        CHECK(lp::check_code(v, good.row_ptr.data(), good.col.data()) != nullptr);
        v = q, v.m = 47;  // fewer checks than the edges need
        CHECK(lp::check_code(v, good.row_ptr.data(), good.col.data()) != nullptr);
    }
    auto refuse = [&](Code c) { CHECK(!accepted(config(c), c)); };
    Code c = good;
    c.row_ptr[0] = 1, refuse(c);
    c = good, c.row_ptr[5] = c.row_ptr[4] - 1, refuse(c);          // descends
    c = good, c.row_ptr[5] = 0xffffffffu, refuse(c);               // far past the edges
    c = good, c.row_ptr[7] = 100000, refuse(c);
    c = good, c.row_ptr.back() = (uint32_t)c.col.size() + 1, refuse(c);
    c = good, c.row_ptr.back() = (uint32_t)c.col.size() - 1, refuse(c);
    c = good, c.row_ptr[3] = c.row_ptr[2], refuse(c);              // a check of degree 0 (and its neighbour of 12)
    c = good, c.row_ptr[3] = c.row_ptr[2] + 1, refuse(c);          // degree 1
    for (uint32_t k = 1; k < c.row_ptr.size(); k++) c.row_ptr[k] = 0xfffffff0u + k;  // every pointer forged
    refuse(c);
    c = good, c.col[10] = 96, refuse(c);
    c = good, c.col[10] = 0xffffffffu, refuse(c);
    c = good, c.col[7] = c.col[6], refuse(c);                      // a repeated column
    c = good, std::swap(c.col[12], c.col[13]), refuse(c);          // descending
    {                                                                // a check of degree 65 and one of 64
        Code w{130, {0}, {}};
        for (uint32_t v = 0; v < 65; v++) w.col.push_back(v);
        w.row_ptr.push_back(65);
        for (uint32_t v = 65; v < 130; v++) w.col.push_back(v);
        w.row_ptr.push_back(130);
        refuse(w);
        Code ok{128, {0, 64, 128}, {}};
        for (uint32_t v = 0; v < 128; v++) ok.col.push_back(v);
        CHECK(accepted(config(ok), ok));
    }
    {  // a variable of degree 0, of 64 and of 65
        Code w = good;
        w.n = 97, refuse(w);
        for (uint32_t deg : {64u, 65u}) {
            Code v{deg * 2 + 1, {0}, {}};
            for (uint32_t k = 0; k < deg; k++) {
                v.col.push_back(0), v.col.push_back(1 + 2 * k), v.col.push_back(2 + 2 * k);
                v.row_ptr.push_back((uint32_t)v.col.size());
            }
            CHECK(accepted(config(v), v) == (deg == 64));
        }
    }
    {  // E above the bound: 16384 checks of degree 5
        Code w{16384, {0}, {}};
        for (uint32_t k = 0; k < 16384; k++) {
            for (uint32_t j = 0; j < 5; j++) w.col.push_back((k + j * 7) % 16384);
            w.row_ptr.push_back((uint32_t)w.col.size());
        }
        refuse(w);
    }
}

// ---- 2. the plan ----
static size_t largest = 0;

static lp::Geom plan_of(const Code &c, const lp::Config &q, lp::Tables &t) {
    CHECK(accepted(q, c));
    const lp::Geom g = lp::geom(q);
    CHECK(g.T % 64 == 0 && g.T >= 64 && g.T <= 1024 && g.G >= 1 && g.G <= lp::kMaxGroup && g.G * g.T <= 1024);
    CHECK(g.off_q >= 2 * g.n && g.off_r >= g.off_q + g.n && g.frame_bytes >= g.off_r + g.E && g.off_q % 4 == 0 && g.frame_bytes % 16 == 0);
    const size_t tables = 4 * (size_t)(g.m + 1) + 4 * (size_t)(g.n + 1) + 4 * (size_t)g.E;
    CHECK(g.table_bytes >= tables);
    CHECK((g.form == lp::kFormTablesLds) == (lp::kHeadBytes + g.table_bytes + g.frame_bytes <= lp::kLdsBudget));
    if (g.form == lp::kFormTablesLds) {
        CHECK(g.off_rowptr == lp::kHeadBytes && g.off_vptr == g.off_rowptr + 4 * (g.m + 1) && g.off_col == g.off_vptr + 4 * (g.n + 1));
        CHECK(g.off_vedge == g.off_col + 2 * g.E && g.off_vedge + 2 * g.E <= g.off_frames && g.off_frames == lp::kHeadBytes + g.table_bytes);
    } else {
        CHECK(g.off_frames == lp::kHeadBytes);
    }
    CHECK(g.off_frames % 16 == 0 && g.lds_bytes == g.off_frames + (size_t)g.G * g.frame_bytes && g.lds_bytes <= lp::kLdsBudget);
    // one frame more, or the threads of one more, would not fit
    CHECK(g.G == lp::kMaxGroup || (g.G + 1) * g.T > 1024 || g.lds_bytes + g.frame_bytes > lp::kLdsBudget);
    if (g.lds_bytes > largest) largest = g.lds_bytes;
    CHECK(lp::groups_for(g, 1) == 1 && lp::groups_for(g, g.G) == 1 && lp::groups_for(g, g.G + 1) == 2 && lp::groups_for(g, (size_t)1 << 22) <= lp::kMaxGrid);
    lp::build_tables(q, c.row_ptr.data(), c.col.data(), t);
    CHECK(t.row_ptr.size() == g.m + 1 && t.vptr.size() == g.n + 1 && t.col.size() == g.E && t.vedge.size() == g.E);
    CHECK(t.vptr[0] == 0 && t.vptr[g.n] == g.E);
    for (uint32_t v = 0; v < g.n; v++) {
        CHECK(t.vptr[v + 1] > t.vptr[v] && t.vptr[v + 1] - t.vptr[v] <= 64);
        for (uint32_t k = t.vptr[v]; k < t.vptr[v + 1]; k++) {
            CHECK(t.col[t.vedge[k]] == v);
            CHECK(k == t.vptr[v] || t.vedge[k] > t.vedge[k - 1]);
        }
    }
    return g;
}

// ---- 3. a frame through the kernel's passes, inside the planned LDS ----
static uint32_t plain(const lp::Config &c, const Code &code, const std::vector<int> &q, std::vector<uint8_t> &hard) {
    const uint32_t m = (uint32_t)c.m, n = (uint32_t)c.n, E = (uint32_t)c.E;
    const std::vector<uint32_t> &rp = code.row_ptr, &col = code.col;
    std::vector<int> r(E, 0), t(E), P(q), next(n);
    hard.assign(n, 0);
    auto unsat = [&]() {
        uint32_t u = 0;
        for (uint32_t k = 0; k < m; k++) {
            uint32_t par = 0;
            for (uint32_t e = rp[k]; e < rp[k + 1]; e++) par ^= P[col[e]] > 0;
            u += par;
        }
        return u;
    };
    uint32_t u = unsat(), it = 0;
    while (u && it < c.max_iters) {
        it++;
        for (uint32_t e = 0; e < E; e++) t[e] = lm::to_check(P[col[e]], r[e]);
        for (uint32_t k = 0; k < m; k++) {
            lm::Check ck = lm::check_start();
            for (uint32_t e = rp[k]; e < rp[k + 1]; e++) lm::check_take(ck, e - rp[k], t[e]);
            for (uint32_t e = rp[k]; e < rp[k + 1]; e++)
                r[e] = lm::to_variable(ck, e - rp[k], t[e], lm::scaled(ck.m1, c.a, c.beta), lm::scaled(ck.m2, c.a, c.beta));
        }
        for (uint32_t v = 0; v < n; v++) next[v] = q[v];
        for (uint32_t e = 0; e < E; e++) next[col[e]] += r[e];
        P.swap(next);
        u = unsat();
    }
    for (uint32_t v = 0; v < n; v++) hard[v] = P[v] > 0;
    return lm::info_word(u, it);
}

static void emulate(const Code &code, const lp::Config &c, const lp::Geom &g, const lp::Tables &t, uint32_t noise) {
    std::vector<int> q(g.n);
    for (uint32_t v = 0; v < g.n; v++) {
        const bool got = v >= g.head && v - g.head < g.N;
        q[v] = got ? (rng() % 100 < noise ? -(int)(rng() % 40) : 127 - (int)(rng() % 120)) : 0;
    }
    std::vector<unsigned char> lds(g.lds_bytes);  // exactly the request
    unsigned char *fr = lds.data() + g.off_frames + (size_t)(g.G - 1) * g.frame_bytes;
    int16_t *P = (int16_t *)fr;
    int8_t *lq = (int8_t *)(fr + g.off_q), *r = (int8_t *)(fr + g.off_r);
    for (uint32_t v = 0; v < g.n; v++) lq[v] = (int8_t)q[v], P[v] = (int16_t)q[v];
    for (uint32_t e = 0; e < g.E; e++) r[e] = 0;
    uint32_t it = 0, u = 0;
    for (;;) {
        const bool last = it == c.max_iters;
        u = 0;
        for (uint32_t k = 0; k < g.m; k++) {
            const uint32_t beg = t.row_ptr[k], end = t.row_ptr[k + 1];
            lm::Check ck = lm::check_start();
            uint32_t syn = 0;
            for (uint32_t e = beg; e < end; e++) {
                const int p = P[t.col[e]];
                const int te = lm::to_check(p, r[e]);
                syn ^= p > 0;
                lm::check_take(ck, e - beg, te);
                r[e] = (int8_t)te;
            }
            if (!last) {
                const int s1 = lm::scaled(ck.m1, c.a, c.beta), s2 = lm::scaled(ck.m2, c.a, c.beta);
                for (uint32_t e = beg; e < end; e++) r[e] = (int8_t)lm::to_variable(ck, e - beg, r[e], s1, s2);
            }
            u += syn;
        }
        if (u == 0 || last) break;
        for (uint32_t v = 0; v < g.n; v++) {
            int s = lq[v];
            for (uint32_t k = t.vptr[v]; k < t.vptr[v + 1]; k++) s += r[t.vedge[k]];
            CHECK(s >= -127 * 65 && s <= 127 * 65);
            P[v] = (int16_t)s;
        }
        it++;
    }
    std::vector<uint8_t> hard;
    const uint32_t want = plain(c, code, q, hard);
    CHECK(lm::info_word(u, it) == want);
    for (uint32_t v = 0; v < g.n; v++) CHECK((P[v] > 0) == (hard[v] != 0));
}

int main() {
    forged();
    lp::Tables t;
    const uint32_t shapes[][3] = {{96, 3, 6}, {512, 3, 6}, {2048, 3, 6}, {128, 2, 2}, {640, 5, 64}, {1024, 64, 64}, {8192, 4, 8}, {16384, 4, 8},
                                  {16384, 2, 2}, {1022, 3, 7}, {65, 1, 5}};
    for (auto &s : shapes) {
        const Code c = banded(s[0], s[1], s[2]);
        lp::Config q = config(c);
        q.max_iters = 6;
        const lp::Geom g = plan_of(c, q, t);
        printf("n %u m %u E %u: T %u G %u form %d frame %u lds %zu\n", g.n, g.m, g.E, g.T, g.G, g.form, g.frame_bytes, g.lds_bytes);
        if (g.E <= 8192)
            for (uint32_t noise : {0u, 8u, 30u}) emulate(c, q, g, t, noise);
    }
    for (int k = 0; k < 60; k++) {  // random admissible codes, heads and data lengths
        const uint32_t dc = 2 + rng() % 12, dv = 1 + rng() % 5, n = dc * (1 + rng() % 300);
        if (n < 2 || (size_t)n * dv > lp::kMaxEdges) continue;
        const Code c = banded(n, dv, dc);
        const uint32_t head = rng() % n, N = 1 + rng() % (n - head > 8192 ? 8192 : n - head), D = 1 + rng() % n;
        lp::Config q = config(c, head, N, D);
        q.max_iters = 1 + rng() % 8, q.a = 1 + rng() % 16, q.beta = rng() % 3;
        const lp::Geom g = plan_of(c, q, t);
        emulate(c, q, g, t, 5 + rng() % 30);
    }
    {  // the largest frame: n = 16384, E = 65536
        const Code c = banded(16384, 4, 8);
        const lp::Geom g = lp::geom(config(c, 100, 8192));
        CHECK(g.form == lp::kFormTablesCache && g.G == 1 && g.T == 1024 && g.frame_bytes == 32768 + 16384 + 65536);
    }
    printf("largest lds: %zu\n", largest);
    if (failures) return 1;
    printf("ldpc_plan ok\n");
    return 0;
}
