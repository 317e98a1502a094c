// ldpc_ref.cpp -- the restatement of the LDPC decoder bank (include/hzsdr_ldpc.h) over csrc/hz_ldpc_math.h, edge by
// edge: one frame at a time, a message per edge and both generations of P in plain arrays, the three steps of an
// iteration one after the other as the header numbers them -- no threads, no tables by variable, no early bookkeeping.
// It computes the bytes the device must produce.
//
//   ldpc_ref run CASES OUT     CASES: records of
//                                uint32 kind, m, n, E, head, N, D, level, max_iters, a, beta; float32 scale;
//                                uint32 row_ptr[m + 1]; uint32 col[E]; int64 R, cap; int32 has_counts; (R uint32 counts);
//                                R * cap dense frame slots: FB bytes each (hard bits) or N float32 each.
//                              OUT: per record R * cap * DB decoded bytes, then R * cap uint32 info; slots from
//                                min(count, cap) up are zero.
//   ldpc_ref check SETS OUT    SETS: records of the eleven uint32 and the scale, then uint32 nrow, ncol and the two
//                                arrays of those lengths.  OUT: per set int32 accepted (0 / 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_ldpc_math.h"
#include "hz_ldpc_plan.h"

using namespace hz;

static bool read_head(FILE *f, lp::Config &q) {
    uint32_t h[11];
    if (fread(h, 4, 11, f) != 11) return false;
    if (fread(&q.scale, 4, 1, f) != 1) exit(3);
    q.kind = (int)h[0], q.m = h[1], q.n = h[2], q.E = h[3], q.head = h[4], q.N = h[5], q.D = h[6];
    q.level = h[7], q.max_iters = h[8], q.a = h[9], q.beta = h[10];
    return true;
}

static bool known(const lp::Config &q) { return q.kind == lp::kBits || q.kind == lp::kSoftF32; }

// one frame: q[v] for every variable -> hard[v], info
static uint32_t decode(const lp::Config &c, const std::vector<uint32_t> &row_ptr, const std::vector<uint32_t> &col, const std::vector<int> &q,
                       std::vector<uint8_t> &hard) {
    const uint32_t m = (uint32_t)c.m, n = (uint32_t)c.n, E = (uint32_t)c.E;
    std::vector<int> r(E, 0), t(E), P(q), next(n);
    auto unsatisfied = [&]() {
        uint32_t u = 0;
        for (uint32_t v = 0; v < n; v++) hard[v] = P[v] > 0;
        for (uint32_t k = 0; k < m; k++) {
            uint32_t par = 0;
            for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) par ^= hard[col[e]];
            u += par;
        }
        return u;
    };
    hard.assign(n, 0);
    uint32_t u = unsatisfied(), it = 0;
    while (u != 0 && it < c.max_iters) {
        it++;
        for (uint32_t k = 0; k < m; k++)
            for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) t[e] = lm::to_check(P[col[e]], r[e]);
        for (uint32_t k = 0; k < m; k++) {
            lm::Check ck = lm::check_start();
            for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) lm::check_take(ck, e - row_ptr[k], t[e]);
            const int s1 = lm::scaled(ck.m1, c.a, c.beta), s2 = lm::scaled(ck.m2, c.a, c.beta);
            for (uint32_t e = row_ptr[k]; e < row_ptr[k + 1]; e++) r[e] = lm::to_variable(ck, e - row_ptr[k], t[e], s1, s2);
        }
        for (uint32_t v = 0; v < n; v++) next[v] = q[v];
        for (uint32_t e = 0; e < E; e++) next[col[e]] += r[e];
        P.swap(next);
        u = unsatisfied();
    }
    return lm::info_word(u, it);
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    lp::Config c;
    while (read_head(f, c)) {
        if (!known(c) || lp::check_config(c)) return 6;
        std::vector<uint32_t> row_ptr(c.m + 1), col(c.E);
        if (fread(row_ptr.data(), 4, row_ptr.size(), f) != row_ptr.size() || fread(col.data(), 4, col.size(), f) != col.size()) return 3;
        if (lp::check_code(c, row_ptr.data(), col.data())) return 6;
        int64_t dim[2];
        int32_t has_counts;
        if (fread(dim, 8, 2, f) != 2 || fread(&has_counts, 4, 1, f) != 1) return 3;
        const int64_t R = dim[0], cap = dim[1];
        if (R < 1 || cap < 1) return 6;
        const uint32_t n = (uint32_t)c.n, N = (uint32_t)c.N, D = (uint32_t)c.D, head = (uint32_t)c.head, FB = (N + 7) / 8, DB = (D + 7) / 8;
        std::vector<uint32_t> counts((size_t)R, (uint32_t)cap);
        if (has_counts && fread(counts.data(), 4, R, f) != (size_t)R) return 3;
        const size_t slot = c.kind == lp::kBits ? FB : (size_t)N * 4;
        std::vector<uint8_t> in((size_t)R * cap * slot);
        if (fread(in.data(), 1, in.size(), f) != in.size()) return 3;
        std::vector<uint8_t> out((size_t)R * cap * DB, 0), hard;
        std::vector<uint32_t> info((size_t)R * cap, 0);
        std::vector<int> q(n);
        for (int64_t r = 0; r < R; r++) {
            for (int64_t fr = 0; fr < cap && fr < (int64_t)counts[r]; fr++) {
                const uint8_t *src = in.data() + ((size_t)r * cap + fr) * slot;
                for (uint32_t v = 0; v < n; v++) q[v] = 0;
                for (uint32_t i = 0; i < N; i++) {
                    if (c.kind == lp::kBits) {
                        q[head + i] = lm::hard(lm::packed_bit(src, i), (int)c.level);
                    } else {
                        float x;
                        memcpy(&x, src + 4 * (size_t)i, 4);
                        q[head + i] = lm::quantise(x, c.scale);
                    }
                }
                info[(size_t)r * cap + fr] = decode(c, row_ptr, col, q, hard);
                uint8_t *dst = out.data() + ((size_t)r * cap + fr) * DB;
                for (uint32_t k = 0; k < D; k++)
                    if (hard[k]) dst[k / 8] |= (uint8_t)(0x80u >> (k % 8));
            }
        }
        fwrite(out.data(), 1, out.size(), o);
        fwrite(info.data(), 4, info.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int check(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    lp::Config c;
    while (read_head(f, c)) {
        uint32_t len[2];
        if (fread(len, 4, 2, f) != 2) return 3;
        std::vector<uint32_t> row_ptr(len[0]), col(len[1]);
        if (fread(row_ptr.data(), 4, len[0], f) != len[0] || fread(col.data(), 4, len[1], f) != len[1]) return 3;
        int32_t ok = known(c) && lp::check_config(c) == nullptr && len[0] == c.m + 1 && len[1] == c.E;
        if (ok) ok = lp::check_code(c, row_ptr.data(), col.data()) == nullptr;
        fwrite(&ok, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: ldpc_ref run CASES OUT | check SETS OUT\n");
    return 64;
}
