// viterbi_ref.cpp -- the restatement of the Viterbi decoder bank (include/hzsdr_viterbi.h) over csrc/hz_viterbi_math.h,
// state by state: one frame at a time, a metric per state in an array, a decision per state and step in a byte each, the
// traceback and the CRC bit by bit -- no lanes, no words, no tiles, no tables.  It computes the bytes the device must
// produce.
//
//   viterbi_ref run CASES OUT    CASES: records of
//                                  uint32 kind, K, n, gens[4], inv, pattern_bits, termination, D, C, poly, init, xorout;
//                                  uint64 pattern; float32 scale; int64 R, cap; int32 has_counts; (R uint32 counts);
//                                  R * cap dense frame slots: FB bytes each (hard bits) or N float32 each.
//                                OUT: per record R * cap * DB decoded bytes, then R * cap uint32 info; slots from
//                                  min(count, cap) up are zero.
//   viterbi_ref check SETS OUT   SETS: records of the fifteen uint32, the pattern and the scale.  OUT: per set int32
//                                  accepted (0 / 1), uint32 N, T (0 when refused).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_viterbi_math.h"
#include "hz_viterbi_plan.h"

using namespace hz;

static bool read_head(FILE *f, vp::Config &q) {
    uint32_t h[15];
    if (fread(h, 4, 15, f) != 15) return false;
    if (fread(&q.pattern, 8, 1, f) != 1 || fread(&q.scale, 4, 1, f) != 1) exit(3);
    q.kind = (int)h[0], q.K = h[1], q.n = h[2];
    for (int j = 0; j < 4; j++) q.gens[j] = h[3 + j];
    q.inv = h[7], q.Lp = h[8], q.term = (int)h[9], q.D = h[10], q.C = h[11], q.poly = h[12], q.init = h[13], q.xorout = h[14];
    return true;
}

static bool known(const vp::Config &q) { return (q.kind == vp::kBits || q.kind == vp::kSoftF32) && q.n <= vp::kMaxRate; }

// one frame: q[m] for every mother-code bit m (0: punctured) -> the decoded bits and info
static uint32_t decode(const vp::Config &c, uint32_t T, const std::vector<int> &q, std::vector<uint8_t> &u) {
    const uint32_t K = c.K, S = 1u << (K - 1), n = c.n;
    std::vector<uint32_t> metric(S, vm::kInf), next(S);
    std::vector<uint8_t> dec((size_t)T * S);
    metric[0] = 0;
    for (uint32_t t = 0; t < T; t++) {
        for (uint32_t s = 0; s < S; s++) {
            uint32_t cost[2];
            for (uint32_t b = 0; b < 2; b++) {
                const uint32_t e = vm::expected(vm::branch_reg(s, b, K), c.gens, n, c.inv);
                cost[b] = 0;
                for (uint32_t j = 0; j < n; j++) cost[b] += vm::position_cost(q[(size_t)t * n + j], (e >> j) & 1u);
            }
            dec[(size_t)t * S + s] = (uint8_t)vm::acs(metric[vm::predecessor(s, 0, S)], cost[0], metric[vm::predecessor(s, 1, S)], cost[1], &next[s]);
        }
        metric.swap(next);
    }
    uint32_t s = 0;
    if (c.term == vp::kTruncated)
        for (uint32_t k = 1; k < S; k++)
            if (metric[k] < metric[s]) s = k;
    const uint32_t fin = metric[s];
    u.assign(T, 0);
    for (uint32_t t = T; t-- > 0;) {
        u[t] = (uint8_t)vm::input_of(s, K);
        s = vm::predecessor(s, dec[(size_t)t * S + s], S);
    }
    uint32_t ok = 0;
    if (c.C) {
        const uint32_t D = (uint32_t)c.D;
        uint32_t reg = c.init, sent = 0;
        for (uint32_t k = 0; k < D - c.C; k++) reg = vm::crc_step(reg, u[k], c.C, c.poly);
        reg ^= c.xorout;
        for (uint32_t k = D - c.C; k < D; k++) sent = (sent << 1) | u[k];
        ok = reg == sent;
    }
    return fin | (ok << 31);
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    vp::Config c;
    while (read_head(f, c)) {
        int64_t dim[2];
        int32_t has_counts;
        if (fread(dim, 8, 2, f) != 2 || fread(&has_counts, 4, 1, f) != 1) return 3;
        const int64_t R = dim[0], cap = dim[1];
        if (!known(c) || vp::check_config(c) || R < 1 || cap < 1) return 6;
        const vp::Geom g = vp::geom(c);
        const uint32_t T = g.T, n = c.n, D = (uint32_t)c.D;
        std::vector<uint32_t> counts((size_t)R, (uint32_t)cap);
        if (has_counts && fread(counts.data(), 4, R, f) != (size_t)R) return 3;
        const size_t slot = c.kind == vp::kBits ? g.FB : (size_t)g.N * 4;
        std::vector<uint8_t> in((size_t)R * cap * slot);
        if (fread(in.data(), 1, in.size(), f) != in.size()) return 3;
        std::vector<uint8_t> out((size_t)R * cap * g.DB, 0), u;
        std::vector<uint32_t> info((size_t)R * cap, 0);
        std::vector<int> q((size_t)T * n);
        for (int64_t r = 0; r < R; r++) {
            for (int64_t fr = 0; fr < cap && fr < (int64_t)counts[r]; fr++) {
                const uint8_t *src = in.data() + ((size_t)r * cap + fr) * slot;
                uint32_t at = 0;  // the puncture walk, bit by bit
                for (uint32_t m = 0; m < T * n; m++) {
                    q[m] = 0;
                    if (!vm::transmitted(c.pattern, c.Lp, m)) continue;
                    if (c.kind == vp::kBits) {
                        q[m] = vm::hard(vm::packed_bit(src, at));
                    } else {
                        float x;
                        memcpy(&x, src + 4 * (size_t)at, 4);
                        q[m] = vm::quantise(x, c.scale);
                    }
                    at++;
                }
                if (at != g.N) return 7;
                info[(size_t)r * cap + fr] = decode(c, T, q, u);
                uint8_t *dst = out.data() + ((size_t)r * cap + fr) * g.DB;
                for (uint32_t k = 0; k < D; k++)
                    if (u[k]) dst[k / 8] |= (uint8_t)(0x80u >> (k % 8));
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
    vp::Config c;
    while (read_head(f, c)) {
        const int32_t ok = known(c) && vp::check_config(c) == nullptr;
        uint32_t nt[2] = {0, 0};
        if (ok) {
            const vp::Geom g = vp::geom(c);
            nt[0] = g.N, nt[1] = g.T;
        }
        fwrite(&ok, 4, 1, o);
        fwrite(nt, 4, 2, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: viterbi_ref run CASES OUT | check SETS OUT\n");
    return 64;
}
