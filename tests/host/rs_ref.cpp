// rs_ref.cpp -- the restatement of the Reed-Solomon decoder bank (include/hzsdr_rs.h) over csrc/hz_rs_math.h, one
// codeword at a time and one element after the other (rsm::decode_word): no lanes, no ballots, no LDS.  It computes the
// bytes the device must produce.
//
//   rs_ref run CASES OUT     CASES: records of
//                              uint32 gfpoly, fcr, prim, nroots, n, interleave, scramble_len, has_in_map, has_out_map;
//                              (256 bytes in_map) (256 bytes out_map) (scramble_len bytes);
//                              int64 R, cap; int32 has_counts; (R uint32 counts); R * cap dense frames of F = I n bytes.
//                            OUT: per record R * cap * I k data bytes, then R * cap uint32 info; slots from
//                              min(count, cap) up are zero.
//   rs_ref check SETS OUT    SETS: records of the first seven uint32.  OUT: per set uint32 accepted (0 / 1), k, t
//                              (0 when refused).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_rs_math.h"
#include "hz_rs_plan.h"

using namespace hz;

static void need(bool ok) {
    if (!ok) exit(3);
}

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const bool run = !strcmp(argv[1], "run");
    if (!run && strcmp(argv[1], "check")) return 2;
    uint32_t h[9];
    while (fread(h, 4, run ? 9 : 7, in) == (run ? 9u : 7u)) {
        const rsp::Config q{h[0], h[1], h[2], h[3], h[4], h[5], h[6]};
        const char *why = rsp::check_config(q);
        if (!run) {
            uint32_t o[3] = {why ? 0u : 1u, 0, 0};
            if (!why) o[1] = rsp::geom(q).k, o[2] = rsp::geom(q).t;
            fwrite(o, 4, 3, out);
            continue;
        }
        need(!why);
        const rsp::Geom g = rsp::geom(q);
        std::vector<uint8_t> imap(256), omap(256), scr(q.scramble_len);
        if (h[7]) need(fread(imap.data(), 1, 256, in) == 256);
        if (h[8]) need(fread(omap.data(), 1, 256, in) == 256);
        if (q.scramble_len) need(fread(scr.data(), 1, q.scramble_len, in) == q.scramble_len);
        int64_t R, cap;
        int32_t has_counts;
        need(fread(&R, 8, 1, in) == 1 && fread(&cap, 8, 1, in) == 1 && fread(&has_counts, 4, 1, in) == 1);
        std::vector<uint32_t> counts((size_t)R, (uint32_t)cap);
        if (has_counts) need(fread(counts.data(), 4, (size_t)R, in) == (size_t)R);
        std::vector<uint8_t> frames((size_t)(R * cap) * g.F), data((size_t)(R * cap) * g.IK, 0);
        need(fread(frames.data(), 1, frames.size(), in) == frames.size());
        std::vector<uint32_t> info((size_t)(R * cap), 0);
        uint8_t exp[rsm::kExpSize], log[rsm::kLogSize];
        need(rsm::build_tables(q.gfpoly, exp, log));
        const rsm::Code c{q.gfpoly, q.fcr, q.prim, q.nroots, q.n};
        for (int64_t r = 0; r < R; r++) {
            for (int64_t f = 0; f < cap && f < (int64_t)counts[(size_t)r]; f++) {
                uint8_t *v = frames.data() + (size_t)(r * cap + f) * g.F;
                for (uint32_t m = 0; m < g.F; m++) {
                    uint8_t b = v[m];
                    if (q.scramble_len) b ^= scr[m % q.scramble_len];
                    v[m] = h[7] ? imap[b] : b;
                }
                uint32_t E = 0, nfail = 0;
                for (uint32_t i = 0; i < q.interleave; i++) {
                    const int e = rsm::decode_word(c, exp, log, v + i, q.interleave);
                    if (e < 0)
                        nfail++;
                    else
                        E += (uint32_t)e;
                }
                uint8_t *d = data.data() + (size_t)(r * cap + f) * g.IK;
                for (uint32_t m = 0; m < g.IK; m++) d[m] = h[8] ? omap[v[m]] : v[m];
                info[(size_t)(r * cap + f)] = E | nfail << 16 | (nfail ? 0u : 1u << 31);
            }
        }
        fwrite(data.data(), 1, data.size(), out);
        fwrite(info.data(), 4, info.size(), out);
    }
    fclose(in);
    return fclose(out) ? 4 : 0;
}
