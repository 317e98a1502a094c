// hdlc_ref.cpp -- the restatement of the HDLC deframer bank (include/hzsdr_hdlc.h) over csrc/hz_hdlc_math.h, bit by bit:
// one decision, one differential step, one 8-bit window, and at a flag behind a flag the span walked bit by bit through
// the stuffed test and the FCS register -- no words, no ring, no tiles, no lanes.  It computes the bytes the device must
// produce.
//
//   hdlc_ref run CASES OUT   CASES: records of
//                              int32 complex (0 / 1), diff, fcs, min_bytes, max_bytes, msb_first, keep_bad, has_state, pushes;
//                              int64 R, cap;
//                              when has_state: R uint64 positions, R uint64 events, R bytes of kinds, R * ceil(K / 8)
//                              history bytes, R bytes of last raw decisions (else the state of create);
//                              per push: int64 n, int32 has_counts, (R uint32 counts), R dense rows of n float32 (real)
//                              or (re, im) pairs (complex).
//                            OUT: per push R * cap * max_bytes frame bytes, R * cap uint64 positions, R * cap uint32 info
//                              (unused slots and slot tails zero), R uint32 counts; behind a record's pushes its state
//                              in the form above.
//   hdlc_ref check SETS OUT  SETS: records of the nine int32 (has_state and pushes 0).  OUT: per set int32 accepted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_hdlc_math.h"
#include "hz_hdlc_plan.h"

using namespace hz;

struct Row {
    uint64_t bits = 0, evend = 0;
    uint32_t evkind = hp::kEvAbort, last = 0;
    std::vector<uint8_t> tail;  // the last K bits, oldest first
};

struct Head {
    int32_t cplx, diff, fcs, min_bytes, max_bytes, msb_first, keep_bad, has_state, pushes;
};

static bool negative(const Head &h) { return h.diff < 0 || h.fcs < 0 || h.min_bytes < 0 || h.max_bytes < 0 || h.msb_first < 0 || h.keep_bad < 0; }
static hp::Config config(const Head &h) {
    return hp::Config{h.cplx ? hp::kC64 : hp::kRealF32, (uint32_t)h.diff, (uint32_t)h.fcs, (uint32_t)h.min_bytes, (uint32_t)h.max_bytes,
                      (uint32_t)h.msb_first, (uint32_t)h.keep_bad};
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    Head h;
    while (fread(&h, 4, 9, f) == 9) {
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], cap = dim[1];
        if (negative(h)) return 6;
        const hp::Config q = config(h);
        if (hp::check_config(q) || R < 1 || cap < 0) return 6;
        const uint32_t Lmax = hp::span_max(q.max_bytes), K = Lmax + 8, MB = q.max_bytes;
        const size_t hb = hp::history_bytes(K), width = h.cplx ? 2 : 1;
        std::vector<Row> rows((size_t)R);
        for (auto &r : rows) r.tail.assign(K, 0);
        if (h.has_state) {
            std::vector<uint64_t> pos((size_t)R), ev((size_t)R);
            std::vector<uint8_t> kinds((size_t)R), hist((size_t)R * hb), last((size_t)R);
            if (fread(pos.data(), 8, R, f) != (size_t)R || fread(ev.data(), 8, R, f) != (size_t)R || fread(kinds.data(), 1, R, f) != (size_t)R ||
                fread(hist.data(), 1, hist.size(), f) != hist.size() || fread(last.data(), 1, R, f) != (size_t)R)
                return 3;
            for (int64_t r = 0; r < R; r++) {
                rows[r].bits = pos[r], rows[r].evend = ev[r], rows[r].evkind = kinds[r] & 1u, rows[r].last = last[r] & 1u;
                for (uint32_t k = 0; k < K; k++) rows[r].tail[k] = (hist[r * hb + k / 8] >> (7 - k % 8)) & 1u;
            }
        }
        for (int p = 0; p < h.pushes; p++) {
            int64_t n;
            int32_t has_counts;
            if (fread(&n, 8, 1, f) != 1 || fread(&has_counts, 4, 1, f) != 1 || n < 0) return 3;
            std::vector<uint32_t> ic((size_t)R, (uint32_t)n);
            if (has_counts && fread(ic.data(), 4, R, f) != (size_t)R) return 3;
            std::vector<uint32_t> x((size_t)R * n * width);
            if (fread(x.data(), 4, x.size(), f) != x.size()) return 3;
            std::vector<uint8_t> frames((size_t)R * cap * MB, 0);
            std::vector<uint64_t> positions((size_t)R * cap, 0);
            std::vector<uint32_t> info((size_t)R * cap, 0), counts((size_t)R, 0);
            std::vector<uint8_t> bits;
            for (int64_t r = 0; r < R; r++) {
                Row &z = rows[r];
                const uint64_t take = ic[r] < (uint64_t)n ? ic[r] : (uint64_t)n;
                const uint32_t *xr = x.data() + (size_t)r * n * width;
                for (uint64_t i = 0; i < take; i++) {
                    const uint32_t d = fm::decide(xr[i * width]);
                    const uint32_t b = fm::diff_bit(d, z.last, (int)q.diff);
                    z.last = d;
                    z.tail.erase(z.tail.begin());
                    z.tail.push_back((uint8_t)b);  // the K bits that end at this one
                    const uint64_t end = ++z.bits;  // this bit's number plus one
                    uint32_t window = 0;
                    for (uint32_t k = 0; k < 8; k++) window |= (uint32_t)z.tail[K - 8 + k] << k;
                    const bool flag = hm::is_flag(window), abort_ = hm::is_abort(window);
                    if (!flag && !abort_) continue;
                    const uint64_t from = z.evend, dist = end - z.evend;
                    const bool pair = flag && z.evkind == hp::kEvFlag;
                    z.evkind = flag ? hp::kEvFlag : hp::kEvAbort, z.evend = end;
                    if (!pair || dist <= 8 || dist - 8 > Lmax) continue;
                    const uint32_t L = (uint32_t)dist - 8;
                    const uint8_t *span = &z.tail[K - 8 - L];  // b[e1+1 ... e2-8]
                    bits.clear();
                    for (uint32_t k = 0; k < L; k++) {
                        uint32_t before = 0;
                        for (uint32_t s = 0; s < 5; s++) before |= (k + s >= 5 ? (uint32_t)span[k + s - 5] : 0u) << s;
                        if (!hm::is_stuffed(span[k], before)) bits.push_back(span[k]);
                    }
                    const uint32_t u = (uint32_t)bits.size();
                    if (!hp::well_formed(u, q.min_bytes, q.max_bytes)) continue;
                    uint32_t good = 1;
                    if (q.fcs) {
                        uint32_t c = hm::fcs_init(q.fcs);
                        for (uint8_t bit : bits) c = hm::fcs_step(c, bit, hm::fcs_poly(q.fcs));
                        good = c == hm::fcs_good(q.fcs);
                    }
                    if (!q.keep_bad && !good) continue;
                    const uint32_t fidx = counts[r]++;
                    if ((int64_t)fidx < cap) {
                        uint8_t *dst = frames.data() + ((size_t)r * cap + fidx) * MB;
                        for (uint32_t k = 0; k < u; k++)
                            if (bits[k]) dst[k / 8] |= (uint8_t)(q.msb_first ? 0x80u >> (k % 8) : 1u << (k % 8));
                        positions[(size_t)r * cap + fidx] = from;
                        info[(size_t)r * cap + fidx] = (u / 8) | (good << 31);
                    }
                }
            }
            fwrite(frames.data(), 1, frames.size(), o);
            fwrite(positions.data(), 8, positions.size(), o);
            fwrite(info.data(), 4, info.size(), o);
            fwrite(counts.data(), 4, counts.size(), o);
        }
        for (int64_t r = 0; r < R; r++) fwrite(&rows[r].bits, 8, 1, o);
        for (int64_t r = 0; r < R; r++) fwrite(&rows[r].evend, 8, 1, o);
        for (int64_t r = 0; r < R; r++) {
            const uint8_t k = (uint8_t)rows[r].evkind;
            fwrite(&k, 1, 1, o);
        }
        for (int64_t r = 0; r < R; r++) {
            std::vector<uint8_t> bytes(hb, 0);
            for (uint32_t k = 0; k < K; k++)
                if (rows[r].tail[k]) bytes[k / 8] |= (uint8_t)(0x80u >> (k % 8));
            fwrite(bytes.data(), 1, hb, o);
        }
        for (int64_t r = 0; r < R; r++) {
            const uint8_t l = (uint8_t)rows[r].last;
            fwrite(&l, 1, 1, o);
        }
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

static int check(const char *sets, const char *outp) {
    FILE *f = fopen(sets, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    Head h;
    while (fread(&h, 4, 9, f) == 9) {
        const int32_t ok = !negative(h) && hp::check_config(config(h)) == nullptr;
        fwrite(&ok, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: hdlc_ref run CASES OUT | check SETS OUT\n");
    return 64;
}
