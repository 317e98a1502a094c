// framesync_ref.cpp -- the restatement of the frame sync bank (include/hzsdr_framesync.h) over csrc/hz_framesync_math.h,
// bit by bit: one decision, one differential step, one window compared bit for bit, one payload bit through its map at a
// time -- no words, no ring, no tiles.  It computes the bytes the device must produce.
//
//   framesync_ref run CASES OUT   CASES: records of
//                                   int32 complex (0 / 1), B, W, thr, H, P, diff, has_state, pushes;
//                                   uint64 mask, holdoff, words[4]; uint32 maps[4]; int64 R, cap;
//                                   when has_state: R uint64 positions, R uint64 holds, R * ceil(K / 8) history bytes,
//                                   R bytes of last raw decisions (else the state of create);
//                                   per push: int64 n, int32 has_counts, (R uint32 counts), R dense rows of n float32
//                                   (real) or (re, im) pairs (complex).
//                                 OUT: per push R * cap * FB frame bytes, R * cap uint64 positions, R * cap uint32 info
//                                   (unused slots zero), R uint32 counts; behind a record's pushes its state in the
//                                   form above.
//   framesync_ref check SETS OUT  SETS: records of the configuration as above (the nine int32 with has_state and pushes
//                                   0, mask, holdoff, words, maps).  OUT: per set int32 accepted (0 / 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_framesync_math.h"
#include "hz_framesync_plan.h"

using namespace hz;

struct Row {
    uint64_t bits = 0, hold = 0;  // bits consumed, the hold-off in symbols
    uint32_t last = 0;
    std::vector<uint8_t> tail;  // the last K bits, oldest first
};

struct Head {
    int32_t cplx, B, W, thr, H, P, diff, has_state, pushes;
    uint64_t mask, holdoff, words[4];
    uint32_t maps[4];
};

static bool read_head(FILE *f, Head &h) {
    if (fread(&h.cplx, 4, 9, f) != 9) return false;
    if (fread(&h.mask, 8, 1, f) != 1 || fread(&h.holdoff, 8, 1, f) != 1 || fread(h.words, 8, 4, f) != 4 || fread(h.maps, 4, 4, f) != 4) exit(3);
    return true;
}

static fp::Config config(const Head &h) {
    fp::Config q{h.cplx ? fp::kC64 : fp::kRealF32, (uint32_t)h.B, (uint32_t)h.W, h.mask, (uint32_t)h.thr, (uint32_t)h.H, {0, 0, 0, 0}, {0, 0, 0, 0},
                 (uint32_t)h.P, (uint32_t)h.diff, h.holdoff};
    for (int k = 0; k < 4; k++) q.words[k] = h.words[k], q.maps[k] = h.maps[k];
    return q;
}

// bit k (0: the first received) of a W-bit word given most significant bit first
static uint32_t word_bit(uint64_t w, uint32_t W, uint32_t k) { return (uint32_t)(w >> (W - 1 - k)) & 1u; }

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    Head h;
    while (read_head(f, h)) {
        int64_t dim[2];
        if (fread(dim, 8, 2, f) != 2) return 3;
        const int64_t R = dim[0], cap = dim[1];
        const fp::Config q = config(h);
        if (fp::check_config(q) || R < 1 || cap < 0) return 6;
        const uint32_t B = q.B, W = q.W, P = q.P, K = W + P - 1, FB = (P + 7) / 8;
        const size_t hb = fp::history_bytes(K), width = h.cplx ? 2 : 1, step = h.cplx && B == 1 ? 2 : 1;
        std::vector<Row> rows((size_t)R);
        for (auto &r : rows) r.tail.assign(K, 0);
        if (h.has_state) {
            std::vector<uint64_t> pos((size_t)R), hold((size_t)R);
            std::vector<uint8_t> hist((size_t)R * hb), last((size_t)R);
            if (fread(pos.data(), 8, R, f) != (size_t)R || fread(hold.data(), 8, R, f) != (size_t)R || fread(hist.data(), 1, hist.size(), f) != hist.size() ||
                fread(last.data(), 1, R, f) != (size_t)R)
                return 3;
            for (int64_t r = 0; r < R; r++) {
                rows[r].bits = pos[r] * B, rows[r].hold = hold[r], rows[r].last = last[r] & 1u;
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
            std::vector<uint8_t> frames((size_t)R * cap * FB, 0);
            std::vector<uint64_t> positions((size_t)R * cap, 0);
            std::vector<uint32_t> info((size_t)R * cap, 0), counts((size_t)R, 0);
            for (int64_t r = 0; r < R; r++) {
                Row &z = rows[r];
                const uint64_t take = ic[r] < (uint64_t)n ? ic[r] : (uint64_t)n, m = take * B;
                const uint32_t *xr = x.data() + (size_t)r * n * width;
                for (uint64_t i = 0; i < m; i++) {
                    const uint32_t d = fm::decide(xr[i * step]);
                    const uint32_t b = fm::diff_bit(d, z.last, (int)q.diff);
                    z.last = d;
                    z.tail.push_back((uint8_t)b);  // K + 1 bits: the window, then the payload, of the frame that completes here
                    const uint64_t g = z.bits++;   // this bit's number
                    if (g >= K && (g + 1 - P) % B == 0) {
                        uint32_t best = 65, bh = 0;
                        for (uint32_t hh = 0; hh < q.H; hh++) {
                            uint32_t dist = 0;
                            for (uint32_t k = 0; k < W; k++)
                                if (word_bit(q.mask, W, k) && z.tail[k] != word_bit(q.words[hh], W, k)) dist++;
                            if (dist < best) best = dist, bh = hh;
                        }
                        const uint64_t s = (g + 1 - P) / B;
                        if (best <= q.thr && s >= z.hold) {
                            z.hold = s + q.holdoff;
                            const uint32_t fidx = counts[r]++;
                            if ((int64_t)fidx < cap) {
                                uint8_t *dst = frames.data() + ((size_t)r * cap + fidx) * FB;
                                for (uint32_t k = 0; k < P; k += B) {
                                    const uint8_t *pb = &z.tail[W + k];
                                    if (B == 1) {
                                        if (fm::map_bit(pb[0], (int)q.maps[bh])) dst[k / 8] |= (uint8_t)(0x80u >> (k % 8));
                                    } else {
                                        const uint32_t dd = fm::map_dibit(pb[0] | (pb[1] << 1), (int)q.maps[bh]);
                                        if (dd & 1u) dst[k / 8] |= (uint8_t)(0x80u >> (k % 8));
                                        if (dd & 2u) dst[(k + 1) / 8] |= (uint8_t)(0x80u >> ((k + 1) % 8));
                                    }
                                }
                                positions[(size_t)r * cap + fidx] = s;
                                info[(size_t)r * cap + fidx] = best | (bh << 8);
                            }
                        }
                    }
                    z.tail.erase(z.tail.begin());
                }
            }
            fwrite(frames.data(), 1, frames.size(), o);
            fwrite(positions.data(), 8, positions.size(), o);
            fwrite(info.data(), 4, info.size(), o);
            fwrite(counts.data(), 4, counts.size(), o);
        }
        for (int64_t r = 0; r < R; r++) {
            const uint64_t pos = rows[r].bits / B;
            fwrite(&pos, 8, 1, o);
        }
        for (int64_t r = 0; r < R; r++) fwrite(&rows[r].hold, 8, 1, o);
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
    while (read_head(f, h)) {
        const int32_t ok = h.B >= 0 && h.W >= 0 && h.thr >= 0 && h.H >= 0 && h.P >= 0 && h.diff >= 0 && fp::check_config(config(h)) == nullptr;
        fwrite(&ok, 4, 1, o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "check")) return check(argv[2], argv[3]);
    fprintf(stderr, "usage: framesync_ref run CASES OUT | check SETS OUT\n");
    return 64;
}
