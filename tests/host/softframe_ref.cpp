// softframe_ref.cpp -- the restatement of the soft frame bank (include/hzsdr_softframe.h) over csrc/hz_softframe_plan.h,
// push by push and float by float, with the history carried as the bank carries it: no lanes, no pairs.  It computes
// the bytes the device must produce.
//
//   softframe_ref run CASES OUT   CASES: records of
//                                   int32 cplx, B, P, H, maps[4], has_state, pushes;  int64 R, cap;
//                                   (has_state: R uint64 positions, R * HF float32 history)
//                                   per push: int64 n; int32 has_counts; (R uint32 in_counts); R * n symbols, dense;
//                                             (cap > 0: R uint32 counts; R * cap uint64 positions; R * cap uint32 info)
//                                 OUT: per push R * cap * P uint32 floats and R * cap uint32 status, 0xA5A5A5A5 in every
//                                   slot from min(counts, cap) up; then R uint64 positions, R * HF float32 history.
//   softframe_ref check SETS OUT  SETS: records of the first ten int32.  OUT: per set int32 accepted (0 / 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hz_softframe_plan.h"

using namespace hz;

static void need(bool ok) {
    if (!ok) exit(3);
}

static const uint32_t kSentinel = 0xA5A5A5A5u;

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 2;
    const bool run = !strcmp(argv[1], "run");
    if (!run && strcmp(argv[1], "check")) return 2;
    int32_t h[10];
    while (fread(h, 4, 10, in) == 10u) {
        sfp::Config q{h[0] ? sfp::kC64 : sfp::kRealF32, (uint32_t)h[1], (uint32_t)h[2], (uint32_t)h[3],
                      {(uint32_t)h[4], (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7]}};
        const char *why = sfp::check_config(q);
        if (!run) {
            const int32_t ok = why ? 0 : 1;
            fwrite(&ok, 4, 1, out);
            continue;
        }
        need(!why);
        const sfp::Geom g = sfp::geom(q);
        int64_t R, cap;
        need(fread(&R, 8, 1, in) == 1 && fread(&cap, 8, 1, in) == 1);
        std::vector<uint64_t> pos((size_t)R, 0);
        std::vector<uint32_t> hist((size_t)R * g.HF, 0), next(hist.size());
        if (h[8]) {
            need(fread(pos.data(), 8, (size_t)R, in) == (size_t)R);
            if (!hist.empty()) need(fread(hist.data(), 4, hist.size(), in) == hist.size());
        }
        for (int32_t p = 0; p < h[9]; p++) {
            int64_t n;
            int32_t has_counts;
            need(fread(&n, 8, 1, in) == 1 && fread(&has_counts, 4, 1, in) == 1);
            std::vector<uint32_t> in_counts((size_t)R, 0), counts((size_t)R, 0), info((size_t)(R * cap));
            std::vector<uint64_t> positions((size_t)(R * cap));
            if (has_counts) need(fread(in_counts.data(), 4, (size_t)R, in) == (size_t)R);
            const size_t row_floats = (size_t)n * g.sym_floats;
            std::vector<uint32_t> x((size_t)R * row_floats);
            if (!x.empty()) need(fread(x.data(), 4, x.size(), in) == x.size());
            if (cap) {
                need(fread(counts.data(), 4, (size_t)R, in) == (size_t)R);
                need(fread(positions.data(), 8, positions.size(), in) == positions.size());
                need(fread(info.data(), 4, info.size(), in) == info.size());
            }
            const char *bad = nullptr;
            need(sfp::check_call(q, {(uint64_t)n, (uint64_t)n, (uint64_t)cap, (uint64_t)cap * q.P, (uint64_t)R, true, true, true, true, true, true}, &bad) == sfp::kOk);
            std::vector<uint32_t> y((size_t)(R * cap) * q.P, kSentinel), status((size_t)(R * cap), kSentinel);
            for (int64_t r = 0; r < R; r++) {
                const uint64_t c = sfp::consumed(has_counts ? in_counts[(size_t)r] : (uint64_t)n, (uint64_t)n);
                const uint64_t p0 = pos[(size_t)r], p1 = p0 + c;
                const uint32_t *hr = hist.data() + (size_t)r * g.HF, *xr = x.data() + (size_t)r * row_floats;
                auto line = [&](uint64_t v) {
                    if (sfp::in_history(v, g.HF)) return hr[v];
                    const uint64_t at = sfp::input_float(v, g.HF, g.in_step);
                    need(at < c * g.sym_floats);  // nothing outside what the row consumes
                    return xr[at];
                };
                for (int64_t f = 0; f < cap && f < (int64_t)counts[(size_t)r]; f++) {
                    const size_t slot = (size_t)(r * cap + f);
                    const uint32_t hyp = (info[slot] >> 8) & 0xffu;
                    const uint32_t st = sfp::window_status(positions[slot], hyp, q.H, p0, p1, g.Kh);
                    status[slot] = st;
                    uint32_t *dst = y.data() + slot * q.P;
                    if (st != sfp::kServed) {
                        for (uint32_t k = 0; k < q.P; k++) dst[k] = sfp::kQuietNaN;
                        continue;
                    }
                    const uint64_t v0 = sfp::line_start(positions[slot], p0, g.Kh, q.B);
                    const uint32_t map = q.maps[hyp];
                    for (uint32_t k = 0; k < q.P; k++) dst[k] = line(v0 + sfp::map_source(k, map, q.B)) ^ sfp::map_flip(k, map, q.B);
                }
                if (n) {  // (a push with n = 0 launches no carry; a row with c = 0 carries its history over as it is)
                    for (uint32_t j = 0; j < g.HF; j++) next[(size_t)r * g.HF + j] = line(sfp::carried_float(c, q.B, j));
                    pos[(size_t)r] = p1;
                }
            }
            if (n) hist.swap(next);
            fwrite(y.data(), 4, y.size(), out);
            fwrite(status.data(), 4, status.size(), out);
        }
        fwrite(pos.data(), 8, pos.size(), out);
        fwrite(hist.data(), 4, hist.size(), out);
    }
    fclose(in);
    return fclose(out) ? 4 : 0;
}
