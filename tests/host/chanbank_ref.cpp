// chanbank_ref.cpp -- the bit-exact restatement of the channel bank (include/hzsdr_chanbank.h), twice over
// csrc/hz_chanbank_math.h, the header the kernel takes the fold's term from.  Built with g++ -O2 -ffp-contract=off, it
// computes the bits the device must produce.
//   (a) The contract evaluated directly: per frame the fold, then per channel the chain of four fused steps per r.
//   (b) A host transcription of the kernel's indexing: the stream cut into the record's pushes, per push the counts of
//       csrc/hz_chanbank_plan.h, per tile A and B filled through the planner's layout functions (held ++ in, the
//       rotation applied to the load indices, dead frames and padding +0) and the 16x16x4 product evaluated as the
//       k-ordered chain of fused multiply-adds, 16-row tile by 16-column tile.
// The two must agree bit for bit: the program fails (exit 5) where they do not.
//
//   chanbank_ref run CASES OUT
//       CASES: records of int32 M, P, D, given, cuts; int64 N; P*M float32 taps; where given = 1 the table as read out
//              of the library, M rows of Mp complex64, and where given = 0 nothing: the program makes it by its OWN copy
//              of step 2 (below, not the planner's); N complex64 samples (already converted); `cuts` int64 stream
//              positions, ascending, at which the stream is cut into pushes (a position may repeat: an empty push).
//       OUT:   per record int64 F, then F rows of M complex64 (frame-major, ZeroFirst) of the whole stream, then the
//              M * Mp table entries that were used.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hz_chanbank_math.h"
#include "hz_chanbank_plan.h"

using namespace hz;
using cb::c32;

// ---- step 2, this program's own copy -------------------------------------------------------------------
// W[k][r] of phase n = (k r) mod M: the octant of 8 n / M in integers, float64 cos and sin of the angle from the
// nearest axis below pi/4
static c32 own_table(int64_t n, int64_t M) {
    const double half_pi = 1.5707963267948966192313216916398;
    const int64_t quad = 4 * n / M, p = 4 * n % M;
    const bool mirror = 2 * p > M;
    const double t = (double)(mirror ? M - p : p) * half_pi / (double)M;
    double a = cos(t), b = sin(t);
    if (p == 0) a = 1.0, b = 0.0;
    const double cr = mirror ? b : a, sr = mirror ? a : b;
    const double cs[4] = {cr, 0.0 - sr, 0.0 - cr, sr}, sn[4] = {sr, cr, 0.0 - sr, 0.0 - cr};
    return c32{(float)cs[quad], (float)(0.0 - sn[quad])};
}

static bool same(const c32 &a, const c32 &b) { return memcmp(&a, &b, sizeof a) == 0; }

// (a): the frames of the whole stream
static std::vector<c32> direct(int64_t M, int64_t P, int64_t D, const std::vector<float> &g, const std::vector<c32> &W, const std::vector<c32> &x) {
    const int64_t Mp = (M + 1) / 2 * 2, L = P * M, N = (int64_t)x.size();
    const int64_t F = N >= L ? (N - L) / D + 1 : 0;
    std::vector<c32> y(F * M), u(Mp);
    for (int64_t j = 0; j < F; j++) {
        for (int64_t r = 0; r < Mp; r++) {
            c32 acc{0.0f, 0.0f};
            if (r < M) {
                const int64_t o = ((r - j * D) % M + M) % M;
                for (int64_t p = 0; p < P; p++) acc = cb::chanbank_fold(acc, g[o + p * M], x[j * D + o + p * M]);
            }
            u[r] = acc;
        }
        for (int64_t k = 0; k < M; k++) {
            c32 acc{0.0f, 0.0f};
            for (int64_t r = 0; r < Mp; r++) acc = cb::chanbank_term(acc, W[k * Mp + r], u[r]);
            y[j * M + k] = acc;
        }
    }
    return y;
}

// (b): push by push, tile by tile, as the kernel indexes
static std::vector<c32> tiled(uint32_t M, uint32_t P, uint32_t D, const std::vector<float> &g, const std::vector<c32> &W, const std::vector<c32> &x,
                              const std::vector<int64_t> &cuts) {
    const cp::Geom geo = cp::chanbank_geom(M);
    const uint32_t L = P * M;
    const std::vector<float> A = cp::chanbank_fill_a(geo, W);
    const uint64_t magic = div_magic(M);
    std::vector<c32> y, tail;
    std::vector<float> B(geo.b_floats);
    cp::State st{};
    int64_t at = 0;
    for (size_t c = 0; c <= cuts.size(); c++) {
        const int64_t end = c < cuts.size() ? cuts[c] : (int64_t)x.size();
        const c32 *in = x.data() + at;
        const uint64_t n = (uint64_t)(end - at);
        const cp::Step p = cp::chanbank_step(st, M, L, D, n);
        if (!p.ok) return {};
        auto sample = [&](uint64_t v) { return v < st.held ? tail[v] : in[v - st.held]; };
        const size_t y0 = y.size();
        y.resize(y0 + p.F * M);
        for (uint64_t tile = 0; tile * geo.T < p.F; tile++) {
            const uint64_t f0 = tile * geo.T;
            const uint32_t rot0 = cp::chanbank_rot(st.rot, f0, D, M);
            for (uint32_t fl = 0; fl < geo.T; fl++) {
                const uint64_t f = f0 + fl;
                const uint32_t w = rot0 + fl * D, s = w - div_by_magic(w, magic) * M;
                for (uint32_t r = 0; r < geo.Mp; r++) {
                    c32 acc{0.0f, 0.0f};
                    if (f < p.F && r < M) {
                        uint32_t o = cp::chanbank_offset(r, s, M);
                        for (uint32_t q = 0; q < P; q++, o += M) acc = cb::chanbank_fold(acc, g[o], sample(f * D + o));
                    }
                    B[cp::chanbank_b_index(2 * r, fl, geo.pitch)] = acc.re;
                    B[cp::chanbank_b_index(2 * r + 1, fl, geo.pitch)] = acc.im;
                }
            }
            for (uint32_t rt = 0; rt < geo.row_tiles; rt++)
                for (uint32_t ct = 0; ct < geo.col_tiles; ct++) {
                    float acc[16][16] = {};
                    for (uint32_t s = 0; s < geo.steps; s++)
                        for (uint32_t k = 0; k < 4; k++) {  // (per output: k ascending inside s ascending)
                            float av[16], bv[16];
                            for (uint32_t i = 0; i < 16; i++) {
                                av[i] = A[cp::chanbank_a_index(rt * 16 + i, 4 * s + k, geo.steps)];
                                bv[i] = B[cp::chanbank_b_index(4 * s + k, ct * 16 + i, geo.pitch)];
                            }
                            for (uint32_t i = 0; i < 16; i++)
                                for (uint32_t j = 0; j < 16; j++) acc[i][j] = __builtin_fmaf(av[i], bv[j], acc[i][j]);
                        }
                    for (uint32_t i = 0; i < 16; i += 2)
                        for (uint32_t j = 0; j < 16; j++) {
                            const uint32_t k = rt * 8 + i / 2;
                            const uint64_t f = f0 + ct * 16 + j;
                            if (k < M && f < p.F) y[y0 + f * M + k] = c32{acc[i][j], acc[i + 1][j]};
                        }
                }
        }
        std::vector<c32> next(p.next.held);
        for (uint64_t i = 0; i < p.next.held; i++) next[i] = sample(p.V - p.next.held + i);
        tail.swap(next);
        st = p.next;
        at = end;
    }
    return y;
}

static int run(const char *cases, const char *outp) {
    FILE *f = fopen(cases, "rb"), *o = fopen(outp, "wb");
    if (!f || !o) return 2;
    int32_t hd[5];
    while (fread(hd, 4, 5, f) == 5) {
        const int64_t M = hd[0], P = hd[1], D = hd[2], Mp = (M + 1) / 2 * 2, L = P * M;
        const bool given = hd[3] != 0;
        int64_t N;
        if (fread(&N, 8, 1, f) != 1) return 3;
        std::vector<float> g(L);
        std::vector<c32> W(M * Mp), x(N);
        std::vector<int64_t> cuts(hd[4]);
        if (fread(g.data(), 4, L, f) != (size_t)L) return 3;
        if (given) {
            if (fread(W.data(), 8, M * Mp, f) != (size_t)(M * Mp)) return 3;
        } else {
            for (int64_t k = 0; k < M; k++)
                for (int64_t r = 0; r < Mp; r++) W[k * Mp + r] = r < M ? own_table(k * r % M, M) : c32{0.0f, 0.0f};
        }
        if (fread(x.data(), 8, N, f) != (size_t)N) return 3;
        if (!cuts.empty() && fread(cuts.data(), 8, cuts.size(), f) != cuts.size()) return 3;
        const std::vector<c32> ya = direct(M, P, D, g, W, x);
        const std::vector<c32> yb = tiled((uint32_t)M, (uint32_t)P, (uint32_t)D, g, W, x, cuts);
        if (ya.size() != yb.size()) {
            fprintf(stderr, "M=%d P=%d D=%d: %zu values directly, %zu tile by tile\n", hd[0], hd[1], hd[2], ya.size(), yb.size());
            return 5;
        }
        for (size_t i = 0; i < ya.size(); i++)
            if (!same(ya[i], yb[i])) {
                fprintf(stderr, "M=%d P=%d D=%d: frame %zu channel %zu: (%a, %a) directly, (%a, %a) tile by tile\n", hd[0], hd[1], hd[2],
                        i / (size_t)M, i % (size_t)M, ya[i].re, ya[i].im, yb[i].re, yb[i].im);
                return 5;
            }
        const int64_t F = (int64_t)ya.size() / M;
        fwrite(&F, 8, 1, o);
        fwrite(ya.data(), 8, ya.size(), o);
        fwrite(W.data(), 8, W.size(), o);
    }
    fclose(f);
    return fclose(o) ? 4 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: chanbank_ref run CASES OUT\n");
    return 64;
}
