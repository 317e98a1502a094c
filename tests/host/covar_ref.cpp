// covar_ref.cpp -- the bit-exact host restatement of the covariance bank and the beam scan (include/hzsdr_covar.h), a
// stand-alone program over csrc/hz_covar_math.h and csrc/hz_covar_plan.h.  Build: g++ -std=c++17 -O2 -ffp-contract=off.
//
// The bank is evaluated twice:
//   * directly from the contract: per block and per pair (p, q) the 256-term chains of the segments, the recursive
//     tree T(lo, hi), the combine;
//   * through the kernels' own indexing: the stream cut into the given pushes and those into launch rounds, regions and
//     items from the planner, a node per item in accumulator order (k-slot j of step t is snapshot 4 t + j, the staged
//     chunk read back through covar_lds_index), a group's three-level counter, the walker's counter with its sixteen
//     nodes at once, the stack and the held snapshots carried from push to push in their two buffers each, entries
//     read through covar_node_index.
// The two must agree bit for bit (exit status 1 otherwise); the device must reproduce them.
//
//   covar_ref run <cases> <out>
// cases: records of int32 mode, N, a, b, int64 n.
//   mode 0 (bank):  a = B, b = cuts; N rows of n complex64 (converted), b int64 ascending push boundaries.
//                   -> int64 blocks (the flushed one included), blocks x N x N complex64
//   mode 1 (scan):  a = G, b = matrices; G x N complex64 weights, b x N x N complex64 matrices -> b x G float32
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hz_covar_math.h"
#include "hz_covar_plan.h"

using namespace hz;
using cv::c32;

static void die(const char *m) {
    fprintf(stderr, "covar_ref: %s\n", m);
    exit(2);
}

// ---- directly ------------------------------------------------------------------------------------------------
static float tree(const std::vector<float> &g, uint32_t lo, uint32_t hi) {
    if (hi - lo == 1) return g[lo];
    uint32_t p = 1;
    while (p * 2 < hi - lo) p *= 2;  // the largest power of two strictly below hi - lo
    const float l = tree(g, lo, lo + p), r = tree(g, lo + p, hi);
    return cv::covar_node(l, r);
}

// row p of V at snapshot n of the stream: (re, im) of channel p / 2
static inline float vrow(const std::vector<c32> &x, uint64_t n_all, uint32_t p, uint64_t n) {
    const c32 &a = x[(size_t)(p >> 1) * n_all + n];
    return (p & 1u) ? a.im : a.re;
}

static void direct_block(const std::vector<c32> &x, uint64_t n_all, uint32_t N, uint64_t first, uint64_t len, c32 *R) {
    const uint32_t nseg = (uint32_t)((len + vp::kSeg - 1) / vp::kSeg), rows = 2 * N;
    std::vector<float> G((size_t)rows * rows), g(nseg);
    for (uint32_t p = 0; p < rows; p++)
        for (uint32_t q = 0; q < rows; q++) {
            for (uint32_t s = 0; s < nseg; s++) {
                float acc = 0.0f;
                for (uint32_t k = 0; k < vp::kSeg; k++) {
                    const uint64_t at = (uint64_t)s * vp::kSeg + k;
                    const float a = at < len ? vrow(x, n_all, p, first + at) : 0.0f, b = at < len ? vrow(x, n_all, q, first + at) : 0.0f;
                    acc = cv::covar_step(acc, a, b);
                }
                g[s] = acc;
            }
            G[(size_t)p * rows + q] = tree(g, 0, nseg);
        }
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t j = 0; j < N; j++)
            R[i * N + j] = cv::covar_combine(G[(size_t)(2 * i) * rows + 2 * j], G[(size_t)(2 * i + 1) * rows + 2 * j + 1],
                                             G[(size_t)(2 * i + 1) * rows + 2 * j], G[(size_t)(2 * i) * rows + 2 * j + 1]);
}

// ---- through the kernels' indexing --------------------------------------------------------------------------------
struct Bank {
    uint32_t N, B, NF;
    vp::State st;
    std::vector<c32> tail[2];
    int tcur = 0;
    std::vector<float> stack[2], nodes;  // (the stack as the kernel has it: read one, write the other)
    int scur = 0;
};

struct Add {
    float operator()(float l, float r) const { return cv::covar_node(l, r); }
};

// one launch round: `in` row i at in[i * pitch + ...], n snapshots (or the flush: w alone)
static void round_run(Bank &b, const vp::Step &p, const c32 *in, size_t pitch, std::vector<c32> &out) {
    const vp::Work &w = p.w;
    const uint32_t N = b.N, NF = b.NF, tiles = NF / vp::kTile, rows = vp::covar_rows(N);
    const std::vector<c32> &tin = b.tail[b.tcur];
    std::vector<c32> &tout = b.tail[b.tcur ^ 1];
    const std::vector<float> &sin = b.stack[b.scur];
    std::vector<float> &sout = b.stack[b.scur ^ 1];
    auto sample = [&](uint32_t i, uint64_t v) { return v < w.held_in ? tin[(size_t)i * vp::kSeg + v] : in[(size_t)i * pitch + (v - w.held_in)]; };
    if (b.nodes.size() < (size_t)w.nodes * NF) b.nodes.resize((size_t)w.nodes * NF);
    std::vector<float> lds((size_t)rows * vp::kPitch, 0.0f);
    // the segment kernel: one wave per item
    for (uint32_t ri = 0; ri < w.regions; ri++) {
        const vp::Region &r = w.r[ri];
        for (uint64_t blk = 0; blk < r.blocks; blk++)
            for (uint32_t it = 0; it < r.items; it++) {
                const vp::Item item = vp::covar_item(r, it);
                std::vector<float> acc(NF), s0(NF), s1(NF), s2(NF);
                for (uint32_t s = 0; s < item.count; s++) {
                    const uint32_t seg = item.seg + s, len = vp::covar_seg_len(r, seg);
                    const uint64_t v0 = vp::covar_seg_start(r, blk, seg, b.B);
                    std::fill(acc.begin(), acc.end(), 0.0f);
                    for (uint32_t h = 0; h < vp::kSeg / vp::kChunk; h++) {
                        const uint32_t c0 = h * vp::kChunk, clen = len > c0 ? len - c0 : 0;
                        for (uint32_t i = 0; i < N; i++)
                            for (uint32_t n = 0; n < vp::kChunk; n++) {
                                const c32 x = n < clen ? sample(i, v0 + c0 + n) : c32{0.0f, 0.0f};
                                lds[vp::covar_lds_index(2 * i, n)] = x.re;
                                lds[vp::covar_lds_index(2 * i + 1, n)] = x.im;
                            }
                        for (uint32_t t = 0; t < vp::kChunk / 4; t++)
                            for (uint32_t tile = 0; tile < tiles; tile++)
                                for (uint32_t lane = 0; lane < 64; lane++)
                                    for (uint32_t reg = 0; reg < 4; reg++) {
                                        // D[row][col] += sum over the k-slots, ascending, of A[row][k] B[k][col]
                                        const uint32_t row = (lane >> 4) * 4 + reg, col = lane & 15u;
                                        // (rows of V behind 2N are +0: such an entry stays +0 through every step)
                                        if (vp::covar_tile_a(tile) + row >= 2 * N || vp::covar_tile_b(tile) + col >= 2 * N) continue;
                                        float a = acc[tile * vp::kTile + lane * 4 + reg];
                                        for (uint32_t k = 0; k < 4; k++)
                                            a = cv::covar_step(a, lds[vp::covar_lds_index(vp::covar_tile_a(tile) + row, 4 * t + k)],
                                                               lds[vp::covar_lds_index(vp::covar_tile_b(tile) + col, 4 * t + k)]);
                                        acc[tile * vp::kTile + lane * 4 + reg] = a;
                                    }
                    }
                    if (item.count > 1)
                        for (uint32_t e = 0; e < NF; e++) {
                            float v = acc[e];
                            if (s & 1u) {
                                v = cv::covar_node(s0[e], v);
                                if (s & 2u) {
                                    v = cv::covar_node(s1[e], v);
                                    if (s & 4u)
                                        v = cv::covar_node(s2[e], v);
                                    else
                                        s2[e] = v;
                                } else
                                    s1[e] = v;
                            } else
                                s0[e] = v;
                            acc[e] = v;
                        }
                }
                memcpy(&b.nodes[(size_t)(r.node0 + blk * r.items + it) * NF], acc.data(), NF * sizeof(float));
            }
    }
    // the walker: one workgroup per block, one lane per entry
    for (uint32_t ri = 0; ri < w.regions; ri++) {
        const vp::Region &r = w.r[ri];
        for (uint64_t blk = 0; blk < r.blocks; blk++) {
            const float *nodes = &b.nodes[(size_t)(r.node0 + blk * r.items) * NF];
            std::vector<float> G(NF);
            for (uint32_t e = 0; e < NF; e++) {
                float col[vp::kLevels];
                uint32_t count = r.seg0;
                if (r.resume)
                    for (uint32_t l = 0; l < vp::kLevels; l++)
                        if ((count >> l) & 1u) col[l] = sin[(size_t)l * NF + e];
                uint32_t it = 0;
                for (; it < r.head; it++) vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], 0u, Add{});
                for (uint32_t g = 0; g < r.groups;) {
                    if (vp::covar_walk_many(count, vp::kGroupLog, r.groups - g)) {
                        float v[vp::kWalk];
                        for (uint32_t k = 0; k < vp::kWalk; k++) v[k] = nodes[(size_t)(it + k) * NF + e];
                        for (uint32_t ww = 1; ww < vp::kWalk; ww *= 2)
                            for (uint32_t k = 0; k < vp::kWalk; k += 2 * ww) v[k] = cv::covar_node(v[k], v[k + ww]);
                        vp::covar_counter_push(col, count, v[0], vp::kGroupLog + vp::kWalkLog, Add{});
                        g += vp::kWalk, it += vp::kWalk;
                    } else {
                        vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], vp::kGroupLog, Add{});
                        g++, it++;
                    }
                }
                for (uint32_t k = 0; k < r.tail; k++, it++) vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], 0u, Add{});
                if (r.complete)
                    G[e] = vp::covar_counter_collapse(col, count, Add{});
                else
                    for (uint32_t l = 0; l < vp::kLevels; l++)
                        if ((count >> l) & 1u) sout[(size_t)l * NF + e] = col[l];
            }
            if (!r.complete) continue;
            for (uint32_t i = 0; i < N; i++)
                for (uint32_t j = 0; j < N; j++)
                    out.push_back(cv::covar_combine(G[vp::covar_node_index(2 * i, 2 * j)], G[vp::covar_node_index(2 * i + 1, 2 * j + 1)],
                                                    G[vp::covar_node_index(2 * i + 1, 2 * j)], G[vp::covar_node_index(2 * i, 2 * j + 1)]));
        }
    }
    // the tail kernel
    for (uint32_t i = 0; i < N; i++)
        for (uint32_t n = 0; n < w.held_out; n++) tout[(size_t)i * vp::kSeg + n] = sample(i, w.V - w.held_out + n);
    if (w.held_out) b.tcur ^= 1;
    if (w.keep) b.scur ^= 1;
    b.st = p.next;
}

static void bank_push(Bank &b, const c32 *in, size_t pitch, uint64_t n_in, std::vector<c32> &out) {
    const uint64_t round = vp::covar_round(b.B);
    for (uint64_t at = 0; at < n_in;) {
        const uint64_t n = n_in - at < round ? n_in - at : round;
        const vp::Step p = vp::covar_step(b.st, b.B, n);
        if (!p.ok) die("push too long");
        round_run(b, p, in + at, pitch, out);
        at += n;
    }
}

static int run(const char *src, const char *dst) {
    FILE *f = fopen(src, "rb"), *o = fopen(dst, "wb");
    if (!f || !o) die("cannot open");
    int32_t h[4];
    int status = 0;
    while (fread(h, sizeof h, 1, f) == 1) {
        int64_t n64;
        if (fread(&n64, 8, 1, f) != 1) die("short header");
        const uint32_t mode = (uint32_t)h[0], N = (uint32_t)h[1];
        if (N < vp::kMinChannels || N > vp::kMaxChannels) die("bad N");
        if (mode == 1) {
            const uint32_t G = (uint32_t)h[2], nm = (uint32_t)h[3];
            std::vector<c32> w((size_t)G * N), Q((size_t)nm * N * N);
            if (fread(w.data(), sizeof(c32), w.size(), f) != w.size() || fread(Q.data(), sizeof(c32), Q.size(), f) != Q.size()) die("short scan");
            std::vector<float> p((size_t)nm * G);
            for (uint32_t b = 0; b < nm; b++)
                for (uint32_t g = 0; g < G; g++) p[(size_t)b * G + g] = cv::scan_power(&Q[(size_t)b * N * N], &w[(size_t)g * N], N);
            fwrite(p.data(), sizeof(float), p.size(), o);
            continue;
        }
        const uint32_t B = (uint32_t)h[2], ncuts = (uint32_t)h[3];
        const uint64_t n = (uint64_t)n64;
        if (B < 1 || B > vp::kMaxBlock) die("bad B");
        std::vector<c32> x((size_t)N * n);
        std::vector<int64_t> cuts(ncuts);
        if (fread(x.data(), sizeof(c32), x.size(), f) != x.size() || fread(cuts.data(), 8, ncuts, f) != ncuts) die("short bank");
        // directly
        const uint64_t blocks = (n + B - 1) / B;
        std::vector<c32> R((size_t)blocks * N * N);
        for (uint64_t b = 0; b < blocks; b++) {
            const uint64_t first = b * B, len = n - first < B ? n - first : B;
            direct_block(x, n, N, first, len, &R[(size_t)b * N * N]);
        }
        // through the kernels' indexing
        Bank bank{N, B, vp::covar_node_floats(N)};
        bank.tail[0].resize((size_t)N * vp::kSeg), bank.tail[1].resize((size_t)N * vp::kSeg);
        bank.stack[0].resize((size_t)vp::kLevels * bank.NF), bank.stack[1].resize((size_t)vp::kLevels * bank.NF);
        std::vector<c32> T;
        uint64_t at = 0;
        for (uint32_t k = 0; k <= ncuts; k++) {
            const uint64_t to = k < ncuts ? (uint64_t)cuts[k] : n;
            if (to < at || to > n) die("bad cut");
            bank_push(bank, x.data() + at, (size_t)n, to - at, T);
            at = to;
        }
        round_run(bank, vp::covar_flush(bank.st), nullptr, 0, T);
        if (T.size() != R.size() || memcmp(T.data(), R.data(), R.size() * sizeof(c32)) != 0) {
            fprintf(stderr, "covar_ref: N = %u B = %u n = %llu: the two evaluations differ\n", N, B, (unsigned long long)n);
            status = 1;
        }
        const int64_t nb = (int64_t)blocks;
        fwrite(&nb, 8, 1, o);
        fwrite(R.data(), sizeof(c32), R.size(), o);
    }
    fclose(f);
    if (fclose(o) != 0) die("write failed");
    return status;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "run")) return run(argv[2], argv[3]);
    fprintf(stderr, "usage: covar_ref run <cases> <out>\n");
    return 2;
}
