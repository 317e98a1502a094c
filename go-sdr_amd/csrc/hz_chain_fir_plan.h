// hz_chain_fir_plan.h -- the host arithmetic of the FIR-decimate terminal's transform form, free of HIP: the
// overlap-save geometry hzsdr_chain_fir_decimate chooses and the list of reference-order blocks the analysis kernel
// dispatches first (hz_chain_fir.hip: slow_blocks; device side: late_block in hz_chain_dev.h).  Plain integers in,
// plain structs out, so that tests/host/chain_fir_plan.cpp can run it under the sanitizers and compare it with the
// restatement the tests size their calls by (tests/fir_ref.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace hz {

// the blocks of a run that do NOT take the late path, ascending (host: slow_blocks)
constexpr int kMaxSlowBlocks = 96;
struct SlowBlocks {
    int n;
    unsigned idx[kMaxSlowBlocks];
};

// The overlap-save block of a filter of n_taps taps behind a decimation by `factor`.
// N_fft = next power of two >= 4 * taps, in [N_min, 8192].  N_min is the smallest size at which the
// fast forms of the kernels apply: the late mixer needs one block per workgroup (N >= 1024) and
// the polyphase analysis N / D >= 256 for D = 2, 4, 8, 16.  Measured on 2^24 u8 samples (us per
// chain_run, N_min = 256 as in round 1 -> now): D = 8, 64 taps 152 -> 43, 256 taps 71 -> 45;
// D = 16, 256 taps 69 -> 41; D = 4, 128 taps 167 -> 54; D = 2, 64 taps 157 -> 78.
// (hzsdr_chain_fir_options' nfft_min overrides N_min: the measurement aid those numbers come from.)
// ok == false: too many taps for the 8192-point block (off + factor > nfft).
struct FirGeom {
    unsigned nfft, off, hop;
    bool ok;
};
inline FirGeom fir_geometry(size_t n_taps, unsigned factor, unsigned nfft_min) {
    unsigned nfft = 1024;
    if (factor == 2 || factor == 4 || factor == 8 || factor == 16) nfft = std::max(1024u, 256u * factor);
    if (nfft_min) nfft = nfft_min;
    if (nfft < 256 || nfft > 8192 || (nfft & (nfft - 1))) nfft = 1024;
    while (nfft < 4 * n_taps && nfft < 8192) nfft <<= 1;
    FirGeom g{nfft, 0, 0, false};
    const uint64_t off = ((uint64_t)(n_taps - 1) + factor - 1) / factor * factor;  // first valid output on the decimation grid
    if (off + factor > nfft) return g;
    g.off = (unsigned)off;
    g.hop = (nfft - g.off) / factor * factor;
    g.ok = true;
    return g;
}

// The blocks of a call of n samples (nblocks overlap-save blocks) that mix in reference order, ascending.
// Block b spans [b*hop - off, b*hop - off + N) and is late iff that span lies in [0, n - off] AND inside
// one clock run that has a filter.  The clock runs are first[0 .. n_runs) (first[0] = 0; n_runs = 0: one run
// over the whole call), has_filter[r] whether run r has a modulated spectrum.
// Walks the runs, not the blocks; more than kMaxSlowBlocks of them -> empty list (stream order).
inline void slow_blocks_plan(int64_t N, int64_t hop, int64_t off, size_t n, size_t nblocks, int n_runs, const uint64_t *first,
                             const bool *has_filter, SlowBlocks *out) {
    out->n = 0;
    std::vector<unsigned> v;
    auto add_range = [&](int64_t lo, int64_t hi) {  // blocks lo .. hi inclusive, clipped
        if (lo < 0) lo = 0;
        if (hi >= (int64_t)nblocks) hi = (int64_t)nblocks - 1;
        for (int64_t b = lo; b <= hi && v.size() <= (size_t)kMaxSlowBlocks; b++) v.push_back((unsigned)b);
    };
    // every block whose span contains a sample of [s_lo, s_hi]: b*hop - off <= s_hi and b*hop - off + N > s_lo
    auto touching = [&](int64_t s_lo, int64_t s_hi) {
        int64_t lo = s_lo + off - N;            // b*hop > lo
        lo = lo < 0 ? 0 : lo / hop + 1;
        add_range(lo, (s_hi + off) / hop);
    };
    // stream edges: spans that start before sample 0 (b*hop < off) or end after n - off (b*hop > n - N)
    if (off > 0) add_range(0, (off - 1) / hop);
    add_range((int64_t)n >= N ? ((int64_t)n - N) / hop + 1 : 0, (int64_t)nblocks - 1);
    const int nr = n_runs > 0 ? n_runs : 1;
    for (int r = 0; r < nr; r++) {
        const int64_t f = n_runs > 0 ? (int64_t)first[r] : 0;
        const int64_t end = (n_runs > 0 && r + 1 < n_runs) ? (int64_t)first[r + 1] : (int64_t)n;
        if (!has_filter[r]) touching(f, end - 1);      // a run without a filter: every block in it
        else if (r > 0) touching(f - 1, f);            // a boundary: the blocks that straddle it
        if (v.size() > (size_t)kMaxSlowBlocks) return;
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    if (v.size() > (size_t)kMaxSlowBlocks) return;
    out->n = (int)v.size();
    for (size_t i = 0; i < v.size(); i++) out->idx[i] = v[i];
}

}  // namespace hz
