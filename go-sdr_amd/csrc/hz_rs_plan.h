// hz_rs_plan.h -- the host arithmetic of the Reed-Solomon decoder bank (include/hzsdr_rs.h), HIP-free so that
// tests/host/rs_plan.cpp can run it under the sanitizers: the validation of a bank's configuration (the primitivity test
// included) and of a call, the sizes, the table block the kernel reads, the LDS layout and the launch plan.
//
// Workgroups.  One workgroup decodes one frame at a time: I waves, wave i owns codeword i (frame bytes i, i + I, ...).
// A workgroup takes frame slot blockIdx (slot = row * cap + frame), then those a grid further on.
//
// The table block, made once at create, on the device: exp (512), log (256), in_map (256), out_map (256; identity where
// the caller gave none), then the scramble sequence written out to F bytes (zeros where there is none), so that the
// kernel neither divides nor branches per byte.  The first four are staged in the workgroup's LDS.
//
// LDS, bytes: [0, off_frame) the four tables; the frame's F prepared symbols (rounded up to 16); per wave kWaveBytes:
// 64 syndromes, 64 locator coefficients, 64 evaluator coefficients; one result word per wave.  5 KiB at the most, so a
// CU's 160 KiB would hold 32 workgroups and more: the occupancy is set by the 32 waves a CU holds, 32 / I workgroups
// (8 waves per SIMD), never by the LDS.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "hz_decodebank_plan.h"
#include "hz_rowwave_plan.h"
#include "hz_rs_math.h"

namespace hz {
namespace rsp {

using rw::kLanes, rw::kLdsBudget;
using dbp::kMaxRows, dbp::kMaxFrames;

constexpr uint32_t kMinRoots = 2, kMaxRoots = rsm::kMaxRoots, kMaxN = 255, kMaxInterleave = 8, kMaxScramble = 2040;
constexpr uint32_t kTabExp = 0, kTabLog = kTabExp + rsm::kExpSize, kTabIn = kTabLog + rsm::kLogSize, kTabOut = kTabIn + 256, kTabBytes = kTabOut + 256;
constexpr uint32_t kWaveSyn = 0, kWaveLam = 64, kWaveOmg = 128, kWaveBytes = 192;
constexpr uint32_t kMaxGroups = 65536;   // the grid at most; a workgroup walks on from slot to slot
constexpr uint32_t kCuLds = 160 * 1024, kCuWaves = 32;
constexpr uint32_t kPasses = (kMaxN + kLanes - 1) / kLanes;  // the Chien search deals n positions over 64 lanes

struct Config {
    uint32_t gfpoly, fcr, prim, nroots, n, interleave, scramble_len;
};

inline uint32_t gcd(uint32_t a, uint32_t b) {
    while (b) {
        const uint32_t r = a % b;
        a = b, b = r;
    }
    return a;
}

// alpha = 0x02 has order 255 under the polynomial
inline bool primitive(uint32_t gfpoly) {
    if ((gfpoly >> 8) != 1u) return false;
    uint32_t x = 1;
    for (uint32_t i = 1; i <= rsm::kOrder; i++) {
        x = rsm::mulx(x, gfpoly);
        if (x == 1) return i == rsm::kOrder;
        if (x == 0) return false;
    }
    return false;
}

// nullptr when the configuration makes a bank, else what is wrong with it
inline const char *check_config(const Config &q) {
    if (!primitive(q.gfpoly)) return "gfpoly is a primitive polynomial of degree 8 (bit 8 set)";
    if (q.nroots < kMinRoots || q.nroots > kMaxRoots) return "2 <= nroots <= 64";
    if (q.n <= q.nroots || q.n > kMaxN) return "nroots < n <= 255";
    if (q.fcr >= rsm::kOrder) return "fcr is below 255";
    if (q.prim < 1 || q.prim >= rsm::kOrder || gcd(q.prim, rsm::kOrder) != 1) return "1 <= prim <= 254 with gcd(prim, 255) = 1";
    if (q.interleave < 1 || q.interleave > kMaxInterleave) return "1 <= interleave <= 8";
    if (q.scramble_len > kMaxScramble) return "scramble_len is at most 2040";
    return nullptr;
}

struct Geom {
    uint32_t k, t, F, IK;            // data symbols, correctable errors, frame bytes I n, data bytes I k
    uint32_t waves, threads;         // per workgroup: I, 64 I
    uint32_t off_frame, off_wave, off_res;
    size_t lds_bytes;
    size_t table_bytes;              // the device block: kTabBytes + F
    uint32_t groups_per_cu;          // min(32 / I waves, 160 KiB / lds_bytes)
};

// a checked configuration
inline Geom geom(const Config &q) {
    Geom g{};
    g.k = q.n - q.nroots, g.t = q.nroots / 2;
    g.F = q.interleave * q.n, g.IK = q.interleave * g.k;
    g.waves = q.interleave, g.threads = q.interleave * kLanes;
    g.off_frame = kTabBytes;
    g.off_wave = g.off_frame + ((g.F + 15u) & ~15u);
    g.off_res = g.off_wave + g.waves * kWaveBytes;
    g.lds_bytes = (size_t)g.off_res + g.waves * 4u;
    g.table_bytes = (size_t)kTabBytes + g.F;
    const uint32_t by_lds = (uint32_t)(kCuLds / g.lds_bytes), by_waves = kCuWaves / g.waves;
    g.groups_per_cu = by_lds < by_waves ? by_lds : by_waves;
    return g;
}

inline uint32_t groups_for(size_t slots) { return (uint32_t)(slots < kMaxGroups ? slots : kMaxGroups); }

// the table block: in_map, out_map (256 bytes each) and scramble (scramble_len bytes) may be null
inline bool build_block(const Config &q, const Geom &g, const uint8_t *in_map, const uint8_t *out_map, const uint8_t *scramble, std::vector<uint8_t> &block) {
    block.assign(g.table_bytes, 0);
    if (!rsm::build_tables(q.gfpoly, block.data() + kTabExp, block.data() + kTabLog)) return false;
    for (uint32_t b = 0; b < 256; b++) {
        block[kTabIn + b] = in_map ? in_map[b] : (uint8_t)b;
        block[kTabOut + b] = out_map ? out_map[b] : (uint8_t)b;
    }
    if (q.scramble_len && scramble) {
        uint32_t ph = 0;
        for (uint32_t m = 0; m < g.F; m++) {
            block[kTabBytes + m] = scramble[ph];
            if (++ph == q.scramble_len) ph = 0;
        }
    }
    return true;
}

// ---- a call ----
// (hz_decodebank_plan.h's, over slots with pitches in bytes; in place, or apart)
using dbp::kOk, dbp::kInvalid, dbp::kDstTooSmall, dbp::Call;
inline dbp::Slots slots(const Geom &g) { return {g.F, g.IK, true, "in_stride is below cap frame slots", "out_stride is below cap frame slots"}; }
inline int check_call(const Geom &g, const Call &c, const char **why) { return dbp::check_call(slots(g), c, why); }

// ---- the kernel's index maps ----
// where symbol p of codeword i lies in the frame
HZ_HD uint32_t frame_index(uint32_t i, uint32_t p, uint32_t I) { return i + p * I; }
// the position that lane `lane` tests in pass q of the Chien search (valid where below n)
HZ_HD uint32_t chien_position(uint32_t q, uint32_t lane) { return q * kLanes + lane; }
// the syndrome that coefficient c needs in iteration r of Berlekamp-Massey (valid where c <= r)
HZ_HD uint32_t bm_syndrome(uint32_t r, uint32_t c) { return r - c; }

}  // namespace rsp
}  // namespace hz
