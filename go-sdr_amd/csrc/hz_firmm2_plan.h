// hz_firmm2_plan.h -- the HOST side of the persistent-pass matrix FIR (hz_firmm2.h): geometry, the kernel's
// argument structures and the planner that cuts one call into clock runs, passes and fix-up tasks.  No HIP in
// here: the library includes it through hz_firmm2.h, and tests/host/ builds it with gcc -fsanitize=address,
// undefined and fuzzes the planner's invariants (the GPU box offers no device sanitizers).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace hz {
namespace mm2 {

constexpr int kT = 8;        // outputs per tile
constexpr int kWaves = 8;    // two per SIMD
constexpr int kThreads = 64 * kWaves;
constexpr int kFixOut = 16;  // outputs per fix-up task
constexpr int kHistPer = 64; // samples per history task
constexpr int kMaxRuns = 16;  // clock runs of a call that take the matrix path (more: the call keeps the transforms)
constexpr int kMaxClockRuns = 32;  // hz_nco.h: kNcoMaxSegs, the runs of the clock that travel in the kernel arguments
constexpr int kMaxFix = kMaxClockRuns + 2;
// outputs: a clock run whose WHOLE line (run_line below: the binade's, not the call's piece of it) is shorter than this is
// left to the fix-up tasks.  (Rounds 3-5: 2560, "while there are workgroups left to take a task each" -- a budget
// counted over the call, so the same run could go one way in a call over four buffers and the other way in the four
// single calls.  By the run's own length the choice belongs to the stream: behind a 2 pi wrap the binades double from
// one sample up, the runs below 1280 outputs add up to ~160 tasks, one per workgroup as before.)
constexpr uint64_t kShortRun = 1280;
constexpr int kU = 12;       // 16-byte pieces per lane of a pass image, any window (768 pieces = 12 KB at most)

// (round 6: factor 16 as well -- one column block per pass, 256 outputs; 24 ... 64 keep the chunk kernel: their tiles
// are 24 ... 64 pieces wide and the matrix loop's operand rings are written for groups of 4 or 8 steps)
constexpr bool factor_ok(unsigned D) { return D == 8 || D == 16; }
constexpr int blocks_for(int D) { return D >= 16 ? 1 : 2; }
constexpr int tile_bytes(int D) { return 2 * D * kT; }
constexpr int pass_tiles(int D) { return 32 * blocks_for(D); }
constexpr int pass_out(int D) { return pass_tiles(D) * kT; }
// bytes of a pass: the windows of its tiles, 32 ks = (ks / GS) tile_bytes
constexpr size_t image_bytes(int D, int ks) { return (size_t)(pass_tiles(D) - 1) * tile_bytes(D) + 32 * (size_t)ks; }
// In LDS a tile is followed by 16 bytes of padding: a fragment read (one piece of 16 consecutive tiles per
// lane group) then falls on 16 different 16-byte bank groups (9 t + p mod 16 for 128-byte tiles), and --
// unlike an XOR swizzle -- every address of the matrix loop is ONE per-lane base plus a constant: tile
// n + g, piece 2 j + h, block b sit at base + tile_stride g + 32 j + 32 tile_stride b.
// `plane`: the per-plane matrix loop (hz_firmm2.h, kPlane; plane_form below).  Its lane 16 kq + r reads piece kq of
// tile r, and ds_read_b128 serves a wave in four groups of sixteen lanes that MIX two values of kq (lanes 0-3, 12-15
// with kq and lanes 20-27 with kq + 1; 4-11, 16-19 and 28-31; the same + 32).  With a stride of 16 c bytes, c odd, c r
// mod 16 takes every value, so the + 1 of kq always meets a 16-byte bank group that the other half of the lane group
// uses: 2-way conflicts on every read at 144 bytes.  c = 2 mod 8 puts the two halves on even and on odd groups: 32 bytes
// of padding, 160 (176, 192 and 208 conflict again).  tests/host/plane_layout.cpp counts the cycles of both.
constexpr int tile_stride(int D, bool plane = false) { return tile_bytes(D) + (plane ? 32 : 16); }
// The instantiation a launch takes (hz_firmm2.hip: launch_fmt) runs the per-plane loop: factor 8, the 1024-tap window's
// 17 groups of 4 steps, the default loop form.  Host and kernel size the LDS by this one flag.
// (loop forms of hzsdr_chain_fir_options: 8 the pair loop, 9 the per-plane loop that reads four tile windows per pair, 10
// the per-plane loop that re-uses them -- reuse_form below; 0, the default, is one of the last two)
constexpr int kLoopPair = 8, kLoopPlane = 9, kLoopReuse = 10;
constexpr int kLoopDefault = kLoopReuse;
constexpr bool plane_form(int D, int ks, int loop_form) {
    return D == 8 && ks == 17 * 4 && (loop_form == 0 || loop_form == kLoopPlane || loop_form == kLoopReuse);
}
// The per-plane loop with the tiles INTERLEAVED over the column blocks: column c of block j is tile 4 c + j (not 16 j + c),
// so lane (c, kq) reads row 4 c + j + t / 2 of the image on pair t, and the fragment of block j on pair t + 2 is the
// fragment of block j + 1 on pair t IN THE SAME LANE: it stays in its register, and a pair reads one new B fragment
// (row 4 c + 3 + t / 2) where the loop above reads four.
constexpr bool reuse_form(int D, int ks, int loop_form) {
    return plane_form(D, ks, loop_form) && (loop_form == 0 ? kLoopDefault : loop_form) == kLoopReuse;
}
// (the loop's look-ahead reads two steps past the last window: one tile behind the image)
constexpr size_t slot_bytes(int D, int ks, bool plane = false) {
    return ((image_bytes(D, ks) / tile_bytes(D) + 1) * tile_stride(D, plane) + 255) / 256 * 256;
}
// The re-using loop's slot: a lane's rows are FOUR rows apart, and at 160 bytes per row that is a lane stride of 640 = 16 *
// 40, 40 = 0 mod 8 -- every lane of a kq on one 16-byte bank group.  Rows 128 bytes apart and 32 bytes of padding behind
// every fourth row: the lane stride is 544 = 16 * 34, 34 = 2 mod 8, the class tile_stride's comment found conflict-free,
// a row's 128 bytes stay contiguous (the landing's writes), and row 4 c + r is at 544 c + reuse_row_offset(r): one
// per-lane base and constants, as before.  tests/host/window_reuse_layout.cpp counts the cycles.
constexpr int reuse_row_offset(int row) { return 128 * row + 32 * (row >> 2); }
// ... what lane (c, kq) reads as column block j's B operand on pair t: piece kq + 4 (t & 1) of row 4 c + j + t / 2
constexpr int reuse_b_offset(int j, int t, int c, int kq) { return reuse_row_offset(4 * c + j + t / 2) + 64 * (t & 1) + 16 * kq; }
// ... the register b[r][s] that holds that fragment, and whether pair t's own load reads it (else it is in the register
// since pair t - 2, as block j + 1's)
constexpr int reuse_b_reg(int j, int t) { return (j + t / 2) & 3; }
constexpr bool reuse_b_read(int j, int t) { return t < 2 || j == 3; }
// (no look-ahead behind the last window: the image's rows, and behind them the epilogue's exchange area, xchg_* below)
constexpr int kXchgBytes = 2048;
constexpr size_t reuse_image_bytes(int D, int ks) {
    return ((size_t)reuse_row_offset((int)(image_bytes(D, ks) / tile_bytes(D))) + 255) / 256 * 256;
}
constexpr size_t reuse_slot_bytes(int D, int ks) { return reuse_image_bytes(D, ks) + kXchgBytes; }
// The re-using loop's accumulators leave lane 16 g + c, block j, register k with output i = 2 g + (k >> 1), part k & 1 of
// tile T = 4 c + j, and the mixer wants lane 32 h + n to hold y[b][a] with h = i >> 2, a = i & 3, n = T & 31, b = T >> 5: a
// lane bit below 4 becomes a register bit, which no permlane swap does.  The sixteen floats per lane go through the 2 KB
// behind the wave's image, one half b of the column blocks' tiles at a time: the four floats k = 0 .. 3 of (lane, j) are
// quad 2 b + (a >> 1) = 2 (c >> 3) + (g & 1) of destination lane d = 32 (g >> 1) + 4 (c & 7) + j -- one ds_write_b128,
// by the lanes with c >> 3 == b -- and lane d reads its two quads of the half back, one ds_read_b128 each.  Quad (a >> 1)
// of lane d lies at 1024 (a >> 1) + 16 sigma(d): sigma spreads the eight lanes of a write group (d = 4 c' + j, c' =
// 0 .. 7) over the eight 16-byte bank groups of 128 bytes and the sixteen lanes of a read group (d >> 2 in {0, 3, 5, 6}
// or {1, 2, 4, 7}, every j) over the sixteen of 256.
constexpr int xchg_sigma(int d) {
    return 32 * (d >> 5) + 16 * (d & 1) + 8 * ((d >> 1) & 1) + ((((d >> 2) & 7)) ^ (d & 1));
}
constexpr int xchg_dst_lane(int lane, int j) { return 32 * (lane >> 5) + 4 * (lane & 7) + j; }
constexpr int xchg_half(int lane) { return (lane >> 3) & 1; }  // b: the round in which the lane writes
constexpr int xchg_write_offset(int lane, int j) { return 1024 * ((lane >> 4) & 1) + 16 * xchg_sigma(xchg_dst_lane(lane, j)); }
constexpr int xchg_read_offset(int lane, int q) { return 1024 * q + 16 * xchg_sigma(lane); }  // q = a >> 1
// table: T[f][E][part][pl] of 16 bytes (digit plane 2 f + pl, most significant first), then (dc_re, dc_im), then the
// mixer's eight step factors of the run (step_factors below)
constexpr size_t table_bytes(int ne) { return (size_t)ne * 128 + 16 + 128; }
constexpr size_t table_lds(int ne) { return (table_bytes(ne) + 255) / 256 * 256; }
constexpr size_t kCtlBytes = 512;  // the queue's counter
// the fix-up task's window (ntaps + D (kFixOut - 1) samples) and taps
constexpr size_t task_bytes(int D, int ntaps) { return ((size_t)(2 * ntaps + D * (kFixOut - 1)) * 8 + 255) / 256 * 256; }
// two tables, the queue's counter, a slot per wave, the fix-up task's scratch
constexpr size_t lds_bytes(int D, int ks, int ne, int ntaps, bool plane = false) {
    return 2 * table_lds(ne) + kCtlBytes + kWaves * slot_bytes(D, ks, plane) + task_bytes(D, ntaps);
}
// ... by the loop form: the re-using loop's slots are its own (reuse_slot_bytes)
constexpr size_t form_slot_bytes(int D, int ks, bool plane, bool reuse) { return reuse ? reuse_slot_bytes(D, ks) : slot_bytes(D, ks, plane); }
constexpr size_t form_lds_bytes(int D, int ks, int ne, int ntaps, bool plane, bool reuse) {
    return 2 * table_lds(ne) + kCtlBytes + kWaves * form_slot_bytes(D, ks, plane, reuse) + task_bytes(D, ntaps);
}

// The per-plane loop's tap table in LDS is PLANE-MAJOR: P[plane][E][part] of 16 bytes, permuted while it is staged (the
// table in global memory keeps T[f][E][part][pl]; the pieces behind the 8 ne of the digits -- the constant term, the
// step factors -- stay where they are).  Lane (r16, kq) of the loop reads row r16 = 2 i + part of entry E = i - kq -
// 4 t + e0 on pair t: in T that is 64 (i - kq) + 32 part, sixteen lanes of a ds_read_b128 group on eight 16-byte bank
// groups, 2-way; in P it is 32 (i - kq) + 16 part = 16 r16 - 32 kq, contiguous per kq and the two halves of a lane
// group either apart or on the SAME addresses (a broadcast).
// piece q of T -> its piece in LDS
constexpr int plane_piece(int ne, int q) {
    return q >= 8 * ne ? q : ((2 * (q / (4 * ne)) + (q & 1)) * ne + (q % (4 * ne)) / 4) * 2 + ((q >> 1) & 1);
}
// byte offset in the LDS table of what lane (r16, kq) reads as plane p's A operand on pair t (D = 8)
constexpr int plane_a_offset(int ne, int e0, int p, int t, int r16, int kq) {
    return 32 * ne * p + 32 * ((r16 >> 1) - kq - 4 * t + e0) + 16 * (r16 & 1);
}
// ... and in the tile slot as column block j's B operand: piece kq + 4 (t & 1) of tile 16 j + r16 + t / 2
constexpr int plane_b_offset(int ts, int j, int t, int r16, int kq) { return ts * (16 * j + t / 2 + r16) + 64 * (t & 1) + 16 * kq; }

struct Geom {
    int ntaps;
    int w0;     // window start before a tile's first output sample: ntaps - 1 rounded up to 8
    int ks;     // 32-byte steps over a tile's window (a multiple of D / 2: whole groups)
    int ne;     // entries E of one fragment row of the table
    int e0;     // E of (i = 0, h = 0, s = 0)
    int shift;  // S: taps are q = round(h' 2^S)
    unsigned off;
    // the step pairs [p0_lo, p0_hi) of the per-plane matrix loop (hz_firmm2.h, kPlane) on which digit plane 0 of some
    // table entry they read may be nonzero, in every clock run's table (plane0_window); make_geom: all of them
    int p0_lo, p0_hi;
};

// What a call hands the kernel.  The kernel arguments are read through the scalar cache, where a miss costs
// ~0.9 us while every wave of the chip is asking (measured: five dependent groups of reads in front of the
// first matrix loop took 4.5 us): the plan keeps what the main path reads in its first line and ONE 64-byte
// line per clock run; the program P and the fix-up intervals F are read by the small tasks only.
struct Run {
    const void *tab;       // the run's digit table
    uint32_t m_lo, m_hi;   // the outputs that take the matrix path (tile-aligned inside the call)
    int pass_first;        // the passes (512 outputs of the call's grid) that hold outputs of the run: a pass that
    int pass_end;          // straddles a boundary belongs to BOTH runs and is multiplied twice, once per table
    // programs with exactly ONE Shift stage: the stage's phase tau ts / 2 pi at the BUFFER's first sample by
    // the run's line, and its increment per sample, in 2^-64 turns (mod 1)
    uint64_t phi, dphi;
    uint64_t first;        // the run's first sample
    int seg;               // the run's index in the program's clock table (programs with several Shift stages)
    int pad[3];
};
static_assert(sizeof(Run) == 64, "one scalar-cache line per run");
struct Plan {
    int n;          // clock runs with outputs on the matrix path, in stream order (at most kMaxRuns)
    int n_pass;     // passes of the call
    int cont;       // run 0 continues the previous call's last run: windows may reach into the raw history
    int shift_op;   // index of the program's only Shift stage, -1: none or several
    int n_task;     // fix-up tasks (F)
    int n_ops;      // stages of the program
    float gain;     // (unused)
    int grid;       // workgroups of the launch (gridDim.x is a read of the dispatch packet: another miss)
    int pass_first[kMaxRuns], pass_end[kMaxRuns];  // (copies: a workgroup finds its runs without reading their lines)
    Run run[kMaxRuns];
};
struct Fix {
    int n;
    int n_task;
    uint32_t m_a[kMaxFix], m_b[kMaxFix];
    int task_first[kMaxFix];
};
// A call over SEVERAL buffers of equal length (hzsdr_chain_run_batch): the kernel works on their concatenation -- the
// planner sees one call of nbuf * n samples -- and finds a sample's (an output's) buffer by its index.  Buffer j's
// VIRTUAL base is its address minus j buffers' worth of bytes, so that base + (index in the concatenation) is the
// sample's address; a pass (512 outputs) never straddles two buffers (the host: n / D is a multiple of pass_out), a
// pass IMAGE does at the first pass of every buffer but the first (its window reaches back into the previous
// buffer: the edge landing, piece by piece).  An ordinary call is nbuf = 1 with the buffers' own addresses.
constexpr int kMaxBatch = 8;
struct Batch {
    int nbuf;
    uint32_t ppb;        // passes per buffer
    uint32_t out_each;   // outputs per buffer
    uint32_t rcp;        // floor(2^32 / ppb) + 1: a pass's buffer is mulhi(pass, rcp) -- ONE scalar instruction (batch_ok bounds ppb)
    uint64_t nb;         // bytes per input buffer
    uint64_t vin[kMaxBatch], vout[kMaxBatch];
};
inline Batch one_buffer(const void *in, void *out, uint64_t n_in, unsigned D) {
    Batch B{};
    B.nbuf = 1;
    B.ppb = 0xffffffffu;
    B.out_each = (uint32_t)(n_in / D);
    B.nb = 2 * n_in;
    B.vin[0] = (uint64_t)(uintptr_t)in;
    B.vout[0] = (uint64_t)(uintptr_t)out;
    return B;
}
// nbuf buffers of n_each samples (n_each / D a multiple of the pass: the caller checks batch_ok)
inline bool batch_ok(uint64_t n_each, unsigned D, size_t nbuf) {
    if (!(nbuf >= 1 && nbuf <= (size_t)kMaxBatch && n_each % D == 0 && (n_each / D) % (uint64_t)pass_out((int)D) == 0 && n_each * nbuf / D < (1ull << 31)))
        return false;
    // pass / ppb as mulhi(pass, floor(2^32 / ppb) + 1): exact for pass < nbuf ppb as long as nbuf ppb^2 < 2^32
    const uint64_t ppb = n_each / D / (uint64_t)pass_out((int)D);
    // (ppb = 1: floor(2^32 / 1) + 1 does not fit 32 bits -- the reciprocal came out as 1 and every pass landed in
    // buffer 0, past its end; such buffers, 512 outputs each, go one by one)
    // (and a buffer of fewer than 4096 outputs does not take the matrix path by itself -- plan_call -- so a call over
    // several of them must not either: hzsdr_chain_run_batch promises the bits of single calls)
    return n_each / D >= 4096 && nbuf * ppb * ppb < (1ull << 32);
}
inline Batch make_batch(const void *const *ins, void *const *outs, size_t nbuf, uint64_t n_each, unsigned D) {
    Batch B{};
    B.nbuf = (int)nbuf;
    B.out_each = (uint32_t)(n_each / D);
    B.ppb = B.out_each / (uint32_t)pass_out((int)D);
    B.rcp = (uint32_t)((1ull << 32) / B.ppb) + 1u;
    B.nb = 2 * n_each;
    for (size_t j = 0; j < nbuf; j++) {
        B.vin[j] = (uint64_t)(uintptr_t)ins[j] - (uint64_t)j * B.nb;
        B.vout[j] = (uint64_t)(uintptr_t)outs[j] - (uint64_t)j * B.out_each * 8;
    }
    return B;
}

// The LINE a clock run lies on.  Inside one binade [2^e, 2^(e+1)) of the clock every value is a multiple of
// u = 2^(e-52) and a run advances by step = S u (hz_host.cpp: hzsdr_nco_segments), so the clock values of a run are
// T u with T = T0 + k S.  Where a CALL first meets the run is the caller's business -- a stream cut into other buffers
// meets it elsewhere -- but the line is the stream's: its anchor is the line's first point in the binade,
// T_a = T0 - floor((T0 - 2^52) / S) S, `before` = (T0 - T_a) / S samples in front of t0, and `full` = the samples of
// the line inside the binade (up to 2 pi in the binade that holds it).  Everything a kernel derives from a run --
// the mixer's phase, whether the run is worth a table -- is derived from the line, so the results do not depend on
// how the stream was cut into calls (hzsdr_chain_run_batch == the same buffers through hzsdr_chain_run, bit for
// bit; the reference's ts recurrence, stream/shifter.go:68-79, does not know about buffers either).
struct Line {
    double t_anchor;   // the clock at the anchor (exact)
    uint64_t before;   // samples between the anchor and t0
    uint64_t full;     // samples of the line in its binade (1: not a line -- a run of one sample, a clock that stands)
};
inline Line run_line(double t0, double step) {
    Line ln{t0, 0, 1};
    if (!(step > 0.0) || !isnormal(t0) || !(t0 > 0.0)) return ln;
    int e2;
    (void)frexp(t0, &e2);
    const int e = e2 - 1;  // t0 in [2^e, 2^(e+1))
    const double u = ldexp(1.0, e - 52);
    const double Td = t0 / u, Sd = step / u;  // (exact: powers of two)
    if (!(Sd >= 1.0) || Sd != floor(Sd) || Td != floor(Td) || !(Td < 9007199254740992.0) || !(Sd < 9007199254740992.0)) return ln;
    const uint64_t T0 = (uint64_t)Td, S = (uint64_t)Sd, Tmin = 1ull << 52;
    if (T0 < Tmin) return ln;
    const uint64_t k = (T0 - Tmin) / S, Ta = T0 - k * S;
    uint64_t Tmax = (1ull << 53) - 1;
    if (e == 2) {  // (the binade of 2 pi: the clock wraps there)
        const uint64_t tu = (uint64_t)(6.283185307179586476925286766559 / u);
        if (tu < Tmax) Tmax = tu;
    }
    ln.t_anchor = (double)Ta * u;  // (exact)
    ln.before = k;
    ln.full = Tmax >= Ta ? (Tmax - Ta) / S + 1 : 1;
    return ln;
}

// (t_prev, t0): the clocks of two consecutive samples of a stream; true when they lie on one line of the clock -- one
// binade, exactly `step` apart (the difference of two values of one binade is exact).  What a chain asks at a call
// boundary: does this call's run 0 continue the run the previous call ended in?
inline bool continues(double t_prev, double t0, double step) {
    if (!(step > 0.0) || !(t_prev > 0.0) || !(t0 > t_prev)) return false;
    int ea, eb;
    (void)frexp(t_prev, &ea);
    (void)frexp(t0, &eb);
    return ea == eb && t0 - t_prev == step;
}

// phase accumulator constants of a run (host): frac(tau step / 2 pi) and frac(tau t0 / 2 pi) - first * the increment,
// in 2^-64 turns.
// Extended precision: the increment is multiplied by up to 2^27 samples.
inline void phase_fix(double tau, double t0, double step, uint64_t first, uint64_t *phi, uint64_t *dphi) {
    const long double inv2pi = 0.159154943091895335768883763372514362L;
    auto fix = [](long double turns) {
        turns -= floorl(turns);  // [0, 1)
        const long double v = turns * 18446744073709551616.0L;
        return v >= 18446744073709551615.0L ? ~0ull : (uint64_t)v;
    };
    *dphi = fix((long double)tau * (long double)step * inv2pi);
    *phi = fix((long double)tau * (long double)t0 * inv2pi) - first * *dphi;  // (mod 2^64: by the run's line at sample 0)
}
// The same constants from the run's LINE (run_line above): the phase at the line's anchor, rounded once, plus whole
// increments -- the phase of a stream sample is then the same 64-bit number whichever call holds the sample and
// wherever that call starts.  (phase_fix rounds tau t0 at the CALL's first sample of the run: 2^-37 turns of rounding
// that differed from cut to cut and moved one pass in thirty across a boundary of sincos_turns32's 2^-32 grid --
// round 5's "a batch equals single calls within an ulp or two of the factor".)
inline void phase_line(double tau, double t0, double step, uint64_t first, uint64_t *phi, uint64_t *dphi) {
    const Line ln = run_line(t0, step);
    uint64_t pa;
    phase_fix(tau, ln.t_anchor, step, 0, &pa, dphi);
    *phi = pa + (ln.before - first) * *dphi;  // (mod 2^64: call sample j of the run is sample before + j - first of the line)
}

// The mixer's step factors of a clock run (chains with exactly one Shift stage): a lane forms ONE Sincos per pass, for
// its first output, and turns it on to its other seven outputs -- (32 kT b + a) D samples further, b = 0, 1 the
// column block, a = 0 .. 3 -- by exp(2 pi i k dphi), kept as float pairs (cos hi, sin hi, cos lo, sin lo).  They depend
// on the run's phase increment alone, so they are a property of the run's table and travel at its end (the kernel
// computed them in its first lines until round 4: two hundred float64 instructions in front of the first barrier).
inline void step_factors(double tau, double step, int D, float out[8][4]) {
    uint64_t phi, dphi;
    phase_fix(tau, 0.0, step, 0, &phi, &dphi);
    for (int i = 0; i < 8; i++) {
        const uint64_t k = (uint64_t)(D * (32 * kT * (i >> 2) + (i & 3)));
        const long double turns = (long double)(k * dphi) * 5.42101086242752217003726400434970855712890625e-20L;  // 2^-64 (k dphi mod 2^64)
        const long double ang = turns * 6.283185307179586476925286766559005768L;
        const long double cs = cosl(ang), sn = sinl(ang);
        const float ch = (float)cs, sh = (float)sn;
        out[i][0] = ch, out[i][1] = sh, out[i][2] = (float)(cs - (long double)ch), out[i][3] = (float)(sn - (long double)sh);
    }
}

// geometry of a chain with `ntaps` taps at decimation D (host)
inline Geom make_geom(int ntaps, int D, unsigned off, int shift) {
    Geom g{};
    g.ntaps = ntaps;
    g.w0 = (ntaps - 1 + 7) / 8 * 8;
    const int window = g.w0 + D * (kT - 1) + 1;  // samples a tile's outputs reach back over
    const int gs = D / 2;                        // steps per group
    g.ks = ((2 * window + 31) / 32 + gs - 1) / gs * gs;
    g.e0 = 2 * (g.ks + 4);
    g.ne = g.e0 + (D / 8) * (kT - 1) + 1;
    g.shift = shift;
    g.off = off;
    g.p0_lo = 0;
    g.p0_hi = g.ks / 2;
    return g;
}

// The step pairs on which the per-plane loop must multiply digit plane 0 (hz_firmm2.h, kPlane), for EVERY clock run's
// table of the chain (hz_firmm_plan.h, digit_table: taps h[k] exp(-i omega k step) scale, whatever omega and step).
//
// Plane 0 of a table byte is zero when its coefficient q satisfies -128 W <= q <= 127 W, W = 2^16 + 2^8 + 1: the three
// balanced base-256 digits d1, d2, d3 in [-128, 127] reach exactly that range, and digit_table's digits are THE
// balanced representation (each r = q mod 256 in [-128, 127], q <- (q - r) / 256), so d0 = 0 iff q is inside it.  (Not
// |q| < 2^23: q = 127 W + 1 = 8 355 712 has d0 = 1.)  A byte's coefficient is +-q_re or +-q_im of one tap, q =
// llround(c 2^S) with c = (hr cr - hi ci) scale or (hr ci + hi cr) scale, and |c| <= hypot(hr, hi) scale (1 + 2^-48)
// (Cauchy-Schwarz, cos^2 + sin^2 = 1 to a few ulp, a few roundings; hypot itself to an ulp).  So with m = hypot(hr, hi)
// scale 2^S: |q| <= m (1 + 2^-48) + 1/2 -- and a tap with m <= 127 W - 1 has |q| <= 127 W - 1/2 + 2^-25, i.e. (q an
// integer) |q| <= 127 W - 1: d0 = 0
// in every run.  Only taps with m > 127 W - 1 are "hot".  Tap k sits in ONE entry, E = e0 + (k - w0 + e) / 8 with
// its byte pair e = (w0 - k) mod 8 (digit_table: kap = 8 (E - e0) + w0 - e); pair t reads the entries (D / 8) i - kq -
// 4 t + e0 (i = 0 .. 7 outputs, kq = 0 .. 3 pieces).  The window is the smallest range of pairs that holds every pair
// reading an entry with a hot tap ([0, 0): none).
inline void plane0_window(Geom &g, int D, const double *taps, double scale) {
    constexpr double kW = 65536.0 + 256.0 + 1.0;
    const int np = g.ks / 2, ne = g.ne;
    bool *hot_e = new bool[ne]();
    for (int k = 0; k < g.ntaps; k++) {
        const double m = ldexp(hypot(taps[2 * k], taps[2 * k + 1]) * scale, g.shift);
        if (m <= 127.0 * kW - 1.0) continue;  // (NaN: hot)
        for (int e = 0; e < 8; e++) {  // byte pair e of entry E holds tap 8 (E - e0) + w0 - e
            const int num = k - g.w0 + e;
            if (num % 8 != 0) continue;
            const int E = g.e0 + num / 8;
            if (E >= 0 && E < ne) hot_e[E] = true;
        }
    }
    int lo = np, hi = 0;
    for (int t = 0; t < np; t++) {
        bool hot = false;
        for (int i = 0; i < kT && !hot; i++)
            for (int kq = 0; kq < 4 && !hot; kq++) {
                const int E = (D / 8) * i - kq - 4 * t + g.e0;
                hot = E >= 0 && E < ne && hot_e[E];
            }
        if (hot) {
            if (t < lo) lo = t;
            hi = t + 1;
        }
    }
    delete[] hot_e;
    g.p0_lo = lo < hi ? lo : 0;
    g.p0_hi = lo < hi ? hi : 0;
}


// ---- the planner ---------------------------------------------------------------------------------------------
// The exactly-linear runs of the NCO clock over the call's samples (hzsdr_nco_segments): run r starts at sample
// first[r] with clock t0[r] and advances by step[r]; tab[r]: the run's digit table (null: none was prepared).
// A chain without a Shift stage passes n = 1, first[0] = 0.
struct ClockRuns {
    int n;
    const uint64_t *first;
    const double *t0, *step;
    const void *const *tab;
};
struct PlanIn {
    uint64_t n_in;     // samples of the call (a multiple of D is consumed)
    unsigned D;
    int ntaps;
    bool has_shift;
    // run 0 continues the run the previous call ended in, and the last `back` samples in front of the call lie in
    // that run AND in the raw history (at most `off` of them): windows of run 0 may reach that far back.  0: they
    // may not reach in front of the call at all.  (Rounds 2-5 knew all or nothing -- `cont`, set when the run already
    // held ntaps samples; a run that starts less than ntaps samples in front of a buffer boundary then gave its first
    // outputs to the tasks in single calls and to the matrix path in a call over several buffers.)
    uint64_t back;
    int shift_op;      // the program's only Shift stage (-1: none or several) and its fl(2 pi f)
    double tau;
    int n_ops;
    int max_grid;      // CUs
};
// Every clock run with a table gets the outputs whose whole window lies in it (tile-aligned) and the passes of
// the call's 512-output grid that hold them -- a pass that straddles a boundary is multiplied once per run, each
// time with that run's table and valid range.  What no run holds -- windows that cross a boundary, the stream's
// start, runs without a table -- are fix-up tasks of kFixOut outputs.  false: the call keeps the transform
// kernels (too short, too many runs or intervals, mostly boundaries).
inline bool plan_call(const PlanIn &in, const ClockRuns &cr, Plan *L, Fix *F, uint64_t *fix_outputs = nullptr) {
    memset(L, 0, sizeof *L);
    memset(F, 0, sizeof *F);
    const uint64_t D = in.D, n_out = in.n_in / D, nt = (uint64_t)in.ntaps, tile = kT, pass = (uint64_t)pass_out((int)D);
    if (fix_outputs) *fix_outputs = 0;
    if (n_out < 4096 || n_out >= (1ull << 31)) return false;  // (a call this short is launch-bound either way)
    if (cr.n < 1 || cr.n > kMaxClockRuns) return false;
    L->cont = in.back > 0 ? 1 : 0;
    L->n_ops = in.n_ops;
    L->gain = 1.0f;
    L->shift_op = in.shift_op;
    uint64_t fix_total = 0, covered = 0;  // outputs below `covered` are planned
    bool too_many = false;
    auto add_fix = [&](uint64_t a, uint64_t b) {
        if (b <= a) return;
        fix_total += b - a;
        if (F->n >= kMaxFix) {
            too_many = true;
            return;
        }
        F->m_a[F->n] = (uint32_t)a;
        F->m_b[F->n] = (uint32_t)b;
        F->task_first[F->n] = F->n_task;
        F->n_task += (int)((b - a + kFixOut - 1) / kFixOut);
        F->n++;
    };
    for (int r = 0; r < cr.n; r++) {
        const uint64_t a = cr.first[r];
        const uint64_t b = r + 1 < cr.n ? cr.first[r + 1] : in.n_in;
        uint64_t lo = (a + nt - 1 + D - 1) / D, hi = (b + D - 1) / D < n_out ? (b + D - 1) / D : n_out;
        if (r == 0 && in.back > 0) lo = in.back >= nt - 1 ? 0 : (nt - 1 - in.back + D - 1) / D;  // (a = 0: D m - (nt - 1) >= -back)
        lo = (lo + tile - 1) / tile * tile;
        if (hi < n_out) hi = hi / tile * tile;
        // a run without a table, or nothing of it on the matrix path.  (Rounds 3-5 also left pieces of fewer than 64
        // outputs to the tasks -- "too short to bother" -- which is a property of the call's cut, not of the run)
        if (!cr.tab[r] || hi <= lo) continue;
        // A SHORT run -- the binades behind a 2*pi wrap of the clock double from a few samples up -- would put its
        // table and one more multiplication of every pass it shares on ONE workgroup (the call's first: 24 items
        // for its eight waves instead of 16, a whole pass time longer than the rest).  As fix-up tasks its outputs
        // spread over the workgroups, one task each.  Short by the run's LINE, not by the call's piece of it.
        if (in.has_shift && run_line(cr.t0[r], cr.step[r]).full / D < kShortRun) continue;
        if (L->n >= kMaxRuns) return false;
        Run &u = L->run[L->n];
        u.tab = cr.tab[r], u.m_lo = (uint32_t)lo, u.m_hi = (uint32_t)hi;
        u.pass_first = (int)(lo / pass), u.pass_end = (int)((hi + pass - 1) / pass);
        u.seg = r;
        u.first = a;
        if (in.shift_op >= 0) phase_line(in.tau, cr.t0[r], cr.step[r], u.first, &u.phi, &u.dphi);
        L->pass_first[L->n] = u.pass_first, L->pass_end[L->n] = u.pass_end;
        add_fix(covered, lo);
        L->n++;
        covered = hi;
    }
    if (L->n == 0) return false;
    add_fix(covered, n_out);
    L->n_pass = (int)((n_out + pass - 1) / pass);
    L->n_task = F->n_task;
    L->grid = in.max_grid < L->n_pass ? in.max_grid : L->n_pass;
    if (L->grid < 1) L->grid = 1;
    if (fix_outputs) *fix_outputs = fix_total;
    // the fix-up tasks are the slow way: a call that is mostly boundaries keeps the transforms; a workgroup takes
    // them one at a time, behind its passes
    return !too_many && F->n_task <= 4 * L->grid && fix_total * 8 <= n_out;
}

}  // namespace mm2
}  // namespace hz
