// hz_firmm2.h -- the int8 matrix FIR (hz_firmm.h) re-cut so that its phases overlap: one PERSISTENT
// workgroup per CU whose eight waves pull small passes from a queue.
//
// hz_firmm.h runs 1024 workgroups, each of which loads 34 KB, multiplies for 24 us and finishes 2048
// outputs -- all of them in the same phase at the same time (accumulators for ALL 2^21 outputs of a
// 2^24-sample call are resident at once, so there is exactly one round): the matrix pipe idles through
// the 9 us input burst and the 5 us epilogue, 44 % busy over the kernel.  A round can only be cut into
// shorter ones with FEWER accumulators per wave, and fewer accumulators mean less operand re-use; what
// makes that affordable is the LDS (256 B/clk/CU for ds_read_b128, a quarter of it used by hz_firmm.h)
// once the tap table lives there too -- which needs ONE copy per CU, i.e. one workgroup per CU:
//
//   * a tile = EIGHT consecutive outputs x (re, im) x TWO digit planes = 32 rows of the Toeplitz
//     matrix (hz_firmm.h: 16 outputs x (re, im), the planes split over two waves).  One wave holds all
//     four planes of its outputs (two A fragments), nothing is exchanged between waves, and a tile's
//     window is 56 samples wider than the taps instead of 120 (68 instead of 72 MFMA steps at 1024 taps);
//   * a PASS = 2 column blocks of 32 tiles = 512 outputs (D = 8): 4 accumulators (64 registers), 10 KB of
//     input in a slot of LDS that belongs to the wave.  Per 32-byte step of the window: two A fragments
//     from the table in LDS, two B fragments from the slot, four MFMAs -- 1 KB of LDS reads per MFMA,
//     half of what the LDS delivers, no global load in the loop;
//   * a wave's life: take a pass from the workgroup's queue (an LDS counter), and while it multiplies,
//     the NEXT pass's bytes are in flight into registers (landed in the slot when the loop is done);
//     the finished pass's float64 combination, mixer and stores then run beside the partner wave's
//     loop on the same SIMD.  The eight waves de-phase by themselves (the queue) and by construction
//     (waves 4-7, the second wave of each SIMD, start half a pass late);
//   * the table (19 KB per clock run at 1024 taps) is loaded once per workgroup; a workgroup whose
//     range of passes spans a run boundary reloads it between the runs (a barrier; one or two of the
//     256 workgroups per call);
//   * fix-up tasks (outputs in reference order) and history tasks are wave-sized here and ride on the
//     waves of all workgroups before their first pass.
//
// Geometry, table contents and the arithmetic (four balanced base-256 digit planes of 32-bit
// fixed-point taps, exact int32 sums, one float64 combination, one rounding) are those of hz_firmm.h.
#pragma once
#include <type_traits>

#include "hz_firmm.h"
#include "hz_firmm2_plan.h"

namespace hz {
namespace mm2 {

using mm::v16i;
using mm::v4i;

using mm::find_le;
using mm::task_window;

// The kernel's arguments as ONE struct (the kernarg segment's layout: the explicit arguments in order, each at its
// natural alignment), for the RARE paths -- fix-up and history tasks, edge landings, the elementwise stages other
// than the one Shift the planner marks.  Left to read the arguments the ordinary way, everything those paths derive
// from them (pointers, comparisons, table addresses) is loop-invariant and the compiler hoists it to the kernel's
// head and parks it in spilled scalar registers: 138 of the 621 instructions in front of the first barrier were
// v_writelane, executed by every wave of every launch at the cold instruction cache's ~7 ns per instruction, for
// paths most launches never take.  A rare path starts with HZ_COLD_ARGS instead: the kernarg pointer through an
// empty asm (nothing derived from it can move above that line) and its own names for the arguments.
struct KernArgs {
    const void *in;
    float2 *out;
    const float2 *hist;
    float2 *new_hist;
    const uint8_t *rhist;
    uint8_t *new_rhist;
    const float2 *taps;
    size_t n_in;
    Geom G;
    Plan L;
    EwProgram P;
    Fix F;
    Batch B;
    unsigned long long *stamps;
};
typedef const KernArgs __attribute__((address_space(4))) *KernArgsP;
#define HZ_COLD_ARGS                                                                                                   \
    KernArgsP ca_ = (KernArgsP)__builtin_amdgcn_kernarg_segment_ptr();                                                 \
    asm volatile("" : "+s"(ca_));                                                                                      \
    [[maybe_unused]] const void *const in = ca_->in;                                                                   \
    [[maybe_unused]] float2 *const out = ca_->out;                                                                     \
    [[maybe_unused]] const float2 *const hist = ca_->hist;                                                             \
    [[maybe_unused]] float2 *const new_hist = ca_->new_hist;                                                           \
    [[maybe_unused]] const uint8_t *const rhist = ca_->rhist;                                                          \
    [[maybe_unused]] uint8_t *const new_rhist = ca_->new_rhist;                                                        \
    [[maybe_unused]] const float2 *const taps = ca_->taps;                                                             \
    [[maybe_unused]] const size_t n_in = ca_->n_in;                                                                    \
    [[maybe_unused]] const Geom &G = *(const Geom *)&ca_->G;                                                           \
    [[maybe_unused]] const Plan &L = *(const Plan *)&ca_->L;                                                           \
    [[maybe_unused]] const EwProgram &P = *(const EwProgram *)&ca_->P;                                                 \
    [[maybe_unused]] const Fix &F = *(const Fix *)&ca_->F;                                                             \
    [[maybe_unused]] const Batch &B = *(const Batch *)&ca_->B

// A Shift stage of a program with SEVERAL Shift stages (float64 phases, as hz_firmm.h), over a lane's outputs
// m = mb + 32 kT b + a of a pass: OUT OF LINE.  Inlined, its two float64 Sincos put twenty-two polynomial constants
// into vector registers at the kernel's head -- loop-invariant, so hoisted, for every wave of every launch -- for a
// path that a chain with one Shift never takes.  `y` travels through memory (the caller copies: its own outputs
// stay in registers).
template <int D, int NB>
__device__ __attribute__((noinline)) void other_shift_stage(float2 *y, double tau_shift, double step, double ts0, int l) {
    double cs0, cc0, fs, fc;
    sincos_late(__dmul_rn(tau_shift, ts0), cs0, cc0);
    const double mult = l == 0 ? (double)D : (double)(32 * kT * D);
    sincos_late(__dmul_rn(tau_shift, __dmul_rn(mult, step)), fs, fc);
    const double e_s = __shfl(fs, 0), e_c = __shfl(fc, 0), b_s = __shfl(fs, 1), b_c = __shfl(fc, 1);
    auto mul32 = [](float2 v, double c, double sn) {
        const float cr = (float)c, ci = (float)sn;
        return make_float2(__fmaf_rn(v.x, cr, -(v.y * ci)), __fmaf_rn(v.x, ci, v.y * cr));
    };
#pragma unroll
    for (int b = 0; b < NB; b++) {
        double zc = cc0, zs = cs0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            y[4 * b + q] = mul32(y[4 * b + q], zc, zs);
            if (q < 3) {
                const double nc = __fma_rn(zc, e_c, -(zs * e_s)), ns = __fma_rn(zc, e_s, zs * e_c);
                zc = nc;
                zs = ns;
            }
        }
        if (b + 1 < NB) {
            const double nc = __fma_rn(cc0, b_c, -(cs0 * b_s)), ns = __fma_rn(cc0, b_s, cs0 * b_c);
            cc0 = nc;
            cs0 = ns;
        }
    }
}

typedef float v2f __attribute__((ext_vector_type(2)));

// EXP: the kernel's compile-time switches.  The library's instantiations differ by the two loop forms alone
// (hz_firmm2.hip); the others are for the tools that measure the kernel as shipped (tools/mfma_fir2.hip,
// tools/mm2_glitch.hip).  The numbers are those of the records under profiles/.
enum : int {
    kExpNoLoads = 1,            // ablation: no input loads
    kExpNoMatrix = 2,           // ablation: no matrix loop
    kExpNoMixer = 4,            // ablation: no elementwise program
    kExpNoStores = 8,           // ablation: no output stores
    kExpPriorities = 32,        // wave priorities (see the pass loop's end)
    kExpStamps = 64,            // s_memrealtime stamps per wave and phase, staged in LDS
    kExpNoVmClear = 128,        // no explicit vmcnt(0) behind a landing
    kExpChecksums = 256,        // the pair loop's accumulator checksums per pass and lane, taken right behind the matrix
                                // loop and again behind the landing, stored (first launch) or compared (tools/mm2_glitch.hip)
    kExpStampPerPass = 1 << 24, // with kExpStamps: a row of stamps for every pass of the wave, up to fifteen
    kExpPlane = 1 << 29,        // loop form: one digit plane per A fragment, plane 0 on its window of step pairs
    kExpReuse = 1 << 30,        // loop form, with kExpPlane: the per-plane loop that re-uses its tile windows
};
// NG: the window's groups (ks / GS) when the instantiation is for ONE tap count -- the matrix loop is then
// straight-line code (a loop header drains the operand pipeline: the compiler cannot count outstanding
// loads across a back edge); 0: any window, a loop over the groups.
template <int FMT, int D, int NG = 0, int EXP = 0, int UG = 0>
__global__ __launch_bounds__(kThreads) void fir_mm2_kernel(
    const void *__restrict__ in, float2 *__restrict__ out, const float2 *__restrict__ hist,
    float2 *__restrict__ new_hist, const uint8_t *__restrict__ rhist, uint8_t *__restrict__ new_rhist,
    const float2 *__restrict__ taps, size_t n_in, Geom G, Plan L, EwProgram P, Fix F, Batch B,
    unsigned long long *stamps = nullptr) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mm_lds[];
    constexpr int TB = tile_bytes(D), PPT = TB / 16, GS = PPT / 2, NB = blocks_for(D);
    constexpr int kPassOut = pass_out(D);
    // pieces per lane of a pass image: known when the window is (NG groups: pass_tiles - 1 + NG tiles of PPT pieces)
    // the matrix loop as straight-line code (NG > 0, UG = 0) or as a loop of UG groups per trip
    constexpr bool STRAIGHT = NG > 0 && UG == 0;
    constexpr int KU = NG > 0 ? ((pass_tiles(D) - 1 + NG) * PPT + 63) / 64 : kU;
    constexpr bool kWhole = NG > 0 && ((pass_tiles(D) - 1 + NG) * PPT) % 64 == 0;  // every lane has KU pieces
    // (kExpPlane: the straight-line form at D = 8 with ONE digit plane per A fragment -- v_mfma_i32_16x16x64_i8 over PAIRS
    // of steps, plane 0 only on the pairs [G.p0_lo, G.p0_hi) where some tap can have a nonzero top digit; see the loop)
    constexpr bool kPlane = STRAIGHT && D == 8 && (EXP & kExpPlane) != 0;
    static_assert(!kPlane || (EXP & kExpChecksums) == 0, "the checksums are the pair loop's");
    static_assert(!kPlane || plane_form(D, NG * GS, 0), "the host sizes the LDS by plane_form");
    // (kExpReuse, with kExpPlane: the per-plane loop with the tiles interleaved over the column blocks -- a pair's B fragments
    // are the fragments of two pairs earlier, one column block on, in the same lane: ONE tile-window read per pair instead
    // of four; the slots in their own layout and the epilogue's exchange through LDS -- hz_firmm2_plan.h, reuse_form)
    constexpr bool kReuse = kPlane && (EXP & kExpReuse) != 0;
    static_assert((EXP & kExpReuse) == 0 || kPlane, "the re-using loop is a per-plane loop");
    static_assert(!kReuse || kXchgBytes == 2 * 64 * 16, "two quads per lane and half in the exchange area");
    // (the per-plane loop's slots: tiles 160 bytes apart, its reads are conflict-free there -- hz_firmm2_plan.h)
    constexpr int TS = tile_stride(D, kPlane);
    // (a tile's row in the slot)
    auto row_at = [](int r) { return kReuse ? reuse_row_offset(r) : TS * r; };
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
    const int wb = blockIdx.x;
    const int n = l & 31, h = l >> 5;
    const size_t tab_lds = table_lds(G.ne), slot_sz = form_slot_bytes(D, G.ks, kPlane, kReuse);
    uint8_t *const tabp = mm_lds;
    unsigned *const ctr = reinterpret_cast<unsigned *>(mm_lds + 2 * tab_lds);
    uint8_t *const slot = mm_lds + 2 * tab_lds + kCtlBytes + (size_t)wave * slot_sz;
    const uint8_t *src = (const uint8_t *)in;
    const int pieces = (int)(image_bytes(D, G.ks) / 16);
    // A call over several buffers (hz_firmm2_plan.h: Batch): `in` / `out` are buffer 0's, buffer j's virtual base is
    // read when a pass of buffer j comes up; everything is indexed by the position in the concatenation.
    const int nbuf = B.nbuf;
    const uint32_t rcp = B.rcp;
    const int64_t nb = (int64_t)B.nb;
    // (pass / ppb by the host's reciprocal: one s_mul_hi_u32 -- a chain of comparisons summed as integers became
    // vector instructions, fifty per pass)
    auto buf_of = [&](uint32_t pass) -> int { return nbuf > 1 ? (int)__umulhi(pass, rcp) : 0; };
    // (as integers, used through GLOBAL pointers: a pointer made from an integer is a generic one to the compiler, and
    // a flat load counts as an LDS operation too -- the matrix loop's first ds_read would wait for the prefetch)
    auto vin_of = [&](int j) -> uint64_t { return j == 0 ? (uint64_t)(uintptr_t)src : B.vin[j]; };
    auto vout_of = [&](int j) -> uint64_t { return j == 0 ? (uint64_t)(uintptr_t)out : B.vout[j]; };
    typedef const v4i __attribute__((address_space(1))) *gload_p;
    // (kExpStamps: s_memrealtime stamps, 10 ns ticks: slot 0 of a wave = its start and end, slots 1 .. 3 its passes)
    // The stamps are kept in LDS (2 KB behind the kernel's own: the harness asks for them) and written out when the wave
    // ends: a global store does not issue while the SIMD partner's MFMAs are back to back (tools/epi_cost.hip), so a
    // stamp stored at once pinned the very phases it was to time to the partner's loop (rounds 3-4 read "the epilogue
    // takes as long as the partner's loop" off such stamps).
    // (kExpStampPerPass, with kExpStamps: a row of stamps for EVERY pass of the wave, up to fifteen -- a call over four buffers gives a wave
    // eight; 8 KB of staging behind the kernel's own LDS, which the harness asks for -- tools/mfma_fir2.hip PASSES=1)
    // (the per-plane form's LDS leaves 2 KB of the CU's 160: its stamped builds stage the stamps where the fix-up task's
    // scratch is, and the scratch moves onto the slots of waves 0 and 1, retired by then -- behind a barrier that the
    // shipped kernel does not need; the harness asks for no LDS beyond the kernel's own)
    constexpr bool kStampShare = kPlane && (EXP & kExpStamps) != 0;
    static_assert(!kStampShare || (8 * 16 * 8 * kWaves <= 8192 && 2 * form_slot_bytes(D, NG * GS, true, kReuse) >= task_bytes(D, 1025)), "the shared areas fit");
    constexpr int kStampRows = (EXP & kExpStampPerPass) != 0 ? 16 : 4;
    int stamp_pass = 0;
    [[maybe_unused]] unsigned long long *const lstamp =
        reinterpret_cast<unsigned long long *>(mm_lds + form_lds_bytes(D, G.ks, G.ne, G.ntaps, kPlane, kReuse) - (kStampShare ? task_bytes(D, G.ntaps) : 0)) +
        (size_t)wave * (8 * kStampRows);
    if constexpr ((EXP & kExpStamps) != 0) {
        for (int i = l; i < 8 * kStampRows; i += 64) lstamp[i] = 0;
    }
    auto stamp = [&](int k) {
        if constexpr ((EXP & kExpStamps) != 0) {
            if (l == 0 && stamp_pass < kStampRows)
                lstamp[(k == 0 || k == 7 || (k >= 8 && k < 16) ? 0 : stamp_pass) * 8 + (k & 7)] = __builtin_amdgcn_s_memrealtime();
        }
    };
    stamp(0);
    // (with the stamps: the shader clock the workgroup ran at -- s_memtime counts shader cycles, s_memrealtime 100 MHz)
    [[maybe_unused]] unsigned long long clk0 = 0, rt0 = 0;
    if constexpr ((EXP & kExpStamps) != 0) clk0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
    if constexpr ((EXP & kExpPriorities) != 0) __builtin_amdgcn_s_setprio(1);
    const Run run0 = L.run[0];  // (read with the header: most workgroups of most calls are in run 0)
    // Everything the way to the first loads reads from the kernel arguments, wanted HERE: the compiler then issues
    // these scalar loads together and waits once (left alone it reads each next to its use: five load-wait
    // groups, ~0.6 us each through the scalar cache while every wave of the chip asks, before the first byte was
    // requested).
    {
        const uint64_t a0 = (uint64_t)(uintptr_t)in, a1 = (uint64_t)n_in, a2 = (uint64_t)(uintptr_t)run0.tab;
        asm volatile("" ::"s"(a0), "s"(a1), "s"(a2), "s"(G.w0), "s"(G.ks), "s"(G.ne), "s"(G.e0), "s"(G.ntaps), "s"(G.off), "s"(L.n),
                     "s"(L.n_pass), "s"(L.grid), "s"(L.n_task), "s"(L.pass_first[0]), "s"(L.pass_end[0]), "s"(L.pass_first[1]),
                     "s"(L.pass_end[1]), "s"(run0.m_lo), "s"(run0.m_hi), "s"(nbuf), "s"(rcp), "s"(nb));
    }

    // ---- this workgroup's passes [pb0, pb1) of the call -------------------------------------------------
    const uint32_t NP = (uint32_t)L.n_pass;
    // (NP / grid passes each, the first NP % grid workgroups one more; 32-bit arithmetic)
    const uint32_t per = NP / (uint32_t)L.grid, rem = NP - per * (uint32_t)L.grid;
    const uint32_t pb0 = (uint32_t)wb * per + min((uint32_t)wb, rem), pb1 = pb0 + per + ((uint32_t)wb < rem ? 1u : 0u);

    // The bytes of a pass: lane l takes pieces l, l + 64, ...  A pass that lies inside the buffer (all but the
    // call's first and last) is prefetched into registers while the previous pass multiplies (issue, then
    // land); the others are brought in piece by piece when their turn comes (land_edge: bytes before the
    // buffer are the previous call's last samples when the clock run continues, zeros otherwise).
    auto pass_p0 = [&](uint32_t pass) { return 2 * ((int64_t)D * ((int64_t)pass * kPassOut) - G.w0); };
    auto inside = [&](uint32_t pass) {  // (the image lies in ONE buffer)
        const int64_t p0 = pass_p0(pass), lo = (int64_t)buf_of(pass) * nb;
        return p0 >= lo && p0 + 16 * (int64_t)pieces <= lo + nb;
    };
    auto issue = [&](v4i(&x)[KU], uint32_t pass) {
        const gload_p p = (gload_p)(vin_of(buf_of(pass)) + (uint64_t)pass_p0(pass));  // (in pieces of 16 bytes)
        const gload_p pl = p + l;  // (ONE address per lane, the pieces at immediate offsets)
#pragma unroll
        for (int u = 0; u < KU; u++) {
            x[u] = v4i{0, 0, 0, 0};  // (pieces past the image: the last piece again, not landed)
            if constexpr ((EXP & kExpNoLoads) != 0) continue;
            if constexpr (kWhole) x[u] = __builtin_nontemporal_load(pl + 64 * u);
            else x[u] = __builtin_nontemporal_load(p + min(l + u * 64, pieces - 1));
        }
    };
    // The first pass's bytes, requested before anything else is even fetched: the instruction cache is cold at every
    // launch, and the path from the kernel's first instruction to this one decides when the matrix pipes start
    // (measured: 2.4 us of the kernel's first 5.5 went by between two stamps with ~300 instructions in between).
    // Waves 0-3 take passes pb0 .. pb0 + 3 when those lie in run 0 (the group loop below checks that it agrees).
    // (The first run's TABLE asked for here as well, 0.7 us ahead of the group loop's head where it is: medians 37.8-38.4
    // against 37.9-38.9 us, minima 36.7-36.9 against 36.3-36.4, interleaved on one box -- nothing, and not kept.)
    v4i x[KU];
    bool pre_issued = false;
    if (wave < kWaves / 2) {
        const uint32_t p = pb0 + (uint32_t)wave;
        if (pb0 >= (uint32_t)L.pass_first[0] && p < min(pb1, (uint32_t)L.pass_end[0]) && inside(p)) {
            issue(x, p);
            pre_issued = true;
        }
    }
    // ---- the small tasks: waves 0-3 of a workgroup, behind their last pass (the calls are at the kernel's end) ------
    // A FIX-UP TASK = 16 outputs in reference order (direct form, float64).  One wave alone took 18-27 us over one
    // (measured: ~3000 instructions per lane, every load a full trip): workgroup t takes task t, its four old
    // waves stage the window's 1144 samples together (load, convert, the elementwise program: five per thread,
    // all loads in flight at once) into a scratch of their own in LDS while the young waves run the workgroup's
    // last pass, and behind the barrier the same 256 threads -- 16 per output, 64 taps each -- sum and store.  One
    // per workgroup and round: a call with more fix-up tasks than four rounds keeps the transform kernels (the host).
    // A HISTORY TASK = 64 samples of the next call's history, one old wave each.
    using RWT = typename Raw<FMT>::t;
    uint32_t fix_m0 = 0;
    int fix_cnt = 0;
    // (the tasks' scratch in LDS behind the slots: the window's samples, the taps beside them)
    auto task_xs = [&](const Geom &G) {
        return reinterpret_cast<float2 *>(mm_lds + 2 * table_lds(G.ne) + kCtlBytes + (kStampShare ? 0 : (size_t)kWaves * form_slot_bytes(D, G.ks, kPlane, kReuse)));
    };
    auto tasks_front_cold = [&](int round, const void *in, const float2 *hist, float2 *new_hist, const uint8_t *rhist, uint8_t *new_rhist,
                                const float2 *taps, size_t n_in, const Geom &G, const Plan &L, const EwProgram &P, const Fix &F, const Batch &B) {
        // (sample pu of the concatenation: its buffer's virtual base)
        auto vbase = [&](int64_t pu) -> const RWT * {
            const void *sb = in;
            for (int i = 1; i < B.nbuf; i++)
                if (2 * pu >= (int64_t)i * (int64_t)B.nb) sb = (const void *)(uintptr_t)B.vin[i];
            return (const RWT *)sb;
        };
        float2 *const xs = task_xs(G);
        float2 *const tl = xs + (G.ntaps + D * (kFixOut - 1));
        const int ftask = (L.grid - 1 - wb) + round * L.grid;  // (from the grid's far end: see the calls)
        if (ftask < L.n_task) {
            const int ct = tid;  // 0 .. 255: the old waves
            const int k = find_le(F.task_first, F.n, ftask);
            fix_m0 = F.m_a[k] + (uint32_t)(ftask - F.task_first[k]) * kFixOut;
            fix_cnt = (int)min((uint32_t)kFixOut, F.m_b[k] - fix_m0);
            if (round == 0)
                for (int q = ct; q < G.ntaps; q += 256) tl[q] = taps[q];
            const int64_t p_lo = (int64_t)D * fix_m0 - (G.ntaps - 1);
            const int n_s = G.ntaps + D * (fix_cnt - 1);
            const NcoWin tw = task_window(P, p_lo, p_lo + n_s - 1);
#pragma unroll 1
            for (int i0 = ct; i0 < n_s; i0 += 5 * 256) {  // (one trip up to 1280 samples: 1160 taps)
                constexpr int W = 5;
                float2 v[W];
#pragma unroll
                for (int u = 0; u < W; u++) {
                    const int64_t pu = p_lo + i0 + u * 256;
                    v[u] = Raw<FMT>::cvt((i0 + u * 256 < n_s && pu >= 0) ? vbase(pu)[pu] : RWT{});
                }
                ew_apply_n<W, 2>(P, v, (uint64_t)(p_lo + i0), tw, (uint64_t)256);
#pragma unroll
                for (int u = 0; u < W; u++) {
                    const int idx = i0 + u * 256;
                    const int64_t pu = p_lo + idx;
                    if (idx < n_s)
                        xs[idx] = pu >= 0 ? v[u] : ((hist && pu + (int64_t)G.off >= 0) ? hist[pu + (int64_t)G.off] : make_float2(0.f, 0.f));
                }
            }
        }
    };
    // A HISTORY TASK = 64 samples of the next call's history (the stages in reference order, and the raw samples): task
    // j goes to workgroup j mod grid, one wave each, and it is the OLD waves that take them, BEHIND their last pass:
    // waves 0-3 are through with their passes ~5 us before waves 4-7, who run the workgroup's last pass alone.  (Round
    // 3 had wave 7 of the first sixteen workgroups do them in front of its first pass -- 5 us of exact Sincos that
    // made those waves, and with them the launch, end 2 us late: tools/mfma_fir2.hip lists the workgroups that end
    // last, and they were workgroups 3 and 11 on every box.)
    auto history_tasks_cold = [&](const void *in0, const float2 *hist, float2 *new_hist, const uint8_t *rhist, uint8_t *new_rhist, size_t n_in,
                                  const Geom &G, const Plan &L, const EwProgram &P, const Batch &B) {
        // (the call's last samples: the last buffer's, which holds at least `off` samples when there are several)
        const void *const in = B.nbuf > 1 ? (const void *)(uintptr_t)B.vin[B.nbuf - 1] : in0;
        const int n_hist_tasks = new_hist ? (int)((G.off + kHistPer - 1) / kHistPer) : 0;
        for (int j = wb + L.grid * wave; j < n_hist_tasks; j += (kWaves / 2) * L.grid) {  // (uniform per wave)
            const unsigned idx = (unsigned)j * kHistPer + l;
            const int64_t h_lo = (int64_t)n_in - (int64_t)G.off + (int64_t)j * kHistPer;
            const NcoWin tw = task_window(P, h_lo, h_lo + kHistPer - 1);
            if (idx < G.off) {
                const int64_t p = (int64_t)n_in - (int64_t)G.off + idx;
                new_hist[idx] = mm::ordered_sample<FMT, 2>(in, P, p, hist, G.off, tw);  // (the tasks' own Sincos flavour: hz_firmm.h)
                reinterpret_cast<RWT *>(new_rhist)[idx] = p >= 0 ? ((const RWT *)in)[p] : reinterpret_cast<const RWT *>(rhist)[p + (int64_t)G.off];
            }
        }
    };
    auto history_tasks = [&]() {
        if (wave >= kWaves / 2 || new_hist == nullptr || wb + L.grid * wave >= (int)((G.off + kHistPer - 1) / kHistPer)) return;
        HZ_COLD_ARGS;
        history_tasks_cold(in, hist, new_hist, rhist, new_rhist, n_in, G, L, P, B);
    };
    // Round r: workgroup wb takes fix-up task wb + r grid.  Round 0 is called ONCE, in front of the run groups, the
    // further rounds of a call with more tasks than workgroups (short calls across many clock boundaries) BEHIND them
    // -- never inside the groups' loop: what a call site inside a loop derives from loop-invariant values (the exact
    // Sincos' twenty-two polynomial constants, for one) is hoisted to the loop's head, i.e. into every launch's first
    // microseconds.
    auto tasks_front = [&](int round) {
        if (wave >= kWaves / 2) return;
        if ((L.grid - 1 - wb) + round * L.grid >= L.n_task) return;  // (what most workgroups of most calls find)
        HZ_COLD_ARGS;
        tasks_front_cold(round, in, hist, new_hist, rhist, new_rhist, taps, n_in, G, L, P, F, B);
    };
    auto tasks_back_cold = [&](float2 *out0, const Geom &G, const Batch &B) {
        float2 *const xs = task_xs(G);
        float2 *const tl = xs + (G.ntaps + D * (kFixOut - 1));
        const int ct = tid;
        const int o = ct >> 4, sl = ct & 15;  // output, tap slice: sixteen lanes per output
        // a lane's 64 (ntaps / 16) taps in float64, like the chunk kernel's tasks (hz_firmm.h).  (Until
        // tests/test_gpu_fir_exact.py these were two packed float32 fma chains per lane, "a chain of 64 terms stays
        // below 1e-7": under a boxcar and a constant input -- every product of one sign -- the fix-up outputs were 3.9e-7
        // from the oracle in relative L2, past the bound every FIR output is held to.)
        double ar = 0.0, ai = 0.0;
        if (o < fix_cnt) {
            const float2 *xo = xs + D * o + (G.ntaps - 1);
#pragma unroll 4
            for (int kk = sl; kk < G.ntaps; kk += 16) {
                const float2 hk = tl[kk], x = xo[-kk];
                const double xr = x.x, xi = x.y, hr = hk.x, hi = hk.y;
                ar = __fma_rn(xr, hr, ar);
                ar = __fma_rn(-xi, hi, ar);
                ai = __fma_rn(xr, hi, ai);
                ai = __fma_rn(xi, hr, ai);
            }
        }
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            ar += __shfl_xor(ar, d);
            ai += __shfl_xor(ai, d);
        }
        if (o < fix_cnt && sl == 0) {
            float2 *ob = out0;  // (output fix_m0 + o of the concatenation: its buffer's virtual base)
            for (int i = 1; i < B.nbuf; i++)
                if (fix_m0 + o >= (uint32_t)i * B.out_each) ob = (float2 *)(uintptr_t)B.vout[i];
            ob[fix_m0 + o] = make_float2((float)ar, (float)ai);
        }
        fix_cnt = 0;
    };
    auto tasks_back = [&]() {  // behind the barrier that follows tasks_front
        if (wave >= kWaves / 2 || fix_cnt == 0) return;
        HZ_COLD_ARGS;
        tasks_back_cold(out, G, B);
    };
    stamp(9);
    auto put = [&](int q, v4i v) {
        if constexpr (FMT == HZSDR_FMT_U8) v ^= (int)0x80808080;  // b - 128 as int8
        *reinterpret_cast<v4i *>(slot + row_at(q / PPT) + 16 * (q % PPT)) = v;
    };
    // The compiler's s_waitcnt pass keeps a load "pending" on every path it cannot prove a wait on (a conditional
    // consumer is enough), right around the pass loop; with stores in flight as well -- loads and stores return out of
    // order -- each later write of such a register becomes s_waitcnt vmcnt(0).  Two of those sat in the pass loop:
    // at its head (the previous pass's stores drained before the queue was read) and in front of the matrix loop
    // (the prefetch just issued waited for, instead of flying under the matrix loop).  An explicit vmcnt(0) where
    // nothing is in flight anyway -- after a landing -- tells the pass so.
    auto vm_clear = [&]() {
        if constexpr ((EXP & kExpNoVmClear) == 0) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), the other counters untouched
    };
    // (flipped: the u8 sign flip has been applied to the registers already -- among the MFMAs of the matrix loop the
    // bytes were in flight under; straight-line forms)
    auto land = [&](v4i(&x)[KU], bool flipped = false) {
        // piece l + 64 u is piece l % PPT of tile l / PPT + (64 / PPT) u: one address and constants
        // (the re-using loop's rows: 64 / PPT = 8 rows on is two whole groups of four rows on, a constant all the same)
        uint8_t *lp = slot + row_at(l / PPT) + 16 * (l % PPT);
        constexpr int kLandStep = kReuse ? reuse_row_offset(64 / PPT) : (64 / PPT) * TS;
        static_assert(!kReuse || (64 / PPT) % 4 == 0, "whole groups of four rows");
        // (the rare un-flipped landing -- a wave's first pass, a pass behind an inactive one -- as a BRANCH.  The
        // condition is uniform, and the compiler turned `if (!flipped) x ^= c` into 40 v_xor + 40 v_cndmask executed
        // by EVERY landing: 80 of a pass's ~490 vector instructions, each of which costs the SIMD partner's matrix loop
        // ~2.5 cycles -- found in the ISA in round 6.  The empty asm keeps the block from being if-converted again.)
        if constexpr (FMT == HZSDR_FMT_U8 && STRAIGHT) {
            if (!flipped) {
#pragma unroll
                for (int u = 0; u < KU; u++) {
                    x[u] ^= (int)0x80808080;
                    asm volatile("" : "+v"(x[u]));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
            if (kWhole || l + u * 64 < pieces) {
                // (the straight-line forms: flipped among the MFMAs, or above in one uniform branch)
                if constexpr (FMT == HZSDR_FMT_U8 && !STRAIGHT) x[u] ^= (int)0x80808080;  // b - 128 as int8
                *reinterpret_cast<v4i *>(lp + u * kLandStep) = x[u];
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto land_edge_cold = [&](uint32_t pass, const uint8_t *src, const uint8_t *rhist, int64_t n_bytes, const Geom &G, const Plan &L, const Batch &B) {
        const int64_t p0 = 2 * ((int64_t)D * ((int64_t)pass * kPassOut) - G.w0);
        const int pieces = (int)(image_bytes(D, G.ks) / 16);
#pragma unroll 1
        for (int q = l; q < pieces; q += 64) {
            const int64_t p = p0 + (int64_t)q * 16;
            v4i v{0, 0, 0, 0};
            if (p >= 0 && p + 16 <= n_bytes) {
                // (a piece never straddles two buffers: their length is a multiple of 16 bytes)
                uint64_t sb = (uint64_t)(uintptr_t)src;
                for (int i = 1; i < B.nbuf; i++)
                    if (p >= (int64_t)i * (int64_t)B.nb) sb = B.vin[i];
                v = *(const v4i __attribute__((address_space(1))) *)(sb + (uint64_t)p);
            } else if (p < 0 && L.cont && p + 2 * (int64_t)G.off >= 0) {
                v = *reinterpret_cast<const v4i *>(rhist + (p + 2 * (int64_t)G.off));  // (2 off is a multiple of 16)
            } else if (p + 16 > 0 && p < n_bytes) {  // straddles the buffer's end: byte by byte
                uint64_t w0 = 0, w1 = 0;  // (no byte array: it would live in scratch memory)
#pragma unroll 1
                for (int e = 0; e < 16; e++)
                    if (p + e >= 0 && p + e < n_bytes) {
                        const uint64_t bb = src[p + e];
                        if (e < 8) w0 |= bb << (8 * e);
                        else w1 |= bb << (8 * (e - 8));
                    }
                v = v4i{(int)(uint32_t)w0, (int)(uint32_t)(w0 >> 32), (int)(uint32_t)w1, (int)(uint32_t)(w1 >> 32)};
            }
            put(q, v);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    auto land_edge = [&](uint32_t pass) {  // (the call's first and last passes)
        HZ_COLD_ARGS;
        land_edge_cold(pass, (const uint8_t *)in, rhist, 2 * (int64_t)n_in, G, L, B);
    };

    // A fragments: lane n is row (a = n >> 3, c = (n >> 2) & 1, part = (n >> 1) & 1, pl = n & 1) = output
    // i = 4 c + a of the tile -- the accumulator then holds FOUR CONSECUTIVE outputs per lane (row =
    // 8 (q >> 2) + 4 (l >> 5) + (q & 3)): entry (D/8) i - h - 2 s + e0, 64 bytes per entry and fragment row
    const int i_row = 4 * ((n >> 2) & 1) + (n >> 3);
    const int a_base = 64 * ((D / 8) * i_row - h + G.e0) + 16 * (n & 3);
    const int f_stride = G.ne * 64;
    const int groups = NG > 0 ? NG : G.ks / GS;  // (NG > 0: the host launches this instantiation for ks = NG GS only)

    // The per-plane matrix loop (kPlane).  The pair loop's A fragment holds TWO digit planes (rows: 8 outputs x (re, im)
    // x planes 2 f, 2 f + 1), and for most taps of a decimating low-pass the top plane is zero: |q| <= 127 (2^16 + 2^8 + 1)
    // (hz_firmm2_plan.h, plane0_window) -- the tails of a windowed sinc, 70 % of the taps of the benchmarked filter.  The
    // MFMA still runs, half of its rows zero, at ~0.8 of a full one's energy, and at the chip's power cap energy is time
    // (DESIGN section 4).  Here a fragment is ONE plane: v_mfma_i32_16x16x64_i8, rows = 8 outputs x (re, im), K = 64
    // bytes = two of the pair loop's steps, columns = 16 tiles; four column blocks = the pass's 64 tiles, sixteen
    // accumulators of four registers (the same 64).  Plane 0's MFMAs run on the pairs [G.p0_lo, G.p0_hi) only, one
    // uniform branch per pair.  Lane l: A row l & 15 (output (l & 15) >> 1, part l & 1), B column l & 15, K piece
    // kq = l >> 4 of the pair -- piece kq of the tile's window at 64 t bytes, and the table's entry E = (D / 8) i - kq -
    // 4 t + e0, whose part and plane rows are the pair loop's own (T[f][E][part][pl]): no other table in memory -- in LDS
    // the group's staging copy has put it plane-major, P[plane][E][part] (hz_firmm2_plan.h, plane_piece: in T's order a
    // lane group's sixteen rows lie on eight 16-byte bank groups, and every A read took twice its cycles).  Operands one
    // pair ahead, one LDS read behind each of the first eight MFMAs; plane 0's operand is read on every pair (a read is
    // cheap, a branch in the middle of the reads is not).  tools/mfma_plane_skip.hip prices the two loops bare.
    [[maybe_unused]] auto plane_loop = [&](v4i(&pa)[4][4], int tab_off) {
        constexpr int KP = NG * GS / 2;                             // step pairs
        constexpr int NE = 2 * (2 * KP + 4) + (D / 8) * (kT - 1) + 1;  // (G.ne)
        const int r16 = l & 15, kq = l >> 4;
        // (the lane's entry of the LAST pair, kept from folding back: DS offsets are unsigned)
        int a_off = plane_a_offset(NE, G.e0, 0, KP - 1, r16, kq) + tab_off;
        asm volatile("" : "+v"(a_off));
        const uint8_t *ap = tabp + a_off;
        // (the re-using loop: column r16 of block j is tile 4 r16 + j -- the lane's rows start at row 4 r16)
        const uint8_t *bp = slot + row_at(kReuse ? 4 * r16 : r16) + 16 * kq;
        // (plane 0's pairs as a bit mask in scalar registers, made opaque at every pair: left to itself the compiler
        // hoists the 34 comparisons to the kernel's head and keeps them as lane masks in a VGPR, two v_readlane each)
        uint64_t p0_mask = (G.p0_hi >= 64 ? ~0ull : (1ull << G.p0_hi) - 1) & ~((1ull << G.p0_lo) - 1);
        v4i a[2][4], b[2][4];
        auto load = [&](auto tc) {  // pair t's operands, in the order the pair uses them (plane 0 last)
            constexpr int t = decltype(tc)::value, r = t & 1;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int p = u == 0 ? 1 : u < 5 ? -1 : u == 7 ? 0 : u - 3, j = u - 1;
                if (p >= 0) a[r][p] = *reinterpret_cast<const v4i *>(ap + 32 * NE * p + 128 * (KP - 1 - t));
                else if constexpr (!kReuse) b[r][j] = *reinterpret_cast<const v4i *>(bp + TS * (16 * j + t / 2) + 64 * (t & 1));
                // (rows j + t / 2 past the lane's first; from pair 2 on the last block's alone, into the register of
                // the fragment that died two pairs earlier -- the other three are there already)
                else if (reuse_b_read(j, t)) b[r][reuse_b_reg(j, t)] = *reinterpret_cast<const v4i *>(bp + reuse_row_offset(j + t / 2) + 64 * (t & 1));
            }
        };
        // the B registers of pair t: block j's fragment
        auto bsel = [](int j, int t) { return kReuse ? reuse_b_reg(j, t) : j; };
        // (planes 1 .. 3 are written by the first pair's MFMAs, the constant 0 as C: plane 0 alone is cleared)
#pragma unroll
        for (int j = 0; j < 4; j++) pa[0][j] = v4i{0, 0, 0, 0};
        load(std::integral_constant<int, 0>{});
        auto pair = [&](auto self, auto tc) {
            constexpr int t = decltype(tc)::value, r = t & 1;
            if constexpr (t < KP) {
                if constexpr (t + 1 < KP) load(std::integral_constant<int, t + 1>{});
#pragma unroll
                for (int p = 1; p < 4; p++)
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        // (inline assembly with early-clobber destinations: no clears, no overlap of destinations and sources)
                        if constexpr (t == 0)
                            asm volatile("v_mfma_i32_16x16x64_i8 %0, %1, %2, 0" : "=&v"(pa[p][j]) : "v"(a[r][p]), "v"(b[r][bsel(j, t)]));
                        else
                            pa[p][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[r][p], b[r][bsel(j, t)], pa[p][j], 0, 0, 0);
                    }
                // (u8: the next pass's bytes get their sign flip here, in the shadow of the wave's own MFMAs -- as in the
                // pair loop, four registers per pair, done a pair before the end)
                if constexpr (FMT == HZSDR_FMT_U8) {
                    constexpr int kFlipFirst = KP - 1 - (KU + 3) / 4;
                    if constexpr (t == kFlipFirst) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
                    if constexpr (t >= kFlipFirst && 4 * (t - kFlipFirst) < KU) {
#pragma unroll
                        for (int u = 4 * (t - kFlipFirst); u < KU && u < 4 * (t - kFlipFirst) + 4; u++) {
                            x[u] ^= (int)0x80808080;
                            asm volatile("" : "+v"(x[u]));
                        }
                    }
                }
                // (the next pair's reads, one behind each of the pair's first MFMAs: eight, or the re-using loop's five)
                constexpr int kReads = kReuse && t + 1 >= 2 ? 5 : 8;
#pragma unroll
                for (int q = 0; q < kReads; q++) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
                    if constexpr (t + 1 < KP) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // LDS read
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 12 - kReads, 0);
                __builtin_amdgcn_sched_barrier(0);
                asm volatile("" : "+s"(p0_mask));
                if ((p0_mask >> t) & 1) {  // (uniform)
#pragma unroll
                    for (int j = 0; j < 4; j++) pa[0][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[r][0], b[r][bsel(j, t)], pa[0][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                self(self, std::integral_constant<int, t + 1>{});
            }
        };
        pair(pair, std::integral_constant<int, 0>{});
    };

    bool first_seg = true, first_stamp = true;
    const double k3 = __hiloint2double((1023 - G.shift) << 20, 0), k2 = k3 * 256.0, k1 = k3 * 65536.0;  // 2^-S 256^d, d = 0, 1, 2
    // a lane holds outputs 4 h + a (a = 0 .. 3) of tile n of each block: planes 2 f + pl at q = 4 a + 2 part + pl.
    // The planes meet in float64 with power-of-two weights (exact; the constant part of a u8 stream and the scale
    // 2^-S folded in), one rounding to float32.
    auto planes = [&](const v16i(&acc)[2][NB], float2(&y)[NB][4], double dcr, double dci) {
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int aa = 0; aa < 4; aa++) {
                float c2[2];
#pragma unroll
                for (int pt = 0; pt < 2; pt++) {
                    const int q = 4 * aa + 2 * pt;
                    double v = __fma_rn((double)acc[1][b][q + 1], k3, pt ? dci : dcr);
                    v = __fma_rn((double)acc[1][b][q], k2, v);
                    // planes 0 and 1 meet in int32 (one v_lshl_add_u32 for a conversion and an fma): the host chose
                    // the taps' scale so that 256 |sum_0| + |sum_1| < 2^31 for every input (digit_shift); every
                    // partial sum of the chain is exact in float64 either way, so the result is the same bits
                    const int hi = (int)(((unsigned)acc[0][b][q] << 8) + (unsigned)acc[0][b][q + 1]);
                    v = __fma_rn((double)hi, k1, v);
                    c2[pt] = (float)v;
                }
                y[b][aa] = make_float2(c2[0], c2[1]);
            }
    };
    // The same combination over the per-plane loop's accumulators (kPlane): plane p, column block j (tiles 16 j + c), lane
    // l = 16 g + c holds rows 4 g + k = 2 i + part, i.e. outputs i = 4 (l >> 5) + 2 ((l >> 4) & 1) + (k >> 1) of tiles
    // c, 16 + c, 32 + c, 48 + c.  The pair loop's lane l = 32 h + n holds outputs 4 h + a of tiles n and 32 + n: lanes l
    // and l ^ 16 each hold half of what the other needs -- one v_permlane16_swap per pair of values (odd 16-lane rows of
    // its first operand trade with even rows of its second) puts every value where the pair loop has it.  Same operations
    // in the same order per output as `planes`: the same bits.
    auto planes16 = [&](const v4i(&pa)[4][4], float2(&y)[NB][4], double dcr, double dci) {
        float z[4][2][2];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int pt = k & 1;
                double v = __fma_rn((double)pa[3][j][k], k3, pt ? dci : dcr);
                v = __fma_rn((double)pa[2][j][k], k2, v);
                const int hi = (int)(((unsigned)pa[0][j][k] << 8) + (unsigned)pa[1][j][k]);
                v = __fma_rn((double)hi, k1, v);
                z[j][k >> 1][pt] = (float)v;
            }
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int a2 = 0; a2 < 2; a2++) {
                float w[2][2];
#pragma unroll
                for (int pt = 0; pt < 2; pt++) {
                    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(z[2 * b][a2][pt]), __float_as_uint(z[2 * b + 1][a2][pt]), false, false);
                    w[0][pt] = __uint_as_float(sw[0]);
                    w[1][pt] = __uint_as_float(sw[1]);
                }
                y[b][a2] = make_float2(w[0][0], w[0][1]);
                y[b][2 + a2] = make_float2(w[1][0], w[1][1]);
            }
    };
    // ... and over the re-using loop's (kReuse): lane 16 g + c, block j, register k holds output 2 g + (k >> 1), part k & 1
    // of tile 4 c + j.  The same combination per element, then the sixteen floats go to the lanes the pair loop has them in
    // through the 2 KB behind the wave's image (hz_firmm2_plan.h, xchg_*), one column-block half b at a time: the lanes that
    // hold tiles of half b (c >> 3 == b) write their four quads, every lane reads its two -- y[b][0 .. 3].  The wave's LDS
    // operations execute in order: no barrier, the reads' s_waitcnt alone.  Called BEHIND the landing, as planes16 is: in
    // front of it the next image's forty registers are still live beside the accumulators (measured: 236 VGPRs against
    // 224).
    [[maybe_unused]] auto planes_xchg = [&](const v4i(&pa)[4][4], float2(&y)[NB][4], double dcr, double dci) {
        typedef float v4f_ __attribute__((ext_vector_type(4)));
        static_assert(!kReuse || NB == 2, "two halves of 32 tiles");
        v4f_ z[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int pt = k & 1;
                double v = __fma_rn((double)pa[3][j][k], k3, pt ? dci : dcr);
                v = __fma_rn((double)pa[2][j][k], k2, v);
                const int hi = (int)(((unsigned)pa[0][j][k] << 8) + (unsigned)pa[1][j][k]);
                v = __fma_rn((double)hi, k1, v);
                z[j][k] = (float)v;
            }
        // (the lane's three addresses formed HERE, a dozen integer instructions per pass: left to the compiler they are
        // loop-invariant, hoisted to the kernel's head and held in registers through every matrix loop)
        int lx = l;
        asm volatile("" : "+v"(lx));
        uint8_t *const xb = slot + reuse_image_bytes(D, NG * GS);
        // (xchg_write_offset(l, j) = xchg_write_offset(l, j & 1) + 128 (j >> 1): sigma's bit 3 is the destination's bit 1)
        uint8_t *const we = xb + xchg_write_offset(lx, 0), *const wo = xb + xchg_write_offset(lx, 1);
        const uint8_t *const rp = xb + xchg_read_offset(lx, 0);
#pragma unroll
        for (int b = 0; b < 2; b++) {
            if (xchg_half(lx) == b) {
#pragma unroll
                for (int j = 0; j < 4; j++) *reinterpret_cast<v4f_ *>(((j & 1) ? wo : we) + 128 * (j >> 1)) = z[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const v4f_ w = *reinterpret_cast<const v4f_ *>(rp + 1024 * q);
                y[b][2 * q] = make_float2(w.x, w.y);
                y[b][2 * q + 1] = make_float2(w.z, w.w);
            }
            // (the other half's writes, and the next landing's, stay behind these reads: the same wave, in order)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    };
    // the elementwise program over a lane's outputs m = mb + 256 b + a of a pass in the run with phase line
    // (phi_r, dphi) / clock-table entry seg: equally spaced in two directions inside one exactly-linear clock run
    auto program = [&](float2(&y)[NB][4], uint32_t mb, uint64_t phi_r, uint64_t dphi, int seg, const float4 *wtab) {
        // The other stages of a program -- Gain, Multiply, the Shifts of a program with several -- through the cold
        // arguments (HZ_COLD_ARGS above): the stage's kind and parameters are read where they are used.  (Read the
        // ordinary way they were five dependent scalar loads per pass in front of the marked Shift.)
        auto other_stage = [&](int oi, int seg, const EwProgram &P) {
            const EwOp &o = P.op[oi];
            if (o.kind == EW_SCALE) {
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        // (scalar products, kept from being paired: a packed float32 instruction waits for the SIMD
                        // partner's matrix loop, as in the mixer)
                        float gx = __fmul_rn(y[b][q].x, o.a), gy = __fmul_rn(y[b][q].y, o.a);
                        asm volatile("" : "+v"(gx), "+v"(gy));
                        y[b][q] = make_float2(gx, gy);
                    }
            } else if (o.kind == EW_ROTATE) {
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int q = 0; q < 4; q++) y[b][q] = go_cmul(y[b][q], make_float2(o.a, o.b));
            } else {
                // (programs with several Shift stages: out of line, other_shift_stage above)
                const double step = P.segs.step[seg];
                const int64_t dj = (int64_t)((uint64_t)D * mb) - (int64_t)P.segs.first[seg];
                const double ts0 = __fma_rn((double)dj, step, P.segs.t0[seg]);
                float2 t[4 * NB];
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int q = 0; q < 4; q++) t[4 * b + q] = y[b][q];
                other_shift_stage<D, NB>(t, o.tau_shift, step, ts0, l);
#pragma unroll
                for (int b = 0; b < NB; b++)
#pragma unroll
                    for (int q = 0; q < 4; q++) y[b][q] = t[4 * b + q];
            }
        };
        // (the program's ONE marked Shift stage: the mixer)
        auto shift_stage = [&]() {
            // The stage's phase is a 64-bit accumulator in turns (exact increments, no float64).  ONE Sincos per
            // lane, for its first output; the other seven are that factor turned on by the group's step factors
            // exp(2 pi i (256 b + a) D dphi) -- double-float constants in LDS, two fma pairs and an add per
            // component (0.4 ulp rms against the 0.3 of a Sincos each, a third of the instructions: every vector
            // instruction here runs beside the SIMD partner's matrix loop and costs both waves).
            // The products are SCALAR float32 instructions: a packed one (v_pk_mul_f32 / v_pk_fma_f32) does not issue
            // beside a SIMD partner that streams MFMAs -- the mixer beside a partner's loop took 5.6 us packed and 1.2 us
            // scalar, which had pinned the epilogue to the partner's loop -- and op_sel:[0,1] with src0 straight is the
            // gfx950 hazard of hz_firmm.h besides.  The empty asm below keeps the compiler from pairing them again;
            // tools/fix_pk_opsel.py checks the built unit all the same.  (The retired forms of the mixer: DESIGN.md.)
            const uint64_t ph0 = phi_r + (uint64_t)D * mb * dphi;
            float s0, c0;
            sincos_turns32((uint32_t)(ph0 >> 32), s0, c0);
            const v2f cs0{c0, s0};
#pragma unroll
            for (int b = 0; b < NB; b++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    v2f f = cs0;
                    if (b + q > 0) {
                        typedef float v4f_ __attribute__((ext_vector_type(4)));
                        const v4f_ w = *reinterpret_cast<const v4f_ *>(wtab + 4 * b + q);  // (cos hi, sin hi, cos lo, sin lo)
                        // (the small terms first, the large ones chained on: four instructions per component)
                        f.x = __fmaf_rn(c0, w.x, __fmaf_rn(-s0, w.y, __fmaf_rn(c0, w.z, -(s0 * w.w))));
                        f.y = __fmaf_rn(c0, w.y, __fmaf_rn(s0, w.x, __fmaf_rn(c0, w.w, s0 * w.z)));
                    }
                    float rx = __fmaf_rn(y[b][q].x, f.x, -(y[b][q].y * f.y)), ry = __fmaf_rn(y[b][q].x, f.y, y[b][q].y * f.x);
                    asm volatile("" : "+v"(rx), "+v"(ry));  // (kept scalar: no re-vectorisation)
                    y[b][q] = make_float2(rx, ry);
                }
        };
        auto other_stage_at = [&](int oi) {
            HZ_COLD_ARGS;
            other_stage(oi, seg, P);
            // (a multi-Shift stage's outputs come back through scratch memory: waited for HERE -- left pending they
            // become a vmcnt(0) at the pass loop's top, behind the next pass's prefetch, and eight register moves on the
            // hot path where the two meet)
            __builtin_amdgcn_s_waitcnt(0x0F70);
        };
        const int n_ops = (EXP & kExpNoMixer) ? 0 : L.n_ops;
        // (the common program -- ONE stage, the marked Shift -- outside the loop over the stages: rolled, the loop
        // carries a lane's sixteen outputs from trip to trip through eight v_mov_b64 that every pass executed)
        if (__builtin_expect(n_ops == 1 && L.shift_op == 0, 1)) {
            shift_stage();
            return;
        }
#pragma unroll 1
        for (int oi = 0; oi < n_ops; oi++) {  // uniform
            const bool other = __builtin_expect(L.shift_op != oi, 0);  // (the cold path)
            if (other) other_stage_at(oi);
            else shift_stage();
        }
    };
    auto store_block = [&](uint64_t outb, float2(&y)[4], uint32_t mo, uint32_t lo, uint32_t hi) {  // (outb: the pass's buffer, virtual base)
        if constexpr ((EXP & kExpNoStores) != 0) return;
        typedef float v4f __attribute__((ext_vector_type(4)));
        typedef float v2f_ __attribute__((ext_vector_type(2)));
        if (mo >= lo && mo + 4 <= hi) {
            v4f __attribute__((address_space(1))) *o4 = (v4f __attribute__((address_space(1))) *)(outb + 8 * (uint64_t)mo);
            __builtin_nontemporal_store(v4f{y[0].x, y[0].y, y[1].x, y[1].y}, o4);
            __builtin_nontemporal_store(v4f{y[2].x, y[2].y, y[3].x, y[3].y}, o4 + 1);
        } else {
            v2f_ __attribute__((address_space(1))) *o2 = (v2f_ __attribute__((address_space(1))) *)(outb + 8 * (uint64_t)mo);
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (mo + q >= lo && mo + q < hi) o2[q] = v2f_{y[q].x, y[q].y};
        }
    };
    // The runs that matter to this workgroup: those with passes in [pb0, pb1).  Two tables fit the LDS: run A of a
    // group and the run B behind it are ONE queue (A's passes, B's passes); the next group slides on by one run (B
    // becomes A, its table stays) behind a barrier.
    auto has_passes = [&](int rr) { return rr < L.n && max(pb0, (uint32_t)L.pass_first[rr]) < min(pb1, (uint32_t)L.pass_end[rr]); };
    // (A pass's stores: beside a SIMD partner that issues MFMAs back to back a wave's vector instructions, LDS reads and
    // writes and global loads go through as if the partner were idle, but a global STORE does not issue until the
    // partner's stream of MFMAs pauses -- tools/epi_cost.hip.  An epilogue that ends in stores ends when the partner's
    // loop ends.  Deferring them into the wave's next matrix loop was measured 1 us per buffer SLOWER: DESIGN.md.)
    int ra = 0;
    while (ra < L.n && !has_passes(ra)) ra++;
    Run ru = run0, rv = run0;
    bool a_done = false;
    int slot_a = 0;  // the half of the table area that holds run A's table
#pragma unroll 1
    while (ra < L.n) {
        const int rb = ra + 1;
        const bool b_pass = has_passes(rb), b_here = b_pass;  // uniform
        uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
        if (!a_done && has_passes(ra)) a0 = max(pb0, (uint32_t)L.pass_first[ra]), a1 = min(pb1, (uint32_t)L.pass_end[ra]);
        if (b_pass) b0 = max(pb0, (uint32_t)L.pass_first[rb]), b1 = min(pb1, (uint32_t)L.pass_end[rb]);
        // items [0, seg_b): pass a0 + q of run A, then pass b0 + q of run B
        const uint32_t n_a = a1 - a0, seg_b = n_a + (b1 - b0);
        auto pass_of = [&](uint32_t q) { return q < n_a ? a0 + q : b0 + (q - n_a); };
        auto prefetchable = [&](uint32_t q) { return q < seg_b && inside(pass_of(q)); };
        if (!first_seg) __syncthreads();  // every wave is done with the table that goes and with the queue
        const bool first_group = first_seg;  // (the workgroup's first group: the small tasks ride on it)
        // Waves 0-3 (one per SIMD) take the queue's first items and put their bytes in flight at once;
        // waves 4-7 start behind the barrier: the first burst is half as large, and the two waves of a SIMD
        // start out of phase.
        constexpr int kEarly = kWaves / 2;
        auto grab = [&]() -> uint32_t {
            unsigned p = 0;
            if (l == 0) p = atomicAdd(ctr, 1u);
            return (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
        };
        uint32_t cur = seg_b;
        bool in0 = false;
        constexpr int kTU = 4;  // table pieces per thread (32 KB at most: the host)
        if (wave < kEarly) {
            cur = min((uint32_t)wave, seg_b);
            in0 = prefetchable(cur);  // uniform
            // (pre_issued: the kernel's first lines have requested pass pb0 + wave -- this one, in the first group)
            if (in0 && !(pre_issued && ra == 0 && !a_done && pass_of(cur) == pb0 + (uint32_t)wave)) issue(x, pass_of(cur));
            pre_issued = false;
        }
        if (first_stamp) stamp(13);
        // (everything the queue reads from the kernel arguments by run, at once)
        // (run A of a later group is the previous group's run B: the lines stay in registers, one at a time is read)
        if (!first_seg) ru = rv;
        else if (ra > 0) ru = L.run[ra];  // (one line)
        if (b_here) rv = L.run[rb];
        const int off_a = slot_a ? (int)tab_lds : 0, off_b = slot_a ? 0 : (int)tab_lds;
        {
            const int tp = (int)(table_bytes(G.ne) + 15) / 16;
            const v4i *tg = (const v4i *)ru.tab, *th = (const v4i *)rv.tab;
            // (one table after the other: both in flight at once, beside the first pass's bytes, spilled registers)
            v4i tq[kTU];
            // (the per-plane loop's table: plane-major in LDS)
            auto tab_piece = [&](int q) {
                if constexpr (kPlane) return plane_piece(2 * (NG * GS + 4) + (D / 8) * (kT - 1) + 1, q);
                else return q;
            };
            if (first_seg) {
#pragma unroll
                for (int u = 0; u < kTU; u++) tq[u] = tid + u * kThreads < tp ? tg[tid + u * kThreads] : v4i{0, 0, 0, 0};
                if (first_stamp) stamp(14);
#pragma unroll
                for (int u = 0; u < kTU; u++)
                    if (tid + u * kThreads < tp) *reinterpret_cast<v4i *>(tabp + off_a + 16 * (size_t)tab_piece(tid + u * kThreads)) = tq[u];
            }
            if (b_here) {
#pragma unroll
                for (int u = 0; u < kTU; u++) tq[u] = tid + u * kThreads < tp ? th[tid + u * kThreads] : v4i{0, 0, 0, 0};
#pragma unroll
                for (int u = 0; u < kTU; u++)
                    if (tid + u * kThreads < tp) *reinterpret_cast<v4i *>(tabp + off_b + 16 * (size_t)tab_piece(tid + u * kThreads)) = tq[u];
            }
        }
        first_seg = false;
        if (first_stamp) stamp(10);
        if (tid == 0) *ctr = kEarly;
        __syncthreads();
        if (first_stamp) stamp(11);
        if constexpr ((EXP & kExpPriorities) != 0) {
            if (first_group) __builtin_amdgcn_s_setprio(1);
        }
        if (wave >= kEarly) {
            cur = grab();
            in0 = prefetchable(cur);
            if (in0) issue(x, pass_of(cur));
        }
        if (cur < seg_b) {
            if (in0) land(x);
            else land_edge(pass_of(cur));
        }
        if (first_stamp) stamp(12);
        first_stamp = false;
        vm_clear();
#pragma unroll 1
        while (cur < seg_b) {
            stamp_pass++;
            stamp(16);
            const uint32_t nxt = grab();
            const bool has_next = nxt < seg_b, in_next = prefetchable(nxt);  // uniform
            stamp(23);
            if (in_next) issue(x, pass_of(nxt));
            stamp(1);
            const bool sel = cur >= n_a;  // uniform: the pass belongs to run B
            const uint32_t m_lo = sel ? rv.m_lo : ru.m_lo, m_hi = sel ? rv.m_hi : ru.m_hi;
            const uint64_t dphi = sel ? rv.dphi : ru.dphi, phi_r = sel ? rv.phi : ru.phi;
            const int tab_off = sel ? off_b : off_a;
            const uint32_t m_start = pass_of(cur) * (uint32_t)kPassOut;
            const uint32_t v_lo = max(m_lo, m_start), v_hi = min(m_hi, m_start + (uint32_t)kPassOut);
            const bool active = v_lo < v_hi;  // uniform
            // (the straight-line forms: the first step writes the accumulators -- the constant 0 as C, through inline
            // assembly with early-clobber destinations: no clears, no overlap of destinations and sources -- and an
            // inactive pass never reads them)
            v16i acc[2][NB];
            [[maybe_unused]] v4i pacc[4][4];
            if constexpr (!STRAIGHT) {
#pragma unroll
                for (int f = 0; f < 2; f++)
#pragma unroll
                    for (int b = 0; b < NB; b++)
#pragma unroll
                        for (int q = 0; q < 16; q++) acc[f][b][q] = 0;
            }
            if constexpr (kPlane) {
                if (active && (EXP & kExpNoMatrix) == 0) plane_loop(pacc, tab_off);
            }
            if (active && (EXP & kExpNoMatrix) == 0 && !kPlane) {
                // step s = GS g + j of the window: the A entries 2 s below the lane's first, B piece 2 j + h of
                // tile n + g -- constants off two per-lane addresses (NG > 0) or off two running ones
                constexpr int KS = NG * GS;
                // (NG > 0: the lane's LAST entry, and the compiler kept from folding the base back to the first
                // one: DS offsets are unsigned, negative ones cost an address add per load)
                int a_off = a_base - (STRAIGHT ? 128 * KS : 0) + tab_off;
                if constexpr (STRAIGHT) asm volatile("" : "+v"(a_off));
                const uint8_t *ap = tabp + a_off;
                const uint8_t *bp = slot + TS * n + 16 * h;
                int s_done = 0, g_done = 0;  // (compile-time values when the groups are unrolled)
                auto load_a = [&](v4i(&a)[2], int s) {
#pragma unroll
                    for (int f = 0; f < 2; f++) {
                        if constexpr (STRAIGHT) a[f] = *reinterpret_cast<const v4i *>(ap + f * (2 * (KS + 4) + (D / 8) * (kT - 1) + 1) * 64 + 128 * (KS - s));
                        else a[f] = *reinterpret_cast<const v4i *>(ap + f * f_stride - 128 * (s - s_done));
                    }
                };
                auto load_b = [&](v4i(&b)[NB], int g, int j) {
#pragma unroll
                    for (int q = 0; q < NB; q++) b[q] = *reinterpret_cast<const v4i *>(bp + TS * (g - g_done) + 32 * j + q * 32 * TS);
                };
                // operands two steps ahead of their MFMAs, in rings of three (straight-line code) or four
                constexpr int RG = STRAIGHT ? 3 : 4;
                v4i a[RG][2], b[RG][NB];
                load_a(a[0], 0);
                load_b(b[0], 0, 0);
                load_a(a[1], 1);
                load_b(b[1], 0, 1);
                // one step; SC: the step as a compile-time value (straight-line form), or -1.  What a step touches, by
                // name: the accumulators, the operand rings, the next pass's image (its sign flip), the two loaders
                auto step = [&acc, &a, &b, &x, &load_a, &load_b](auto sc, int g, int j, int jx = 0) {
                    constexpr int SC = decltype(sc)::value;
                    const int s = SC >= 0 ? SC : GS * g + j;
                    const int sx = SC >= 0 ? SC : jx;  // (ring positions: the step mod 3, or the step of the trip mod 4)
                    load_a(a[(sx + 2) % RG], s + 2);
                    if (j + 2 < GS) load_b(b[(sx + 2) % RG], g, j + 2);
                    else load_b(b[(sx + 2) % RG], g + 1, j + 2 - GS);
#pragma unroll
                    for (int f = 0; f < 2; f++)
#pragma unroll
                        for (int q = 0; q < NB; q++) {
                            if constexpr (STRAIGHT && SC == 0)
                                asm volatile("v_mfma_i32_32x32x32_i8 %0, %1, %2, 0" : "=&v"(acc[f][q]) : "v"(a[sx % RG][f]), "v"(b[sx % RG][q]));
                            else
                                acc[f][q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[sx % RG][f], b[sx % RG][q], acc[f][q], 0, 0, 0);
                        }
                    // (u8 sources, straight-line form: the NEXT pass's bytes -- in flight since the loop's first lines, here long
                    // since -- get their sign flip in the shadow of this wave's own MFMAs, where a vector instruction
                    // costs 2-3 cycles; left to the landing they are 40 instructions of the epilogue, which runs
                    // beside the SIMD partner's loop at one instruction per MFMA slot.  Registers without a load in
                    // flight hold stale values that nobody lands.)
                    if constexpr (STRAIGHT && FMT == HZSDR_FMT_U8 && SC >= 0) {
                        constexpr int kFlipFirst = KS - 2 - (KU + 1) / 2;  // two registers per step, done two steps before the end
                        if constexpr (SC == kFlipFirst) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
                        if constexpr (SC >= kFlipFirst && 2 * (SC - kFlipFirst) < KU) {
#pragma unroll
                            for (int u = 2 * (SC - kFlipFirst); u < KU && u < 2 * (SC - kFlipFirst) + 2; u++) {
                                x[u] ^= (int)0x80808080;
                                asm volatile("" : "+v"(x[u]));  // (here, not at the landing)
                            }
                        }
                    }
                    // the step's loads between its MFMAs, nothing moved across steps
#pragma unroll
                    for (int q = 0; q < 2 + NB; q++) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // LDS read
                    }
                    __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB - 2 - NB > 0 ? 2 * NB - 2 - NB : 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                };
                static_assert(GS == 4 || GS == 8, "ring indices repeat per group");
                if constexpr (STRAIGHT) {
                    auto all = [&](auto self, auto sc) {
                        constexpr int S = decltype(sc)::value;
                        if constexpr (S < KS) {
                            step(sc, S / GS, S % GS);
                            self(self, std::integral_constant<int, S + 1>{});
                        }
                    };
                    all(all, std::integral_constant<int, 0>{});
                } else {
                    // UG groups per trip: a back edge costs a drain of the operand pipeline (the compiler cannot count
                    // outstanding loads across it)
                    constexpr int UGv = UG > 0 ? UG : 1;
                    int g = 0;
#pragma unroll 1
                    for (; g + UGv <= groups; g += UGv) {
#pragma unroll
                        for (int gq = 0; gq < UGv; gq++)
#pragma unroll
                            for (int j = 0; j < GS; j++) step(std::integral_constant<int, -1>{}, g + gq, j, GS * gq + j);
                        ap -= 128 * GS * UGv;
                        bp += TS * UGv;
                        s_done += GS * UGv;
                        g_done += UGv;
                    }
                    if constexpr (UGv > 1) {
#pragma unroll 1
                        for (; g < groups; g++) {
#pragma unroll
                            for (int j = 0; j < GS; j++) step(std::integral_constant<int, -1>{}, g, j, j);
                            ap -= 128 * GS;
                            bp += TS;
                            s_done += GS;
                            g_done++;
                        }
                    }
                }
            }
            stamp(2);
            [[maybe_unused]] int cs_e1 = 0, cs_e2 = 0, cs_l1 = 0, cs_l2 = 0;
            [[maybe_unused]] auto csum = [&](int &s1, int &s2) {
#pragma unroll
                for (int f = 0; f < 2; f++)
#pragma unroll
                    for (int b = 0; b < NB; b++) asm volatile("" : "+v"(acc[f][b]));
                s1 = 0, s2 = 0;
#pragma unroll
                for (int f = 0; f < 2; f++)
#pragma unroll
                    for (int b = 0; b < NB; b++)
#pragma unroll
                        for (int q = 0; q < 16; q++) s1 += acc[f][b][q], s2 += (1 + q + 16 * (b + NB * f)) * acc[f][b][q];
                asm volatile("" : "+v"(s1), "+v"(s2));
            };
            if constexpr ((EXP & kExpChecksums) != 0) csum(cs_e1, cs_e2);
            if (in_next) land(x, active && (EXP & kExpNoMatrix) == 0);  // (the matrix loop ran: it flipped the bytes' signs)
            else if (has_next) land_edge(pass_of(nxt));
            vm_clear();
            stamp(3);
            if constexpr ((EXP & kExpChecksums) != 0) {
                // stamps[0]: 0 = store, 1 = compare; [1]: the stored checksums (int4 per pass and lane); [2]: records
                // written; [8 + 8 r ...]: record r
                csum(cs_l1, cs_l2);
                v4i *ref = reinterpret_cast<v4i *>((uintptr_t)stamps[1]);
                const size_t ci = (size_t)pass_of(cur) * 64 + l;
                if (active) {
                    if (stamps[0] == 0) {
                        ref[ci] = v4i{cs_e1, cs_e2, cs_l1, cs_l2};
                    } else {
                        const v4i r = ref[ci];
                        if (r[0] != cs_e1 || r[1] != cs_e2 || r[2] != cs_l1 || r[3] != cs_l2) {
                            const unsigned long long slot_r = atomicAdd(&stamps[2], 1ull);
                            if (slot_r < 4000) {
                                unsigned long long *rec = stamps + 8 + 8 * slot_r;
                                rec[0] = (unsigned long long)pass_of(cur) | ((unsigned long long)l << 32) | ((unsigned long long)wave << 40);
                                rec[1] = (unsigned long long)(unsigned)wb | ((unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(4 | (31 << 11)) << 32);
                                rec[2] = (unsigned long long)(unsigned)cs_e1 | ((unsigned long long)(unsigned)cs_e2 << 32);
                                rec[3] = (unsigned long long)(unsigned)cs_l1 | ((unsigned long long)(unsigned)cs_l2 << 32);
                                rec[4] = (unsigned long long)(unsigned)r[0] | ((unsigned long long)(unsigned)r[1] << 32);
                                rec[5] = (unsigned long long)(unsigned)r[2] | ((unsigned long long)(unsigned)r[3] << 32);
                                rec[6] = __builtin_amdgcn_s_memrealtime();
                                rec[7] = (unsigned long long)(unsigned)__builtin_amdgcn_s_getreg(20 | (31 << 11));
                            }
                        }
                    }
                }
            }
            if (active) {
                const double *dc = reinterpret_cast<const double *>(tabp + tab_off + (size_t)G.ne * 128);
                float2 y[NB][4];
                if constexpr (kReuse) planes_xchg(pacc, y, dc[0] * k3, dc[1] * k3);
                else if constexpr (kPlane) planes16(pacc, y, dc[0] * k3, dc[1] * k3);
                else planes(acc, y, dc[0] * k3, dc[1] * k3);
                if constexpr ((EXP & kExpStamps) != 0) {  // (the stamp behind the combination, not in the middle of it)
#pragma unroll
                    for (int b = 0; b < NB; b++)
#pragma unroll
                        for (int q = 0; q < 4; q++) asm volatile("" : "+v"(y[b][q].x), "+v"(y[b][q].y));
                }
                stamp(4);
                const uint32_t mb = m_start + (uint32_t)n * kT + 4 * h;
                {
                    // (the run's step factors: behind the constant term at the table's end, hz_firmm2_plan.h)
                    program(y, mb, phi_r, dphi, sel ? rv.seg : ru.seg, reinterpret_cast<const float4 *>(dc + 2));
                    stamp(5);
                    const uint64_t outp = vout_of(buf_of(pass_of(cur)));
#pragma unroll
                    for (int b = 0; b < NB; b++) store_block(outp, y[b], mb + (uint32_t)(32 * kT) * b, v_lo, v_hi);
                }
            }
            stamp(6);
            // No wave priorities in the library (kExpPriorities turns them on for study: the matrix pipe goes to the wave of
            // higher priority, then to the OLDER one, and ranking a wave on its first pass above one that has finished
            // a pass makes the two waves of a SIMD alternate pass by pass): the kernel is as fast without them
            // (tools/mfma_fir2.hip: 38.6 against 38.9 us).  Round 4, tasks off the head: launch by launch with an event
            // pair each the priorities are worth 0.4-1.8 us of the median -- and in bench.py's back-to-back
            // stream they COST 0.6 us per step (0.0392 against 0.0386, three times over on one box).  Still off.
            if constexpr ((EXP & kExpPriorities) != 0) __builtin_amdgcn_s_setprio(0);
            cur = nxt;
        }
        if (!b_here) break;
        ra = rb;
        slot_a ^= 1;
        a_done = true;
        if (!has_passes(ra + 1)) break;
    }
    history_tasks();
    // The fix-up tasks, BEHIND the passes: the old waves stage round 0's window while the young ones are still in
    // the workgroup's last pass (~5 us of slack), the sums follow the barrier that ends the passes.  (Rounds 2-4
    // did round 0 in front of the first pass -- "the matrix pipes idle there anyway" -- but the workgroup's first
    // barrier then waited for the window's loads and the young waves started their passes behind the sums: a call
    // with a clock boundary took 3-4 us longer than one without, four calls of 7.5.)
#pragma unroll 1
    // (Task t of a round goes to workgroup grid - 1 - t: the history tasks sit on the first sixteen workgroups' old
    // waves, and the few tasks of a call with one clock boundary should not queue up behind them.)
    for (int round = 0; (L.grid - 1 - wb) + round * L.grid < L.n_task; round++) {  // (uniform; round > 0: more tasks than workgroups)
        if (round > 0 || kStampShare) __syncthreads();
        tasks_front(round);
        __syncthreads();
        tasks_back();
    }
    stamp(7);
    if constexpr ((EXP & kExpStamps) != 0) {
        for (int i = l; i < 8 * kStampRows; i += 64) stamps[((size_t)wb * kWaves + wave) * (8 * kStampRows) + i] = lstamp[i];
        if (tid == 0) {  // (behind every wave's rows: shader cycles and 10 ns ticks of this workgroup's first wave)
            unsigned long long *ck = stamps + (size_t)L.grid * kWaves * (8 * kStampRows) + 2 * (size_t)wb;
            ck[0] = __builtin_amdgcn_s_memtime() - clk0;
            ck[1] = __builtin_amdgcn_s_memrealtime() - rt0;
        }
    }
}

// hz_firmm2.hip
int launch_fir(hipStream_t stream, int num_cus, int fmt, unsigned D, const void *in, float2 *out, const float2 *hist,
               float2 *new_hist, const uint8_t *rhist, uint8_t *new_rhist, const float2 *taps, size_t n, const Geom &g,
               const Plan &L, const EwProgram &P, const Fix &F, const Batch &B, int loop_form = 0);
// the history tasks alone, as a kernel of their own (n >= off): hz_firmm2.hip
int launch_history(hipStream_t stream, int fmt, const void *in, float2 *new_hist, uint8_t *new_rhist, size_t n, unsigned off, const EwProgram &P);

}  // namespace mm2
}  // namespace hz
