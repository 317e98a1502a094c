// mfma_plane_skip.hip -- the price of the FIR pass's matrix loop in two cuts, at the power cap, before the library
// changes: every SIMD of every CU runs two waves that multiply "passes" back to back, operands from LDS as the
// kernel (csrc/hz_firmm2.h) reads them, random bytes everywhere except where a digit plane of the taps is zero.
//
//   PAIR: today's loop -- 68 steps of 32 bytes, per step two A fragments (rows = 8 outputs x (re, im) x TWO digit
//         planes: fragment 0 holds planes 0 and 1, fragment 1 planes 2 and 3) x two B fragments (32 tiles each),
//         four v_mfma_i32_32x32x32_i8.  Where plane 0 is zero, half of fragment 0's rows are zero (the MFMA runs).
//   PLANE: one plane per fragment -- 34 step pairs of 64 bytes, per pair four A fragments (rows = 8 outputs x
//          (re, im), one plane each) x four B fragments (16 tiles each), v_mfma_i32_16x16x64_i8.  Outside the
//          plane-0 window [LO, HI) plane 0 is SKIPPED (12 MFMAs and 7 reads instead of 16 and 8), or issued with a
//          zero A (ZERO), or issued with random bytes like the others (the loop without any zero plane).
//
// The PLANE rows read their operands at lds + 16 lane -- contiguous, no bank conflict -- unless they say otherwise: the
// rows "kernel's lanes" read with the addresses of the kernel's lanes (r16 = lane & 15, kq = lane >> 4: A row r16 of
// entry i - kq - 4 t + e0, B piece kq of tile r16), plane 0's A on every pair as the kernel does, in the layout the
// kernel had first (the table in its memory order T[f][E][part][pl], tiles 144 bytes apart: every read 2-way
// conflicted), in the one it had next (plane-major table, tiles 160 bytes apart: hz_firmm2_plan.h), and as the loop that
// re-uses its tile windows reads them (column r16 of block j = tile 4 r16 + j, rows by reuse_row_offset, ONE B read per
// pair from pair 2 on into the register of the fragment that died two pairs earlier: 176 reads a pass instead of 272).
//
// Reads run AH pairs (PLANE) or 2 steps (PAIR) ahead of their MFMAs, rings of AH + 1, placed one read behind each
// MFMA (sched_group_barrier) as the kernel places them.  Reports per form: ns per pass per SIMD (two waves, each
// pass once), the shader clock the waves saw (s_memtime cycles per 10 ns of s_memrealtime), cycles per MFMA, and
// dense-equivalent Pop/s (the PAIR form's 272 x 32x32x32 per pass counted for every form: the useful work).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "hz_firmm2_plan.h"

#include <algorithm>
#include <utility>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// LDS: R = 24 KB of random bytes (A fragments), Z = 1 KB of zeros, H = 1 KB with the even lanes' 16 bytes zero
// (PAIR's fragment 0 where plane 0 is zero: lane n & 1 is the plane of its row), then a slot of B per wave (the
// contiguous rows use 6 KB of it)
constexpr int kR = 0, kZ = 24576, kH = kZ + 1024, kB = kH + 1024, kBW = 13056, kLds = kB + 8 * kBW;
constexpr int kPairs = 34, kSteps = 68;
// the kernel's geometry at 1024 taps (hz_firmm2_plan.h: make_geom)
constexpr int kNe = 152, kE0 = 144;
enum { LAY_FLAT = 0, LAY_FIRST = 1, LAY_NOW = 2, LAY_REUSE = 3 };
static_assert(hz::mm2::plane_a_offset(kNe, kE0, 3, 0, 15, 0) + 16 <= kZ && 64 * (7 + kE0) + 32 + 64 * kNe + 32 <= kZ, "A addresses inside the random area");
static_assert(hz::mm2::plane_b_offset(160, 3, kPairs - 1, 15, 3) + 16 <= kBW, "B addresses inside the wave's slot");
static_assert(hz::mm2::reuse_b_offset(3, kPairs - 1, 15, 3) + 16 <= kBW, "... the re-using loop's too");

enum { FILL_SKIP = 0, FILL_ZERO = 1, FILL_RANDOM = 2 };

template <int I> using ic = std::integral_constant<int, I>;
template <class F, int... I> __device__ __forceinline__ void unroll_seq(F &f, std::integer_sequence<int, I...>) { (f(ic<I>{}), ...); }
template <int N, class F> __device__ __forceinline__ void unroll(F &&f) { unroll_seq(f, std::make_integer_sequence<int, N>{}); }

__device__ void fill_lds(uint8_t *lds, unsigned seed) {
    unsigned h = (seed * 512u + threadIdx.x) * 2654435761u + 12345u;  // (per thread: every lane sees other bytes)
    for (int i = threadIdx.x; i < kLds / 4; i += blockDim.x) {
        h ^= h << 13, h ^= h >> 17, h ^= h << 5;
        const int byte = 4 * i;
        unsigned v = h;
        if (byte >= kZ && byte < kH) v = 0;
        if (byte >= kH && byte < kB && (((byte - kH) >> 4) & 1) == 0) v = 0;
        reinterpret_cast<unsigned *>(lds)[i] = v;
    }
    __syncthreads();
}

__device__ __forceinline__ void finish(unsigned long long *out, int *sink, int s, unsigned long long t0, unsigned long long r0) {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (s == 0x12345678) *sink = s;
    const unsigned tid = threadIdx.x + blockIdx.x * blockDim.x;
    if ((threadIdx.x & 63) == 0) {
        out[2 * (tid >> 6)] = t1 - t0;
        out[2 * (tid >> 6) + 1] = r1 - r0;
    }
}

// today's loop: step s reads A (s, f) and B (s, q); plane 0 zero outside steps [2 LO, 2 HI) unless FILL_RANDOM
template <int LO, int HI, int FILL>
__global__ __launch_bounds__(512) void pair_pass(unsigned long long *out, int trips, int *sink) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    fill_lds(lds, blockIdx.x);
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *ab = lds + 16 * l, *bb = lds + kB + kBW * wave + 16 * l;
    auto a_addr = [&](int s, int f) -> const v4i * {
        if (f == 0 && FILL != FILL_RANDOM && (s < 2 * LO || s >= 2 * HI)) return reinterpret_cast<const v4i *>(ab + kH);
        return reinterpret_cast<const v4i *>(ab + kR + ((2 * s + f) % 24) * 1024);
    };
    auto b_addr = [&](int s, int q) { return reinterpret_cast<const v4i *>(bb + ((2 * s + q) % 6) * 1024); };
    v16i c[2][2];
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    for (int t = 0; t < trips; t++) {
        for (int f = 0; f < 2; f++)
            for (int q = 0; q < 2; q++) c[f][q] = v16i{};
        v4i a[3][2], b[3][2];
        for (int s = 0; s < 2; s++)
            for (int f = 0; f < 2; f++) a[s][f] = *a_addr(s, f), b[s][f] = *b_addr(s, f);
        unroll<kSteps>([&](auto sc) {
            constexpr int s = decltype(sc)::value;
            if constexpr (s + 2 < kSteps) {
#pragma unroll
                for (int f = 0; f < 2; f++) a[(s + 2) % 3][f] = *a_addr(s + 2, f), b[(s + 2) % 3][f] = *b_addr(s + 2, f);
            }
#pragma unroll
            for (int f = 0; f < 2; f++)
#pragma unroll
                for (int q = 0; q < 2; q++) c[f][q] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s % 3][f], b[s % 3][q], c[f][q], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
        asm volatile("" : "+v"(c[0][0]), "+v"(c[0][1]), "+v"(c[1][0]), "+v"(c[1][1]));
    }
    int s = 0;
    for (int f = 0; f < 2; f++)
        for (int q = 0; q < 2; q++)
            for (int i = 0; i < 16; i++) s += c[f][q][i];
    finish(out, sink, s, t0, r0);
}

// one plane per fragment: pair t reads A (t, p) for its planes and B (t, j); plane 0 outside [LO, HI) as FILL says
template <int LO, int HI, int FILL, int AH, int LAY = LAY_FLAT>
__global__ __launch_bounds__(512) void plane_pass(unsigned long long *out, int trips, int *sink) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    fill_lds(lds, blockIdx.x);
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *ab = lds + 16 * l, *bb = lds + kB + kBW * wave + 16 * l;
    // (the kernel's lanes: per-lane bases, the pair and the plane / block at constant offsets)
    const int r16 = l & 15, kq = l >> 4;
    constexpr bool kTabNow = LAY == LAY_NOW || LAY == LAY_REUSE;  // (the plane-major table)
    static_assert(LAY != LAY_REUSE || AH == 1, "the rotation is written for reads one pair ahead");
    int a_lane = kTabNow ? hz::mm2::plane_a_offset(kNe, kE0, 0, kPairs - 1, r16, kq) : 64 * ((r16 >> 1) - kq - 4 * (kPairs - 1) + kE0) + 32 * (r16 & 1);
    asm volatile("" : "+v"(a_lane));  // (the last pair's entry as the base: unsigned offsets, as the kernel)
    const uint8_t *al = lds + kR + a_lane;
    const uint8_t *bl = lds + kB + kBW * wave + (LAY == LAY_REUSE ? hz::mm2::reuse_row_offset(4 * r16) : (LAY == LAY_NOW ? 160 : 144) * r16) + 16 * kq;
    auto a_addr = [&](int t, int p) -> const v4i * {
        if constexpr (kTabNow) return reinterpret_cast<const v4i *>(al + 32 * kNe * p + 128 * (kPairs - 1 - t));
        if constexpr (LAY == LAY_FIRST) return reinterpret_cast<const v4i *>(al + (p >> 1) * 64 * kNe + 16 * (p & 1) + 256 * (kPairs - 1 - t));
        if (p == 0 && FILL == FILL_ZERO && (t < LO || t >= HI)) return reinterpret_cast<const v4i *>(ab + kZ);
        return reinterpret_cast<const v4i *>(ab + kR + ((4 * t + p) % 24) * 1024);
    };
    auto b_addr = [&](int t, int j) {
        if constexpr (LAY == LAY_REUSE) return reinterpret_cast<const v4i *>(bl + hz::mm2::reuse_row_offset(j + t / 2) + 64 * (t & 1));
        if constexpr (LAY != LAY_FLAT) return reinterpret_cast<const v4i *>(bl + (LAY == LAY_NOW ? 160 : 144) * (16 * j + t / 2) + 64 * (t & 1));
        return reinterpret_cast<const v4i *>(bb + ((4 * t + j) % 6) * 1024);
    };
    static_assert(LAY == LAY_FLAT || FILL != FILL_ZERO, "the kernel's lanes read the table itself");
    auto has0 = [](int t) { return LAY != LAY_FLAT || FILL != FILL_SKIP || (t >= LO && t < HI); };  // (plane 0's A: the kernel reads it on every pair)
    constexpr int RG = AH + 1;
    v4i c[4][4];
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
#pragma unroll 1
    for (int tr = 0; tr < trips; tr++) {
        for (int p = 0; p < 4; p++)
            for (int j = 0; j < 4; j++) c[p][j] = v4i{};
        v4i a[RG][4], b[RG][4];
        auto load = [&](int t, int r) {
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (p > 0 || has0(t)) a[r][p] = *a_addr(t, p);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if constexpr (LAY != LAY_REUSE) b[r][j] = *b_addr(t, j);
                else if (hz::mm2::reuse_b_read(j, t)) b[r][hz::mm2::reuse_b_reg(j, t)] = *b_addr(t, j);
            }
        };
        for (int t = 0; t < AH; t++) load(t, t);
        unroll<kPairs>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            if constexpr (t + AH < kPairs) load(t + AH, (t + AH) % RG);
            constexpr bool h0 = FILL != FILL_SKIP || (t >= LO && t < HI);
#pragma unroll
            for (int p = h0 ? 0 : 1; p < 4; p++)
#pragma unroll
                for (int j = 0; j < 4; j++) c[p][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[t % RG][p], b[t % RG][LAY == LAY_REUSE ? hz::mm2::reuse_b_reg(j, t) : j], c[p][j], 0, 0, 0);
            constexpr int nm = h0 ? 16 : 12;
            constexpr int nr = t + AH >= kPairs ? 0 : LAY == LAY_REUSE && t + AH >= 2 ? 5 : (LAY != LAY_FLAT || FILL != FILL_SKIP || (t + AH >= LO && t + AH < HI) ? 8 : 7);
#pragma unroll
            for (int i = 0; i < nm; i++) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (i < nr) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
#pragma unroll
        for (int p = 0; p < 4; p++) asm volatile("" : "+v"(c[p][0]), "+v"(c[p][1]), "+v"(c[p][2]), "+v"(c[p][3]));
    }
    int s = 0;
    for (int p = 0; p < 4; p++)
        for (int j = 0; j < 4; j++) s += c[p][j][0] + c[p][j][1] + c[p][j][2] + c[p][j][3];
    finish(out, sink, s, t0, r0);
}

template <class K> static void run(const char *name, K kern, int mfmas, int mfma_cycles, unsigned long long *dout, int *sink, double target_us) {
    const int grid = 256, waves = grid * 8;
    const int trips = (int)(target_us * 1700.0 / (2.0 * 8704.0)) + 1;  // ~1.7 GHz, two waves per SIMD
    CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float ms = 0;
    for (int rep = 0; rep < 3; rep++) {
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kLds, 0, dout, trips, sink);
        CK(hipGetLastError());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
    }
    std::vector<unsigned long long> h(2 * waves);
    CK(hipMemcpy(h.data(), dout, h.size() * 8, hipMemcpyDeviceToHost));
    std::vector<double> ghz, cyc;
    for (int w = 0; w < waves; w++) ghz.push_back((double)h[2 * w] / (double)h[2 * w + 1] / 10.0), cyc.push_back((double)h[2 * w]);
    std::sort(ghz.begin(), ghz.end());
    std::sort(cyc.begin(), cyc.end());
    const double passes_per_simd = 2.0 * trips;
    const double ns_pass = ms * 1e6 / passes_per_simd;
    // cycles per MFMA: a wave's own cycles over its MFMAs, halved (two waves share the pipe)
    const double cyc_mfma = cyc[waves / 2] / ((double)trips * mfmas) / 2.0;
    printf("  %-58s %7.1f us  clock %.3f GHz (min %.3f max %.3f)  %6.1f ns per pass per SIMD  %4d MFMAs = %5d pipe cycles per pass, %5.1f cycles per MFMA (nominal %2d)  duty %.2f  useful %.2f Pop/s\n",
           name, ms * 1e3, ghz[waves / 2], ghz[0], ghz.back(), ns_pass, mfmas, mfmas * mfma_cycles, cyc_mfma, mfma_cycles,
           (double)mfmas * mfma_cycles / (ns_pass * ghz[waves / 2]), 1024.0 * 272.0 * 65536.0 / ns_pass * 1e-6);
}

int main(int argc, char **argv) {
    const double us = argc > 1 ? atof(argv[1]) : 2000.0;
    unsigned long long *dout;
    int *sink;
    CK(hipMalloc(&dout, 2 * 2048 * 8));
    CK(hipMalloc(&sink, 4));
    // the plane-0 window: 16 of 34 step pairs (18 skipped = 72 of 544 16x16x64 = 0.13 of the matrix work)
    constexpr int LO = 9, HI = 25;
    constexpr int kSkip = 34 * 16 - 18 * 4;
    printf("FIR pass matrix loops on every SIMD of 256 CUs, two waves per SIMD, random bytes, ~%.0f us launches\n", us);
    printf("plane-0 window: step pairs [%d, %d) of %d (skip fraction %.3f of the matrix work)\n", LO, HI, kPairs, 18.0 * 4 / 544.0);
    for (int rep = 0; rep < 2; rep++) {
        run("PAIR 32x32x32, all random", pair_pass<LO, HI, FILL_RANDOM>, 272, 32, dout, sink, us);
        run("PAIR 32x32x32, plane 0 zero outside (today's kernel)", pair_pass<LO, HI, FILL_ZERO>, 272, 32, dout, sink, us);
        run("PLANE 16x16x64, all random, skip 0 (reads 2 ahead)", plane_pass<LO, HI, FILL_RANDOM, 2>, 544, 16, dout, sink, us);
        run("PLANE 16x16x64, plane 0 zero A outside (2 ahead)", plane_pass<LO, HI, FILL_ZERO, 2>, 544, 16, dout, sink, us);
        run("PLANE 16x16x64, plane 0 skipped outside, 0.13 (2 ahead)", plane_pass<LO, HI, FILL_SKIP, 2>, kSkip, 16, dout, sink, us);
        run("PLANE 16x16x64, all random, skip 0 (reads 1 ahead)", plane_pass<LO, HI, FILL_RANDOM, 1>, 544, 16, dout, sink, us);
        run("PLANE 16x16x64, plane 0 skipped outside, 0.13 (1 ahead)", plane_pass<LO, HI, FILL_SKIP, 1>, kSkip, 16, dout, sink, us);
        run("... kernel's lanes, table as in memory, tiles 144 B apart", plane_pass<LO, HI, FILL_SKIP, 1, LAY_FIRST>, kSkip, 16, dout, sink, us);
        run("... kernel's lanes, plane-major table, tiles 160 B apart", plane_pass<LO, HI, FILL_SKIP, 1, LAY_NOW>, kSkip, 16, dout, sink, us);
        run("PLANE all random, skip 0 (1 ahead), kernel's lanes, 144 B", plane_pass<LO, HI, FILL_RANDOM, 1, LAY_FIRST>, 544, 16, dout, sink, us);
        run("PLANE all random, skip 0 (1 ahead), kernel's lanes, 160 B", plane_pass<LO, HI, FILL_RANDOM, 1, LAY_NOW>, 544, 16, dout, sink, us);
        run("... kernel's lanes, windows re-used: 1 B read per pair", plane_pass<LO, HI, FILL_SKIP, 1, LAY_REUSE>, kSkip, 16, dout, sink, us);
        run("PLANE all random, skip 0 (1 ahead), windows re-used", plane_pass<LO, HI, FILL_RANDOM, 1, LAY_REUSE>, 544, 16, dout, sink, us);
    }
    return 0;
}
