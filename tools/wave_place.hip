// wave_place.hip -- where the waves of a launch of ONE-WAVE workgroups land: the row-wave banks (csrc/hz_rowwave.h) launch
// up to 1024 workgroups of 64 lanes and count on one wave per SIMD (256 CUs x 4).  Every wave reads its hardware id
// (XCC, SE, SH, CU, SIMD) once, then spins on a dependent chain long enough for the whole launch to be resident
// together, and lane 0 stores the id.  Prints, per launch, the waves per SIMD id over the chip, the number of distinct
// (XCC, SE, SH, CU) and (..., SIMD) places used, and the most waves that share a CU and a SIMD.
//
//     tools/bin/wave_place            256, 512 and 1024 workgroups, each with 2 KiB and with 40 KiB of LDS
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define HIP_OK(call)                                                                  \
    do {                                                                              \
        hipError_t e__ = (call);                                                      \
        if (e__ != hipSuccess) {                                                      \
            printf("%s: %s (line %d)\n", #call, hipGetErrorString(e__), __LINE__);     \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

// s_getreg_b32's immediate: register id, first bit, bits - 1
#define GETREG(id, first, bits) ((id) | ((first) << 6) | (((bits)-1) << 11))
constexpr int kHwId = 4, kXccId = 20;

__global__ __launch_bounds__(64) void place_kernel(uint32_t *ids, uint32_t *xcc, float *sink, int spin) {
    extern __shared__ float lds[];
    const uint32_t id = __builtin_amdgcn_s_getreg(GETREG(kHwId, 0, 32));
    const uint32_t xc = __builtin_amdgcn_s_getreg(GETREG(kXccId, 0, 4));
    float v = (float)threadIdx.x;
    for (int i = 0; i < spin; i++) v = fmaf(v, 0.99999f, 1e-3f);  // (a dependent chain: one wave, one lane's rate)
    lds[threadIdx.x] = v;
    if (threadIdx.x == 0) {
        ids[blockIdx.x] = id;
        xcc[blockIdx.x] = xc;
        if (lds[0] == -1.0f) sink[0] = v;  // (keeps the chain)
    }
}

int main() {
    const int spin = 400000;
    uint32_t *ids, *xcc;
    float *sink;
    HIP_OK(hipMalloc((void **)&ids, 1024 * 4));
    HIP_OK(hipMalloc((void **)&xcc, 1024 * 4));
    HIP_OK(hipMalloc((void **)&sink, 4));
    for (size_t lds : {(size_t)2048, (size_t)40 * 1024})
        for (int waves : {256, 512, 1024}) {
            for (int rep = 0; rep < 2; rep++) {  // (the first launch loads the code)
                hipLaunchKernelGGL(place_kernel, dim3(waves), dim3(64), lds, 0, ids, xcc, sink, spin);
                HIP_OK(hipGetLastError());
                HIP_OK(hipDeviceSynchronize());
            }
            std::vector<uint32_t> h(waves), x(waves);
            HIP_OK(hipMemcpy(h.data(), ids, waves * 4, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(x.data(), xcc, waves * 4, hipMemcpyDeviceToHost));
            int per_simd[4] = {0, 0, 0, 0};
            std::map<uint32_t, int> cu, slot;
            for (int w = 0; w < waves; w++) {
                // HW_ID: wave [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]
                const uint32_t simd = h[w] >> 4 & 3u, where = (x[w] << 16) | (h[w] >> 8 & 0xffu);
                per_simd[simd]++;
                cu[where]++;
                slot[where << 2 | simd]++;
            }
            int most_cu = 0, most_slot = 0;
            for (auto &kv : cu) most_cu = kv.second > most_cu ? kv.second : most_cu;
            for (auto &kv : slot) most_slot = kv.second > most_slot ? kv.second : most_slot;
            printf("lds %6zu B, %4d workgroups of one wave: waves per SIMD id %d %d %d %d; %zu CUs and %zu SIMDs in use; at most %d waves on a CU, %d on a SIMD\n",
                   lds, waves, per_simd[0], per_simd[1], per_simd[2], per_simd[3], cu.size(), slot.size(), most_cu, most_slot);
        }
    return 0;
}
