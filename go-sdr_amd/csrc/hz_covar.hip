// hz_covar.hip -- the covariance bank and the beam scan (include/hzsdr_covar.h).
//
// The bank.  The N channels' real and imaginary parts are 2N <= 32 real rows V; per segment of 256 snapshots
// G = V V^T is 64 steps of v_mfma_f32_16x16x4_f32 per accumulator tile: one tile for N <= 8, the tiles (0,0), (0,1)
// and (1,1) for N <= 16.  A and B of the diagonal tiles are the same register.  Two kernels:
//   * covar_segment_kernel: one wave per item (hz_covar_plan.h: a segment, or an aligned group of 8).  Half a segment
//     at a time is loaded coalesced (consecutive lanes, consecutive snapshots of one row), converted in the loads and
//     stored as float rows in LDS, snapshots behind the block's or the flush's end as +0; lane l then reads
//     V[l & 15][4 t + (l >> 4)], so that k-slot j of step t is snapshot 4 t + j.  A group's eight segment sums go
//     through the balanced tree in registers.  The wave writes one node in accumulator order.
//   * covar_walk_kernel: one workgroup per block of the push; lane e owns entry e of a tile and walks the block's
//     nodes through the binary counter (LDS, one column per lane), then collapses it, combines and writes R -- or
//     stores the counter into the bank's stack for the next push.  The stack is two buffers, read one, write the other:
//     the block that resumes and the block left open are two workgroups of one launch and may use the same levels.
// No atomics; every sum has one owner.  The steps, the node and the combine are hz_covar_math.h (shared with
// tests/host/covar_ref.cpp), counts, regions, items and both index maps hz_covar_plan.h.
//
// The scan: one lane per (matrix, weight vector), the matrix in LDS, the terms of hz_covar_math.h.
// make NO_PK_F32=1 (csrc/Makefile): no packed float32 instruction in this unit's device code, as in hz_tuner.hip
#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "hz_chain_host.h"
#include "../../include/hzsdr_covar.h"
#include "hz_covar_math.h"
#include "hz_covar_plan.h"

struct hzsdr_covar {
    hzsdr_ctx *ctx;
    int fmt;
    uint32_t N, B;
    float2 *tail[2] = {nullptr, nullptr};  // the open segment's snapshots, converted, 256 per row: read one, write the other
    int tcur = 0;
    float *stack[2] = {nullptr, nullptr};  // the counter's levels, kLevels nodes: read one, write the other
    int scur = 0;
    float *nodes = nullptr;                // the node scratch of a launch round, grow-only
    size_t nodes_cap = 0;                  // in nodes
    hz::vp::State st{};
};

struct hzsdr_scan {
    hzsdr_ctx *ctx;
    uint32_t N, G;
    float2 *w = nullptr;  // G rows of N
};

namespace hz {

struct CvRows {
    const void *p[vp::kMaxChannels];
};

struct CvArgs {
    CvRows rows;        // row i of the push
    const float2 *tail; // the snapshots held: row i at 256 i
    float2 *tail_out;
    float *nodes;
    const float *stack;  // the open block's group sums as the last push left them
    float *stack_out;
    float2 *out;
    size_t out_stride;
    vp::Work w;
    uint32_t N, B;
};

typedef float cv_f4 __attribute__((ext_vector_type(4)));

// snapshot v of held ++ in, row i
template <int FMT>
__device__ __forceinline__ float2 cv_sample(const CvArgs &a, uint32_t i, uint64_t v) {
    using RT = typename Raw<FMT>::t;
    return v < a.w.held_in ? a.tail[i * vp::kSeg + v] : Raw<FMT>::cvt(((const RT *)a.rows.p[i])[v - a.w.held_in]);
}

// NP: channels the load loop is unrolled for (8: one tile, 16: three)
template <int FMT, int NP>
__global__ __launch_bounds__(vp::kSegThreads) void covar_segment_kernel(CvArgs a) {
    constexpr uint32_t NT = NP == 8 ? 1 : 3;
    extern __shared__ __align__(16) float cv_lds[];
    const uint32_t lane = threadIdx.x;
    // the region, the block and the item of this wave
    uint64_t idx = blockIdx.x;
    uint32_t ri = 0;
    while (ri + 1 < a.w.regions && idx >= a.w.r[ri].blocks * a.w.r[ri].items) idx -= a.w.r[ri].blocks * a.w.r[ri].items, ri++;
    const vp::Region &r = a.w.r[ri];
    const uint64_t blk = idx / r.items;
    const uint32_t it = (uint32_t)(idx - blk * r.items);
    const vp::Item item = vp::covar_item(r, it);

    // the rows behind 2N are +0 and stay so
    for (uint32_t row = 2 * a.N; row < 2 * NP; row++)
        for (uint32_t n = lane; n < vp::kChunk; n += 64) cv_lds[vp::covar_lds_index(row, n)] = 0.0f;

    [[maybe_unused]] cv_f4 st0[NT], st1[NT], st2[NT];
    cv_f4 acc[NT];
    [[maybe_unused]] const uint32_t rowl = lane & 15u, kk = lane >> 4;
    for (uint32_t s = 0; s < item.count; s++) {
        const uint32_t seg = item.seg + s, len = vp::covar_seg_len(r, seg);
        const uint64_t v0 = vp::covar_seg_start(r, blk, seg, a.B);
#pragma unroll
        for (uint32_t t = 0; t < NT; t++) acc[t] = cv_f4{0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t h = 0; h < vp::kSeg / vp::kChunk; h++) {
            const uint32_t c0 = h * vp::kChunk, clen = len > c0 ? len - c0 : 0;
            if (s || h) __syncthreads();  // (the last chunk is read no more)
            float2 x[NP][vp::kChunk / 64];
            if (clen && v0 + c0 >= a.w.held_in) {
                // the whole chunk lies in the push: every load is issued before the first is waited for (a lane behind the
                // chunk's end loads the chunk's first snapshot and drops it)
                using RT = typename Raw<FMT>::t;
                const uint64_t off = v0 + c0 - a.w.held_in;
                RT raw[NP][vp::kChunk / 64];
#pragma unroll
                for (uint32_t i = 0; i < NP; i++)
#pragma unroll
                    for (uint32_t m = 0; m < vp::kChunk / 64; m++) {
                        const uint32_t n = lane + 64 * m;
                        raw[i][m] = RT();
                        if (i < a.N) raw[i][m] = ((const RT *)a.rows.p[i])[off + (n < clen ? n : 0u)];
                    }
#pragma unroll
                for (uint32_t i = 0; i < NP; i++)
#pragma unroll
                    for (uint32_t m = 0; m < vp::kChunk / 64; m++) {
                        const float2 c = Raw<FMT>::cvt(raw[i][m]);
                        x[i][m] = lane + 64 * m < clen ? c : make_float2(0.0f, 0.0f);
                    }
            } else {
                // the chunk starts in the snapshots held from the last push (the first segment of a push), or is empty
#pragma unroll
                for (uint32_t i = 0; i < NP; i++)
#pragma unroll
                    for (uint32_t m = 0; m < vp::kChunk / 64; m++) {
                        const uint32_t n = lane + 64 * m;
                        x[i][m] = (i < a.N && n < clen) ? cv_sample<FMT>(a, i, v0 + c0 + n) : make_float2(0.0f, 0.0f);
                    }
            }
#pragma unroll
            for (uint32_t i = 0; i < NP; i++)
#pragma unroll
                for (uint32_t m = 0; m < vp::kChunk / 64; m++) {
                    if (i >= a.N) continue;
                    const uint32_t n = lane + 64 * m;
                    cv_lds[vp::covar_lds_index(2 * i, n)] = x[i][m].x;
                    cv_lds[vp::covar_lds_index(2 * i + 1, n)] = x[i][m].y;
                }
            __syncthreads();
#if defined(__HIP_DEVICE_COMPILE__)
            const float *lo = cv_lds + vp::covar_lds_index(rowl, kk);
#pragma unroll 8
            for (uint32_t t = 0; t < vp::kChunk / 4; t++) {
                // v[h]: this lane's element of rows 16 h .. 16 h + 15, the A and the B operand alike
                float v[NT == 1 ? 1 : 2];
                v[0] = lo[4 * t];
                if constexpr (NT > 1) v[1] = lo[vp::covar_lds_index(16, 0) + 4 * t];
#pragma unroll
                for (uint32_t tile = 0; tile < NT; tile++)
                    acc[tile] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[vp::covar_tile_a(tile) / 16], v[vp::covar_tile_b(tile) / 16], acc[tile], 0, 0, 0);
            }
#endif
        }
        // the balanced tree over the group's segments: a counter of three levels in registers
        if (item.count > 1) {
#pragma unroll
            for (uint32_t t = 0; t < NT; t++) {
                cv_f4 v = acc[t];
                if (s & 1u) {
                    v = st0[t] + v;
                    if (s & 2u) {
                        v = st1[t] + v;
                        if (s & 4u)
                            v = st2[t] + v;
                        else
                            st2[t] = v;
                    } else
                        st1[t] = v;
                } else
                    st0[t] = v;
                acc[t] = v;
            }
        }
    }
    float *node = a.nodes + (size_t)(r.node0 + blk * r.items + it) * (NT * vp::kTile);
#pragma unroll
    for (uint32_t t = 0; t < NT; t++) *(cv_f4 *)(node + t * vp::kTile + lane * 4) = acc[t];
}

struct CvAdd {
    __device__ __forceinline__ float operator()(float l, float r) const { return cv::covar_node(l, r); }
};

// a lane's column of the counter in LDS: level l
struct CvColumn {
    float *p;
    __device__ __forceinline__ float &operator[](uint32_t l) const { return p[l * vp::kWalkThreads]; }
};

__global__ __launch_bounds__(vp::kWalkThreads) void covar_walk_kernel(CvArgs a) {
    __shared__ float stack[vp::kLevels][vp::kWalkThreads];
    __shared__ float G[3 * vp::kTile];
    const uint32_t tid = threadIdx.x, NF = vp::covar_node_floats(a.N), tiles = NF / vp::kTile;
    uint64_t blk = blockIdx.x;
    uint32_t ri = 0;
    while (ri + 1 < a.w.regions && blk >= a.w.r[ri].blocks) blk -= a.w.r[ri].blocks, ri++;
    const vp::Region &r = a.w.r[ri];
    const float *nodes = a.nodes + (size_t)(r.node0 + blk * r.items) * NF;
    const CvColumn col{&stack[0][tid]};
    for (uint32_t tile = 0; tile < tiles; tile++) {
        const uint32_t e = tile * vp::kTile + tid;
        // (a.stack is read, a.stack_out written: the block that resumes and the block left open are two workgroups of this
        // launch)
        uint32_t count = r.seg0;
        if (r.resume)
            for (uint32_t l = 0; l < vp::kLevels; l++)
                if ((count >> l) & 1u) col[l] = a.stack[(size_t)l * NF + e];
        uint32_t it = 0;
        for (; it < r.head; it++) vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], 0u, CvAdd{});
        for (uint32_t g = 0; g < r.groups;) {
            if (vp::covar_walk_many(count, vp::kGroupLog, r.groups - g)) {
                float v[vp::kWalk];
#pragma unroll
                for (uint32_t k = 0; k < vp::kWalk; k++) v[k] = nodes[(size_t)(it + k) * NF + e];
#pragma unroll
                for (uint32_t w = 1; w < vp::kWalk; w *= 2)
#pragma unroll
                    for (uint32_t k = 0; k < vp::kWalk; k += 2 * w) v[k] = cv::covar_node(v[k], v[k + w]);
                vp::covar_counter_push(col, count, v[0], vp::kGroupLog + vp::kWalkLog, CvAdd{});
                g += vp::kWalk, it += vp::kWalk;
            } else {
                vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], vp::kGroupLog, CvAdd{});
                g++, it++;
            }
        }
        for (uint32_t k = 0; k < r.tail; k++, it++) vp::covar_counter_push(col, count, nodes[(size_t)it * NF + e], 0u, CvAdd{});
        if (r.complete) {
            G[e] = vp::covar_counter_collapse(col, count, CvAdd{});
        } else {
            for (uint32_t l = 0; l < vp::kLevels; l++)
                if ((count >> l) & 1u) a.stack_out[(size_t)l * NF + e] = col[l];
        }
    }
    if (!r.complete) return;
    __syncthreads();
    if (tid < a.N * a.N) {
        const uint32_t i = tid / a.N, j = tid - i * a.N;
        const cv::c32 v = cv::covar_combine(G[vp::covar_node_index(2 * i, 2 * j)], G[vp::covar_node_index(2 * i + 1, 2 * j + 1)],
                                            G[vp::covar_node_index(2 * i + 1, 2 * j)], G[vp::covar_node_index(2 * i, 2 * j + 1)]);
        a.out[(size_t)(r.out0 + blk) * a.out_stride + tid] = make_float2(v.re, v.im);
    }
}

// the open segment's snapshots for the next push: held ++ in [V - held_out, V), every row
template <int FMT>
__global__ __launch_bounds__(vp::kSeg) void covar_tail_kernel(CvArgs a) {
    const uint32_t i = blockIdx.x, n = threadIdx.x;
    if (n < a.w.held_out) a.tail_out[i * vp::kSeg + n] = cv_sample<FMT>(a, i, a.w.V - a.w.held_out + n);
}

template <int FMT>
static int cv_launch_fmt(hzsdr_covar *c, const CvArgs &a) {
    hipStream_t s = c->ctx->stream;
    if (a.w.items) {
        const dim3 grid((unsigned)a.w.items), block(vp::kSegThreads);
        if (c->N <= 8)
            hipLaunchKernelGGL((covar_segment_kernel<FMT, 8>), grid, block, vp::covar_lds_bytes(c->N), s, a);
        else
            hipLaunchKernelGGL((covar_segment_kernel<FMT, 16>), grid, block, vp::covar_lds_bytes(c->N), s, a);
        HZ_HIP(c->ctx, hipGetLastError());
    }
    if (a.w.blocks) {
        hipLaunchKernelGGL(covar_walk_kernel, dim3((unsigned)a.w.blocks), dim3(vp::kWalkThreads), 0, s, a);
        HZ_HIP(c->ctx, hipGetLastError());
    }
    if (a.w.held_out) {
        hipLaunchKernelGGL(covar_tail_kernel<FMT>, dim3(c->N), dim3(vp::kSeg), 0, s, a);
        HZ_HIP(c->ctx, hipGetLastError());
    }
    return HZSDR_OK;
}

static int cv_launch(hzsdr_covar *c, const CvArgs &a) {
    return with_format(c->fmt, [&](auto f) { return cv_launch_fmt<decltype(f)::value>(c, a); });
}

// the node scratch for `nodes` nodes, grow-only
static int cv_scratch(hzsdr_covar *c, uint64_t nodes) {
    hzsdr_ctx *ctx = c->ctx;
    if (nodes <= c->nodes_cap) return HZSDR_OK;
    HZ_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the old scratch may still be read by a launched round)
    if (c->nodes) (void)hipFree(c->nodes);
    c->nodes = nullptr, c->nodes_cap = 0;
    HZ_HIP(ctx, hipMalloc((void **)&c->nodes, (size_t)nodes * vp::covar_node_floats(c->N) * sizeof(float)));
    c->nodes_cap = (size_t)nodes;
    return HZSDR_OK;
}

// one launch round: n snapshots of the device rows (or the flush), blocks to dout; the scratch holds p.w.nodes
static int cv_round(hzsdr_covar *c, const vp::Step &p, const CvRows &rows, float2 *dout, size_t out_stride) {
    CvArgs a{rows, c->tail[c->tcur], c->tail[c->tcur ^ 1], c->nodes, c->stack[c->scur], c->stack[c->scur ^ 1], dout, out_stride, p.w, c->N, c->B};
    HZ_TRY(cv_launch(c, a));
    if (p.w.held_out) c->tcur ^= 1;
    if (p.w.keep) c->scur ^= 1;
    c->st = p.next;
    return HZSDR_OK;
}

// the whole push over device rows, cut into rounds.  The scratch of the largest round is there before the first one is
// launched, so that nothing but a failed launch can stop a push half way.
static int cv_push_device(hzsdr_covar *c, const CvRows &rows, size_t n_in, float2 *dout, size_t out_stride) {
    const uint64_t round = vp::covar_round(c->B);
    const size_t size = (size_t)format_size(c->fmt);
    uint64_t most = 0;
    vp::State st = c->st;
    for (size_t at = 0; at < n_in;) {
        const size_t n = n_in - at < round ? n_in - at : (size_t)round;
        const vp::Step p = vp::covar_step(st, c->B, n);
        if (p.w.nodes > most) most = p.w.nodes;
        st = p.next, at += n;
    }
    HZ_TRY(cv_scratch(c, most));
    size_t at = 0;
    while (at < n_in) {
        const size_t n = n_in - at < round ? n_in - at : (size_t)round;
        const vp::Step p = vp::covar_step(c->st, c->B, n);
        CvRows here;
        for (uint32_t i = 0; i < c->N; i++) here.p[i] = (const char *)rows.p[i] + at * size;
        for (uint32_t i = c->N; i < vp::kMaxChannels; i++) here.p[i] = nullptr;
        HZ_TRY(cv_round(c, p, here, dout, out_stride));
        dout += (size_t)p.w.written * out_stride;
        at += n;
    }
    return HZSDR_OK;
}

__global__ __launch_bounds__(kThreads) void scan_kernel(const float2 *__restrict__ mats, size_t mat_stride, const float2 *__restrict__ w, uint32_t N,
                                                        uint32_t G, float *__restrict__ out, size_t out_stride) {
    __shared__ cv::c32 Q[vp::kMaxChannels * vp::kMaxChannels];
    const size_t b = blockIdx.y;
    for (uint32_t i = threadIdx.x; i < N * N; i += kThreads) {
        const float2 q = mats[b * mat_stride + i];
        Q[i] = cv::c32{q.x, q.y};
    }
    __syncthreads();
    const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
    if (g >= G) return;
    cv::c32 wv[vp::kMaxChannels];
    for (uint32_t i = 0; i < N; i++) {
        const float2 x = w[(size_t)g * N + i];
        wv[i] = cv::c32{x.x, x.y};
    }
    out[b * out_stride + g] = cv::scan_power(Q, wv, N);
}

}  // namespace hz

extern "C" {

int hzsdr_covar_create(hzsdr_ctx *ctx, int src_format, size_t channels, size_t block, hzsdr_covar **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (format_size(src_format) == 0) return fail(ctx, HZSDR_ERR_FORMAT_UNKNOWN, "covar: unknown source format");
    if (channels < vp::kMinChannels || channels > vp::kMaxChannels) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: the channel count is 2 ... 16");
    if (block < 1 || block > vp::kMaxBlock) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: the block is 1 ... 2^24 snapshots");
    HZ_TRY(enter(ctx));
    hzsdr_covar *c = new hzsdr_covar{ctx, src_format, (uint32_t)channels, (uint32_t)block};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&c->stack[i], (size_t)vp::kLevels * vp::covar_node_floats(c->N) * sizeof(float));
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipMalloc((void **)&c->tail[i], (size_t)c->N * vp::kSeg * sizeof(float2));
    if (e != hipSuccess) {
        hzsdr_covar_free(c);
        return hip_fail(ctx, e, "covar_create", __FILE__, __LINE__);
    }
    *out = c;
    return HZSDR_OK;
}

int hzsdr_covar_blocks_for(const hzsdr_covar *c, size_t n_in, size_t *blocks) {
    if (!c || !blocks) return HZSDR_ERR_INVALID_ARGUMENT;
    const hz::vp::Step p = hz::vp::covar_step(c->st, c->B, n_in);
    if (!p.ok) return hz::fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: the push is too long");
    *blocks = (size_t)p.w.written;
    return HZSDR_OK;
}

// rows: the caller's N row pointers (HOST or DEVICE space)
static int covar_push_rows(hzsdr_covar *c, const void *const *rows, const void *pitched, size_t n_in, size_t in_stride, void *out, size_t out_cap,
                           size_t out_stride, size_t *written) {
    using namespace hz;
    hzsdr_ctx *ctx = c->ctx;
    const vp::Step p = vp::covar_step(c->st, c->B, n_in);
    if (!p.ok) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: the push is too long");
    const size_t nb = (size_t)p.w.written, nn = (size_t)c->N * c->N, size = (size_t)format_size(c->fmt);
    if (out_cap < nb) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "covar: output buffer too small for the blocks of the push");
    if (nb > 1 && out_stride < nn) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "covar: out_stride is below channels^2");
    if (nb && !out) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: null output");
    HZ_TRY(enter(ctx));
    if (n_in == 0) return HZSDR_OK;
    if (nb <= 1) out_stride = nn;
    Stage st(ctx);
    CvRows dev{};
    if (pitched) {
        const void *din;
        HZ_TRY(st.in(1, pitched, ((size_t)(c->N - 1) * in_stride + n_in) * size, &din));
        for (uint32_t i = 0; i < c->N; i++) dev.p[i] = (const char *)din + (size_t)i * in_stride * size;
    } else {
        for (uint32_t i = 0; i < c->N; i++) HZ_TRY(st.in(1 + (int)i, rows[i], n_in * size, &dev.p[i]));
    }
    void *dout = nullptr;
    if (nb) {
        const size_t bytes = ((nb - 1) * out_stride + nn) * sizeof(float2);
        if (out_stride > nn)
            HZ_TRY(st.out_preserve(0, out, bytes, &dout));  // (the columns behind N^2 stay as they are)
        else
            HZ_TRY(st.out(0, out, bytes, &dout));
    }
    HZ_TRY(cv_push_device(c, dev, n_in, (float2 *)dout, out_stride));
    HZ_TRY(st.finish());
    if (written) *written = nb;
    return HZSDR_OK;
}

int hzsdr_covar_push(hzsdr_covar *c, const void *in, size_t n_in, size_t in_stride, void *out, size_t out_blocks_cap, size_t out_stride,
                     size_t *blocks_written) {
    using namespace hz;
    if (blocks_written) *blocks_written = 0;
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (n_in && !in) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: null input");
    if (in_stride < n_in) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: in_stride is below the samples of the push");
    return covar_push_rows(c, nullptr, in, n_in, in_stride, out, out_blocks_cap, out_stride, blocks_written);
}

int hzsdr_covar_push_channels(hzsdr_covar *c, const void *const *channels, size_t n_in, void *out, size_t out_blocks_cap, size_t out_stride,
                              size_t *blocks_written) {
    using namespace hz;
    if (blocks_written) *blocks_written = 0;
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (!channels) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: null channel list");
    for (uint32_t i = 0; i < c->N; i++)
        if (n_in && !channels[i]) return fail(c->ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: null channel");
    return covar_push_rows(c, channels, nullptr, n_in, 0, out, out_blocks_cap, out_stride, blocks_written);
}

int hzsdr_covar_flush(hzsdr_covar *c, void *out, size_t out_blocks_cap, size_t *blocks_written) {
    using namespace hz;
    if (blocks_written) *blocks_written = 0;
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = c->ctx;
    const vp::Step p = vp::covar_flush(c->st);
    const size_t nb = (size_t)p.w.written, nn = (size_t)c->N * c->N;
    if (out_blocks_cap < nb) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "covar: output buffer too small for the open block");
    if (nb && !out) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "covar: null output");
    HZ_TRY(enter(ctx));
    if (nb) {
        Stage st(ctx);
        void *dout;
        HZ_TRY(st.out(0, out, nn * sizeof(float2), &dout));
        HZ_TRY(cv_scratch(c, p.w.nodes));
        HZ_TRY(cv_round(c, p, CvRows{}, (float2 *)dout, nn));
        HZ_TRY(st.finish());
    }
    c->st = p.next;
    if (blocks_written) *blocks_written = nb;
    return HZSDR_OK;
}

int hzsdr_covar_pending(const hzsdr_covar *c, uint64_t *consumed, uint64_t *next_block, size_t *open_snapshots) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (consumed) *consumed = c->st.consumed;
    if (next_block) *next_block = c->st.block;
    if (open_snapshots) *open_snapshots = c->st.open;
    return HZSDR_OK;
}

int hzsdr_covar_plan(const hzsdr_covar *c, size_t *segment, size_t *group_segments, int *form) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    if (segment) *segment = hz::vp::kSeg;
    if (group_segments) *group_segments = hz::vp::kGroup;
    if (form) *form = c->N <= 8 ? HZSDR_COVAR_FORM_ONE_TILE : HZSDR_COVAR_FORM_THREE_TILES;
    return HZSDR_OK;
}

int hzsdr_covar_reset(hzsdr_covar *c) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    // (the held snapshots and the stack are only read behind a later push's own writes: nothing to clear)
    c->st = hz::vp::State{};
    return HZSDR_OK;
}

int hzsdr_covar_free(hzsdr_covar *c) {
    if (!c) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(c->ctx, {c->tail[0], c->tail[1], c->stack[0], c->stack[1], c->nodes});
    delete c;
    return HZSDR_OK;
}

int hzsdr_scan_create(hzsdr_ctx *ctx, size_t channels, const void *weights, size_t count, hzsdr_scan **out) {
    using namespace hz;
    if (!ctx || !out) return HZSDR_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (channels < vp::kMinChannels || channels > vp::kMaxChannels) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: the channel count is 2 ... 16");
    if (count < 1 || count > HZSDR_SCAN_MAX_VECTORS) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: 1 ... 65536 weight vectors");
    if (!weights) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: null weights");
    HZ_TRY(enter(ctx));
    hzsdr_scan *s = new hzsdr_scan{ctx, (uint32_t)channels, (uint32_t)count};
    const size_t bytes = count * channels * sizeof(float2);
    hipError_t e = hipMalloc((void **)&s->w, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(s->w, weights, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // (weights is the caller's: free to go when create returns)
    if (e != hipSuccess) {
        hzsdr_scan_free(s);
        return hip_fail(ctx, e, "scan_create", __FILE__, __LINE__);
    }
    *out = s;
    return HZSDR_OK;
}

int hzsdr_scan_run(hzsdr_scan *s, const void *mats, size_t n_mats, size_t mat_stride, void *out, size_t out_cap, size_t out_stride) {
    using namespace hz;
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hzsdr_ctx *ctx = s->ctx;
    const size_t nn = (size_t)s->N * s->N;
    if (n_mats == 0) return HZSDR_OK;
    if (!mats || !out) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: null buffer");
    if (n_mats > 65535) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: at most 65535 matrices per run");
    if (n_mats > 1 && mat_stride < nn) return fail(ctx, HZSDR_ERR_INVALID_ARGUMENT, "scan: mat_stride is below channels^2");
    if (n_mats > 1 && out_stride < s->G) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "scan: out_stride is below the weight vectors");
    if (n_mats == 1) mat_stride = nn, out_stride = s->G;
    if (out_cap < (n_mats - 1) * out_stride + s->G) return fail(ctx, HZSDR_ERR_DST_TOO_SMALL, "scan: output buffer too small");
    HZ_TRY(enter(ctx));
    Stage st(ctx);
    const void *dm;
    void *dout;
    HZ_TRY(st.in(1, mats, ((n_mats - 1) * mat_stride + nn) * sizeof(float2), &dm));
    const size_t obytes = ((n_mats - 1) * out_stride + s->G) * sizeof(float);
    if (out_stride > s->G)
        HZ_TRY(st.out_preserve(0, out, obytes, &dout));
    else
        HZ_TRY(st.out(0, out, obytes, &dout));
    hipLaunchKernelGGL(scan_kernel, dim3((s->G + kThreads - 1) / kThreads, (unsigned)n_mats), dim3(kThreads), 0, ctx->stream, (const float2 *)dm,
                       mat_stride, s->w, s->N, s->G, (float *)dout, out_stride);
    HZ_HIP(ctx, hipGetLastError());
    return st.finish();
}

int hzsdr_scan_free(hzsdr_scan *s) {
    if (!s) return HZSDR_ERR_INVALID_ARGUMENT;
    hz::bank_release(s->ctx, {s->w});
    delete s;
    return HZSDR_OK;
}

}  // extern "C"

#if defined(HZSDR_NO_PK_F32) && defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
