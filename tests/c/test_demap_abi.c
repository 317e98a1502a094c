/* test_demap_abi.c -- the demapper bank (hzsdr_demap.h) exercised by a C compiler (gcc -std=c99) in a HOST context:
 * QPSK points written here with bit 1 on the positive side of each axis, two pitched rows of three frame slots of four
 * symbols; the signs of the values are the sent bits and their sizes are 4 |x| g by the algebra of the four points; a
 * perm with a hole and a flip reorder, erase and negate them; a NaN symbol is an erasure; the slots behind a row's count
 * and the floats behind cap frames stay as they were; per-bit values pass with gain and sign alone; sizes and plan;
 * refused calls write nothing; configurations out of bounds are refused.  Prints "demap-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_demap.h"

static int failures = 0;
static hzsdr_ctx *ctx;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                            \
        }                                                          \
    } while (0)
#define OK(call)                                                                                                      \
    do {                                                                                                              \
        int rc__ = (call);                                                                                            \
        if (rc__ != HZSDR_OK) {                                                                                       \
            printf("FAIL %s:%d: %s -> %s (%s)\n", __FILE__, __LINE__, #call, hzsdr_strerror(rc__), hzsdr_last_error(ctx)); \
            failures++;                                                                                               \
        }                                                                                                             \
    } while (0)

enum { S = 4, M = 2, W = 2 * S, N = S * M, R = 2, CAP = 3, IPITCH = CAP * W + 3, OPITCH = CAP * N + 5, NP = N + 1 };
/* label p = b0 b1: b0 on Re, b1 on Im, 1 is the positive side; the points at +-1 */
static const float points[8] = {-1, -1, -1, 1, 1, -1, 1, 1};

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

static unsigned dibit_of(int r, int f, int s) { return (unsigned)(r * 7 + f * 3 + s) & 3u; }

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;

    hzsdr_demap *d = NULL, *bad = NULL;
    const float gains[R] = {0.5f, 2.0f}, one = 1.0f, zero = 0.0f, inf_point[8] = {-1, -1, -1, 1, 1, -1, 1, INFINITY};
    uint32_t perm[NP], forged[NP];
    for (int k = 0; k < N; k++) perm[k] = (uint32_t)(N - 1 - k); /* reversal */
    perm[N] = HZSDR_DEMAP_ERASED;
    perm[2] = perm[3]; /* a repeat */
    memcpy(forged, perm, sizeof forged);
    forged[4] = N;
    const uint8_t flip[2] = {0x0F, 0x80}; /* the bits 4 ... 8 */
    CHECK(hzsdr_demap_create(ctx, 7, M, points, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, 0, points, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, 9, points, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, NULL, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, inf_point, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, 0, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, HZSDR_DEMAP_MAX_SYMBOLS + 1, perm, NP, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N - 1, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, perm, 0, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, forged, NP, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, &zero, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, NULL, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, gains, R, R + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, &one, 1, HZSDR_DEMAP_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_LLR_F32, 1, points, S, NULL, S, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_create(ctx, HZSDR_DEMAP_LLR_F32, 2, NULL, S, NULL, N, NULL, &one, 1, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(bad == NULL);

    OK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, gains, R, R, &d));
    size_t s = 0, w = 0, m = 0, n = 0, g = 0, t = 0, bytes = 0;
    int form = -1;
    OK(hzsdr_demap_sizes(d, &s, &w, &m, &n));
    OK(hzsdr_demap_plan(d, &g, &t, &bytes, &form));
    CHECK(s == S && w == W && m == M && n == N && g == 8 && t == 64 && bytes == 4 * N && form == HZSDR_DEMAP_FORM_GROUPED);
    OK(hzsdr_demap_sizes(d, NULL, NULL, NULL, NULL));

    float *in = (float *)calloc((size_t)R * IPITCH, sizeof(float)), *out = (float *)malloc((size_t)R * OPITCH * sizeof(float));
    const uint32_t counts[R] = {CAP + 4, 2};
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++)
            for (int k = 0; k < S; k++) {
                const unsigned p = dibit_of(r, f, k);
                const float mag = 0.25f * (float)(1 + (r + f + k) % 4); /* exact in float32 */
                in[r * IPITCH + f * W + 2 * k] = ((p & 2u) ? 1.0f : -1.0f) * mag;
                in[r * IPITCH + f * W + 2 * k + 1] = ((p & 1u) ? 1.0f : -1.0f) * mag * 0.5f;
            }
    in[0 * IPITCH + 1 * W + 2] = NAN; /* row 0, frame 1, symbol 1: Re */
    memset(out, 0xA5, (size_t)R * OPITCH * sizeof(float));
    OK(hzsdr_demap_run(d, in, IPITCH, counts, CAP, out, OPITCH));
    for (int r = 0; r < R; r++) {
        for (int f = 0; f < CAP; f++)
            for (int k = 0; k < S; k++)
                for (int j = 0; j < M; j++) {
                    const float v = out[r * OPITCH + f * N + k * M + j], x = in[r * IPITCH + f * W + 2 * k + j];
                    if (f >= (int)(counts[r] < CAP ? counts[r] : CAP)) {
                        CHECK(bits_of(v) == 0xA5A5A5A5u);
                    } else if (r == 0 && f == 1 && k == 1) {
                        CHECK(bits_of(v) == 0x7FC00000u);
                    } else { /* (x + 1)^2 - (x - 1)^2 = 4 x, exact for these values: the other axis cancels */
                        CHECK(v == 4.0f * x * gains[r]);
                    }
                }
        for (int b = CAP * N; b < OPITCH; b++) CHECK(bits_of(out[r * OPITCH + b]) == 0xA5A5A5A5u);
    }
    /* refused calls write nothing */
    memset(out, 0xA5, (size_t)R * OPITCH * sizeof(float));
    CHECK(hzsdr_demap_run(d, in, IPITCH, NULL, CAP, out, CAP * N - 1) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_demap_run(d, in, CAP * W - 1, NULL, CAP, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, in, IPITCH, NULL, 0, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, in, IPITCH, NULL, HZSDR_DEMAP_MAX_FRAMES / R + 1, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, NULL, IPITCH, NULL, CAP, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, in, IPITCH, NULL, CAP, NULL, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, out, OPITCH, NULL, CAP, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(d, out + 7, OPITCH, NULL, 1, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demap_run(NULL, in, IPITCH, NULL, CAP, out, OPITCH) == HZSDR_ERR_INVALID_ARGUMENT);
    for (int b = 0; b < R * OPITCH; b++) CHECK(bits_of(out[b]) == 0xA5A5A5A5u);
    OK(hzsdr_demap_free(d));

    /* order, a hole, a repeat and signs: one row, shared gain 1 */
    hzsdr_demap *p = NULL;
    float dense[N], ordered[NP];
    OK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, NULL, N, NULL, &one, 1, 1, &d));
    OK(hzsdr_demap_create(ctx, HZSDR_DEMAP_C64, M, points, S, perm, NP, flip, &one, 1, 1, &p));
    OK(hzsdr_demap_plan(p, NULL, NULL, NULL, &form));
    CHECK(form == (HZSDR_DEMAP_FORM_GROUPED | HZSDR_DEMAP_FORM_PERM));
    OK(hzsdr_demap_run(d, in + IPITCH, 0, NULL, 1, dense, 0));
    OK(hzsdr_demap_run(p, in + IPITCH, 0, NULL, 1, ordered, 0));
    for (int k = 0; k < NP; k++) {
        const int flipped = k >= 4 && k <= 8;
        if (perm[k] == HZSDR_DEMAP_ERASED)
            CHECK(bits_of(ordered[k]) == 0x7FC00000u);
        else
            CHECK(bits_of(ordered[k]) == (bits_of(dense[perm[k]]) ^ (flipped ? 0x80000000u : 0u)));
    }
    OK(hzsdr_demap_free(d));
    OK(hzsdr_demap_free(p));

    /* per-bit values: gain and sign alone */
    hzsdr_demap *l = NULL;
    const uint8_t every = 0xFF;
    const float half = 0.5f, vals[8] = {1.0f, -2.0f, 0.0f, -0.0f, INFINITY, NAN, 3.5f, -1e-40f};
    float got[8];
    OK(hzsdr_demap_create(ctx, HZSDR_DEMAP_LLR_F32, 1, NULL, 8, NULL, 8, &every, &half, 1, 1, &l));
    OK(hzsdr_demap_sizes(l, &s, &w, &m, &n));
    CHECK(s == 8 && w == 8 && m == 1 && n == 8);
    OK(hzsdr_demap_run(l, vals, 0, NULL, 1, got, 0));
    for (int k = 0; k < 8; k++) CHECK(bits_of(got[k]) == (k == 5 ? 0x7FC00000u : bits_of(-(vals[k] * 0.5f))));
    OK(hzsdr_demap_free(l));
    CHECK(hzsdr_demap_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    free(in), free(out);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demap-abi ok\n");
    return 0;
}
