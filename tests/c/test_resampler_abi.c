/* test_resampler_abi.c -- the polyphase rational resampler (hzsdr_resampler.h) exercised by a C compiler
 * (gcc -std=c99) in a HOST context: 3/2 of a short complex64 stream against the definition evaluated here in double,
 * the counts of pushes and flush, samples cut anywhere writing the bits one push writes, two pitched rows equal to
 * two single-stream runs, a too-small destination refused without a change of state.  Prints "resampler-abi ok" and
 * exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_resampler.h"

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

enum { U = 3, D = 2, L = 22, Q = (L + U - 1) / U, N = 1000, HEAD = (N * U + D - 1) / D, TOTAL = ((N - 1) * U + L + D - 1) / D, PITCH = N + 7 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    float h[L];
    for (int k = 0; k < L; k++) h[k] = (float)(0.05 * (k + 1) * (L - k) / L) * ((k % 5) ? 1.0f : -1.0f);
    /* two rows that differ, with a pitch */
    float *x = (float *)calloc((size_t)2 * PITCH * 2, sizeof(float));
    for (int s = 0; s < 2; s++)
        for (int i = 0; i < N; i++) {
            x[2 * (s * PITCH + i)] = (float)sin(0.37 * i + s) * 0.7f;
            x[2 * (s * PITCH + i) + 1] = (float)cos(0.11 * i * (s + 1)) * 0.4f;
        }
    hzsdr_resampler *r = NULL, *two = NULL, *bad = NULL;
    CHECK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, 0, D, h, L, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, U, 1025, h, L, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, U, D, NULL, L, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, U, D, h, L, 8193, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_resampler_create(ctx, 9, U, D, h, L, 1, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    OK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, U, D, h, L, 1, &r));
    OK(hzsdr_resampler_create(ctx, HZSDR_FMT_C64, U, D, h, L, 2, &two));
    size_t tile = 0, got = 0, want = 0, fl = 0;
    int form = -1;
    uint64_t consumed = 9, next = 9;
    OK(hzsdr_resampler_plan(r, &tile, &form));
    CHECK(tile >= 64 && form == 0);
    OK(hzsdr_resampler_outputs_for(r, N, &want));
    CHECK(want == HEAD);
    float *a = (float *)calloc((size_t)TOTAL * 2, sizeof(float));
    /* a destination one value short: refused, nothing consumed */
    CHECK(hzsdr_resampler_push(r, x, N, 0, a, HEAD - 1, 0, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_resampler_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    OK(hzsdr_resampler_push(r, x, N, 0, a, HEAD, 0, &got));
    CHECK(got == HEAD);
    OK(hzsdr_resampler_pending(r, &consumed, &next, &fl));
    CHECK(consumed == N && next == HEAD && fl == TOTAL - HEAD);
    CHECK(hzsdr_resampler_flush(r, a + 2 * HEAD, TOTAL - HEAD - 1, 0, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_resampler_flush(r, a + 2 * HEAD, TOTAL - HEAD, 0, &got));
    CHECK(got == TOTAL - HEAD);
    OK(hzsdr_resampler_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    /* the definition: y[m] = sum_q h[phi + q U] x[i - q], phi = m D mod U, i = m D / U */
    for (int m = 0; m < TOTAL; m++) {
        const int phi = (m * D) % U, i = (m * D) / U;
        double re = 0.0, im = 0.0, mag = 0.0;
        for (int q = 0; q < Q; q++) {
            const int k = phi + q * U, j = i - q;
            if (k >= L || j < 0 || j >= N) continue;
            re += (double)h[k] * x[2 * j];
            im += (double)h[k] * x[2 * j + 1];
            mag += fabs((double)h[k]);
        }
        CHECK(fabs(a[2 * m] - re) <= 1e-6 * mag + 1e-30 && fabs(a[2 * m + 1] - im) <= 1e-6 * mag + 1e-30);
    }
    /* the same samples in five pushes (one empty, one of a single sample, one inside the first Q - 1) */
    float *b = (float *)calloc((size_t)TOTAL * 2, sizeof(float));
    const size_t cuts[6] = {0, 3, 3, 4, 611, N};
    size_t done = 0;
    for (int i = 0; i < 5; i++) {
        size_t w = 0;
        OK(hzsdr_resampler_push(r, x + 2 * cuts[i], cuts[i + 1] - cuts[i], 0, b + 2 * done, TOTAL - done, 0, &w));
        done += w;
        CHECK(done == (cuts[i + 1] * U + D - 1) / D);
    }
    OK(hzsdr_resampler_flush(r, b + 2 * done, TOTAL - done, 0, &got));
    CHECK(done + got == TOTAL);
    CHECK(memcmp(a, b, sizeof(float) * 2 * TOTAL) == 0);
    /* two rows with pitches on both sides: row 0 is the run above, row 1 a run of its own; the columns behind the
     * outputs stay as they were */
    const size_t opitch = TOTAL + 3;
    float *c = (float *)malloc(sizeof(float) * 2 * 2 * opitch);
    memset(c, 0x7f, sizeof(float) * 2 * 2 * opitch);
    CHECK(hzsdr_resampler_push(two, x, N, N - 1, c, opitch, opitch, &got) == HZSDR_ERR_INVALID_ARGUMENT && got == 0);
    CHECK(hzsdr_resampler_push(two, x, N, PITCH, c, opitch, HEAD - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_resampler_push(two, x, N, PITCH, c, opitch, opitch, &got));
    CHECK(got == HEAD);
    OK(hzsdr_resampler_flush(two, c + 2 * HEAD, opitch - HEAD, opitch, &got));
    CHECK(got == TOTAL - HEAD);
    CHECK(memcmp(c, a, sizeof(float) * 2 * TOTAL) == 0);
    OK(hzsdr_resampler_push(r, x + 2 * PITCH, N, 0, b, TOTAL, 0, &done));
    OK(hzsdr_resampler_flush(r, b + 2 * done, TOTAL - done, 0, &got));
    CHECK(memcmp(c + 2 * opitch, b, sizeof(float) * 2 * TOTAL) == 0);
    for (int s = 0; s < 2; s++)
        for (size_t k = 2 * TOTAL; k < 2 * opitch; k++) {
            uint32_t v;
            memcpy(&v, c + 2 * s * opitch + k, 4);
            CHECK(v == 0x7f7f7f7fu);
        }
    /* reset mid-stream */
    OK(hzsdr_resampler_push(r, x, 10, 0, b, TOTAL, 0, &got));
    OK(hzsdr_resampler_reset(r));
    OK(hzsdr_resampler_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    OK(hzsdr_resampler_free(r));
    OK(hzsdr_resampler_free(two));
    free(x);
    free(a);
    free(b);
    free(c);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("resampler-abi ok\n");
    return 0;
}
