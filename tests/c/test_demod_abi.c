/* test_demod_abi.c -- the demodulator bank (hzsdr_demod.h) exercised by a C compiler (gcc -std=c99) in a HOST context:
 * FM of a short complex64 stream, filtered and decimated by 3, against the definition evaluated here in double, the
 * counts of pushes and flush, samples cut anywhere writing the bits one push writes, two pitched rows equal to two
 * single-stream runs, a too-small destination refused without a change of state, the envelope of a 3-4-5 sample.
 * Prints "demod-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_demod.h"

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

enum { D = 3, Q = 22, N = 1000, HEAD = (N + D - 1) / D, TOTAL = (N - 1 + Q + D - 1) / D, PITCH = N + 7 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    float h[Q];
    for (int k = 0; k < Q; k++) h[k] = (float)(0.05 * (k + 1) * (Q - k) / Q) * ((k % 5) ? 1.0f : -1.0f);
    /* two rows that differ, with a pitch */
    float *x = (float *)calloc((size_t)2 * PITCH * 2, sizeof(float));
    for (int s = 0; s < 2; s++)
        for (int i = 0; i < N; i++) {
            /* an FM signal with a moving envelope: the phase advances by 0.3 +- 0.05 rad per sample */
            const double phi = 0.3 * i + 2.0 * sin(0.013 * i * (s + 1)), amp = 0.6 + 0.3 * cos(0.07 * i + s);
            x[2 * (s * PITCH + i)] = (float)(amp * cos(phi));
            x[2 * (s * PITCH + i) + 1] = (float)(amp * sin(phi));
        }
    hzsdr_demod *r = NULL, *two = NULL, *bad = NULL;
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, 0, D, h, Q, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_POWER + 1, D, h, Q, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, 65, h, Q, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, D, NULL, Q, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, D, h, 1025, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, D, h, Q, 8193, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_demod_create(ctx, 9, HZSDR_DEMOD_FM, D, h, Q, 1, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    OK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, D, h, Q, 1, &r));
    OK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_FM, D, h, Q, 2, &two));
    size_t tile = 0, got = 0, want = 0, fl = 0;
    int form = -1;
    uint64_t consumed = 9, next = 9;
    OK(hzsdr_demod_plan(r, &tile, &form));
    CHECK(tile == 1024 && form == HZSDR_DEMOD_FORM_TRANSPOSED);
    OK(hzsdr_demod_outputs_for(r, N, &want));
    CHECK(want == HEAD);
    float *a = (float *)calloc((size_t)TOTAL, sizeof(float));
    /* a destination one value short: refused, nothing consumed */
    CHECK(hzsdr_demod_push(r, x, N, 0, a, HEAD - 1, 0, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_demod_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    OK(hzsdr_demod_push(r, x, N, 0, a, HEAD, 0, &got));
    CHECK(got == HEAD);
    OK(hzsdr_demod_pending(r, &consumed, &next, &fl));
    CHECK(consumed == N && next == HEAD && fl == TOTAL - HEAD);
    CHECK(hzsdr_demod_flush(r, a + HEAD, TOTAL - HEAD - 1, 0, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_demod_flush(r, a + HEAD, TOTAL - HEAD, 0, &got));
    CHECK(got == TOTAL - HEAD);
    OK(hzsdr_demod_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    /* the definition: d[n] = angle(x[n] conj(x[n - 1])), y[m] = sum_q h[q] d[m D - q] */
    double *d = (double *)calloc(N, sizeof(double));
    for (int n = 0; n < N; n++) {
        const double ar = x[2 * n], ai = x[2 * n + 1], br = n ? x[2 * n - 2] : 0.0, bi = n ? x[2 * n - 1] : 0.0;
        const double pr = ar * br + ai * bi, pi = ai * br - ar * bi;
        d[n] = (pr == 0.0 && pi == 0.0) ? 0.0 : atan2(pi, pr);
    }
    for (int m = 0; m < TOTAL; m++) {
        double y = 0.0, mag = 0.0;
        for (int q = 0; q < Q; q++) {
            const int n = m * D - q;
            if (n < 0 || n >= N) continue;
            y += (double)h[q] * d[n];
            mag += fabs((double)h[q]);
        }
        /* (the float32 product's own rounding moves the angle of a small product: 2e-6 per tap is generous) */
        CHECK(fabs(a[m] - y) <= 2e-6 * mag + 1e-30);
    }
    /* the same samples in five pushes (one empty, one of a single sample, one inside the first Q) */
    float *b = (float *)calloc((size_t)TOTAL, sizeof(float));
    const size_t cuts[6] = {0, 3, 3, 4, 611, N};
    size_t done = 0;
    for (int i = 0; i < 5; i++) {
        size_t w = 0;
        OK(hzsdr_demod_push(r, x + 2 * cuts[i], cuts[i + 1] - cuts[i], 0, b + done, TOTAL - done, 0, &w));
        done += w;
        CHECK(done == (cuts[i + 1] + D - 1) / D);
    }
    OK(hzsdr_demod_flush(r, b + done, TOTAL - done, 0, &got));
    CHECK(done + got == TOTAL);
    CHECK(memcmp(a, b, sizeof(float) * TOTAL) == 0);
    /* two rows with pitches on both sides: row 0 is the run above, row 1 a run of its own; the columns behind the
     * outputs stay as they were */
    const size_t opitch = TOTAL + 3;
    float *c = (float *)malloc(sizeof(float) * 2 * opitch);
    memset(c, 0x7f, sizeof(float) * 2 * opitch);
    CHECK(hzsdr_demod_push(two, x, N, N - 1, c, opitch, opitch, &got) == HZSDR_ERR_INVALID_ARGUMENT && got == 0);
    CHECK(hzsdr_demod_push(two, x, N, PITCH, c, opitch, HEAD - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_demod_push(two, x, N, PITCH, c, opitch, opitch, &got));
    CHECK(got == HEAD);
    OK(hzsdr_demod_flush(two, c + HEAD, opitch - HEAD, opitch, &got));
    CHECK(got == TOTAL - HEAD);
    CHECK(memcmp(c, a, sizeof(float) * TOTAL) == 0);
    OK(hzsdr_demod_push(r, x + 2 * PITCH, N, 0, b, TOTAL, 0, &done));
    OK(hzsdr_demod_flush(r, b + done, TOTAL - done, 0, &got));
    CHECK(memcmp(c + opitch, b, sizeof(float) * TOTAL) == 0);
    for (int s = 0; s < 2; s++)
        for (size_t k = TOTAL; k < opitch; k++) {
            uint32_t v;
            memcpy(&v, c + s * opitch + k, 4);
            CHECK(v == 0x7f7f7f7fu);
        }
    /* reset mid-stream */
    OK(hzsdr_demod_push(r, x, 10, 0, b, TOTAL, 0, &got));
    OK(hzsdr_demod_reset(r));
    OK(hzsdr_demod_pending(r, &consumed, &next, &fl));
    CHECK(consumed == 0 && next == 0 && fl == 0);
    OK(hzsdr_demod_free(r));
    OK(hzsdr_demod_free(two));
    /* the bare envelope and power: exact on a 3-4-5 sample */
    const float one_tap[1] = {1.0f}, s345[4] = {3.0f, -4.0f, 0.0f, 0.0f};
    float e[2];
    OK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_ENVELOPE, 1, one_tap, 1, 1, &r));
    OK(hzsdr_demod_push(r, s345, 2, 0, e, 2, 0, &got));
    CHECK(got == 2 && e[0] == 5.0f && e[1] == 0.0f);
    OK(hzsdr_demod_free(r));
    OK(hzsdr_demod_create(ctx, HZSDR_FMT_C64, HZSDR_DEMOD_POWER, 1, one_tap, 1, 1, &r));
    OK(hzsdr_demod_push(r, s345, 2, 0, e, 2, 0, &got));
    CHECK(got == 2 && e[0] == 25.0f && e[1] == 0.0f);
    OK(hzsdr_demod_free(r));
    free(x);
    free(a);
    free(b);
    free(c);
    free(d);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("demod-abi ok\n");
    return 0;
}
