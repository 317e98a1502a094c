/* test_spectrum_abi.c -- the fused power spectrum (hzsdr_spectrum.h) exercised by a C compiler (gcc -std=c99) in
 * a HOST context: a tone lands in its bin in both orders, a push that is cut anywhere writes the rows one push
 * writes, a too-small destination is refused without a change of state.  Prints "spectrum-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_spectrum.h"

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

enum { N = 256, HOP = 128, AVG = 3, LEN = 20 * HOP + N };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* a tone in bin 10: exp(2 pi i 10 t / N) */
    float *x = (float *)malloc(sizeof(float) * 2 * LEN);
    for (int t = 0; t < LEN; t++) {
        const double ph = 2.0 * 3.14159265358979323846 * 10.0 * (double)t / N;
        x[2 * t] = (float)cos(ph);
        x[2 * t + 1] = (float)sin(ph);
    }
    hzsdr_spectrum *z = NULL, *g = NULL;
    OK(hzsdr_spectrum_create(ctx, HZSDR_FMT_C64, N, HOP, AVG, NULL, 1.0f / ((float)AVG * N * N), HZSDR_ORDER_ZERO_FIRST,
                             HZSDR_SPECTRUM_POWER, &z));
    OK(hzsdr_spectrum_create(ctx, HZSDR_FMT_C64, N, HOP, AVG, NULL, 1.0f / ((float)AVG * N * N), HZSDR_ORDER_NEGATIVE_FIRST,
                             HZSDR_SPECTRUM_DB, &g));
    size_t rows = 0, got = 0, frames = 0, held = 0;
    OK(hzsdr_spectrum_rows_for(z, LEN, &rows));
    CHECK(rows == ((LEN - N) / HOP + 1) / AVG);
    float *a = (float *)calloc(rows * N, sizeof(float)), *b = (float *)calloc(rows * N, sizeof(float));
    /* a destination of rows - 1: refused, nothing consumed */
    CHECK(hzsdr_spectrum_push(z, x, LEN, a, rows - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_spectrum_pending(z, &frames, &held));
    CHECK(frames == 0 && held == 0);
    OK(hzsdr_spectrum_push(z, x, LEN, a, rows, &got));
    CHECK(got == rows);
    for (size_t r = 0; r < rows; r++) {
        CHECK(fabsf(a[r * N + 10] - 1.0f) < 1e-4f);
        CHECK(a[r * N + 11] < 1e-8f);
    }
    /* the same stream in three pushes (one shorter than a frame), NegativeFirst in dB: bin 10 sits at N/2 + 10 */
    size_t w0 = 0, w1 = 0, w2 = 0;
    OK(hzsdr_spectrum_options(g, HZSDR_SPECTRUM_FORM_FRAME_PARALLEL));
    OK(hzsdr_spectrum_push(g, x, 100, b, rows, &w0));
    OK(hzsdr_spectrum_push(g, x + 2 * 100, 1000, b + w0 * N, rows - w0, &w1));
    OK(hzsdr_spectrum_push(g, x + 2 * 1100, LEN - 1100, b + (w0 + w1) * N, rows - w0 - w1, &w2));
    CHECK(w0 + w1 + w2 == rows);
    int form = 0;
    OK(hzsdr_spectrum_last_form(g, &form));
    CHECK(form == HZSDR_SPECTRUM_FORM_FRAME_PARALLEL);
    for (size_t r = 0; r < rows; r++) CHECK(fabsf(b[r * N + N / 2 + 10] - 10.0f * log10f(a[r * N + 10])) < 1e-4f);
    OK(hzsdr_spectrum_reset(g));
    OK(hzsdr_spectrum_pending(g, &frames, &held));
    CHECK(frames == 0 && held == 0);
    OK(hzsdr_spectrum_free(z));
    OK(hzsdr_spectrum_free(g));
    free(x);
    free(a);
    free(b);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("spectrum-abi ok\n");
    return 0;
}
