/* test_equalizer_abi.c -- the equalizer bank (hzsdr_equalizer.h) exercised by a C compiler (gcc -std=c99) in a HOST
 * context: a fresh bank (w[centre] = 1) with mu = 0 copies two pitched complex rows bit for bit and leaves the columns
 * behind them alone; with taps of small integers brought by set_state it is a fixed FIR whose outputs are exact sums;
 * counts stop a row where they say and are not rewritten; symbols cut anywhere write what one push writes, the state
 * carries into a second object, in place equals out of place, a refused push changes nothing, new parameters keep the
 * state, reset restores the initial one; one decision-directed update of a real row, worked out by hand.
 * Prints "equalizer-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_equalizer.h"

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

enum { N = 600, R = 2, PITCH = N + 5, OPITCH = N + 3, TPITCH = N + 2, TAPS = 3, WORDS = R * (2 * TAPS - 1) * 2 };

/* the fixed FIR of the test, w = (1, 2 - i, -1): y[n] = x[n] + (2 - i) x[n - 1] - x[n - 2], exact on small integers */
static void fir(const float *x, int n, float *re, float *im) {
    float xr[3] = {0, 0, 0}, xi[3] = {0, 0, 0};
    for (int k = 0; k < 3; k++)
        if (n - k >= 0) xr[k] = x[2 * (n - k)], xi[k] = x[2 * (n - k) + 1];
    *re = xr[0] + (2.0f * xr[1] + xi[1]) - xr[2];
    *im = xi[0] + (2.0f * xi[1] - xr[1]) - xi[2];
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    const float still[2] = {0.0f, 1.0f}, live[2] = {0.5f, 0.75f}, nonfinite[2] = {(float)INFINITY, 1.0f}, fast[2] = {1.5f, 1.0f}, flat[2] = {0.1f, 0.0f};
    float *x = (float *)calloc((size_t)R * PITCH * 2, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            x[(r * PITCH + i) * 2] = (float)(2 + (i * 7 + r * 3) % 23) * ((i + r) % 3 ? 1.0f : -1.0f);
            x[(r * PITCH + i) * 2 + 1] = (float)(2 + (i * 5 + r) % 19) * ((i + 2 * r) % 5 ? -1.0f : 1.0f);
        }
    hzsdr_equalizer *f = NULL, *g = NULL, *bad = NULL;
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, still, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, still, 0, HZSDR_EQUALIZER_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, 0, 0, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, HZSDR_EQUALIZER_MAX_TAPS + 1, 0, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, TAPS, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, 3, TAPS, 0, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_EQUALIZER_REAL_F32, HZSDR_EQUALIZER_DD_QPSK, TAPS, 0, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, NULL, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, nonfinite, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, fast, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_CMA, TAPS, 0, flat, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_create(ctx, HZSDR_FMT_U8, HZSDR_EQUALIZER_CMA, TAPS, 0, still, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    OK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_DD_QPSK, TAPS, 0, still, 0, R, &f));
    size_t rows_per_wave = 0, tile = 0;
    int form = -1;
    OK(hzsdr_equalizer_plan(f, &rows_per_wave, &tile, &form));
    CHECK(rows_per_wave == 1 && tile == 256 && form == HZSDR_EQUALIZER_FORM_COMPLEX);
    float *a = (float *)malloc(sizeof(float) * 2 * R * OPITCH), *b = (float *)malloc(sizeof(float) * 2 * R * OPITCH);
    float *t = (float *)malloc(sizeof(float) * R * TPITCH);
    for (int i = 0; i < 2 * R * OPITCH; i++) a[i] = b[i] = -77.0f;
    for (int i = 0; i < R * TPITCH; i++) t[i] = -77.0f;
    /* a fresh bank with mu = 0: a copy; the track is |clip(decision - y)|^2 = 2 for these integers */
    OK(hzsdr_equalizer_push(f, x, N, PITCH, NULL, a, OPITCH, t, TPITCH));
    for (int r = 0; r < R; r++) {
        CHECK(memcmp(a + 2 * r * OPITCH, x + 2 * r * PITCH, sizeof(float) * 2 * N) == 0);
        for (int i = 0; i < N; i++) CHECK(t[r * TPITCH + i] == 2.0f);
        for (int i = N; i < OPITCH; i++) CHECK(a[2 * (r * OPITCH + i)] == -77.0f && a[2 * (r * OPITCH + i) + 1] == -77.0f);
        for (int i = N; i < TPITCH; i++) CHECK(t[r * TPITCH + i] == -77.0f);
    }
    float z[WORDS], z2[WORDS], fresh[WORDS];
    CHECK(hzsdr_equalizer_get_state(f, z, WORDS - 1) == HZSDR_ERR_DST_TOO_SMALL);
    OK(hzsdr_equalizer_get_state(f, z, WORDS));
    for (int r = 0; r < R; r++) { /* taps (1, 0, 0), then x[N - 1], x[N - 2] */
        const float *zr = z + r * (2 * TAPS - 1) * 2, *xr = x + 2 * r * PITCH;
        CHECK(zr[0] == 1.0f && zr[1] == 0.0f && zr[2] == 0.0f && zr[3] == 0.0f && zr[4] == 0.0f && zr[5] == 0.0f);
        CHECK(zr[6] == xr[2 * (N - 1)] && zr[7] == xr[2 * (N - 1) + 1] && zr[8] == xr[2 * (N - 2)] && zr[9] == xr[2 * (N - 2) + 1]);
    }
    /* a fixed FIR: w = (1, 2 - i, -1) by set_state, the history empty */
    OK(hzsdr_equalizer_reset(f));
    OK(hzsdr_equalizer_get_state(f, fresh, WORDS));
    memset(z, 0, sizeof z);
    for (int r = 0; r < R; r++) {
        float *zr = z + r * (2 * TAPS - 1) * 2;
        CHECK(fresh[r * (2 * TAPS - 1) * 2] == 1.0f);
        zr[0] = 1.0f, zr[2] = 2.0f, zr[3] = -1.0f, zr[4] = -1.0f;
    }
    CHECK(hzsdr_equalizer_set_state(f, z, WORDS + 1) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_set_state(f, z, WORDS - 1) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_equalizer_set_state(f, z, WORDS));
    OK(hzsdr_equalizer_push(f, x, N, PITCH, NULL, a, OPITCH, NULL, 0));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            float re, im;
            fir(x + 2 * r * PITCH, i, &re, &im);
            CHECK(a[2 * (r * OPITCH + i)] == re && a[2 * (r * OPITCH + i) + 1] == im);
        }
    OK(hzsdr_equalizer_get_state(f, z2, WORDS));
    /* the same stream cut at 1, 0, 1 (shorter than the history), 255 and 257 symbols, the state carried into a second
     * object half way, the second half in place */
    OK(hzsdr_equalizer_create(ctx, HZSDR_FMT_C64, HZSDR_EQUALIZER_DD_QPSK, TAPS, 0, still, 0, R, &g));
    OK(hzsdr_equalizer_set_state(g, z, WORDS));
    const int cuts[] = {1, 0, 1, 255, 257, N - 514};
    int done = 0;
    for (int k = 0; k < 6; k++) {
        if (k == 3) {
            float carry[WORDS];
            OK(hzsdr_equalizer_get_state(g, carry, WORDS));
            OK(hzsdr_equalizer_reset(g));
            OK(hzsdr_equalizer_set_state(g, carry, WORDS));
        }
        OK(hzsdr_equalizer_push(g, x + 2 * done, (size_t)cuts[k], PITCH, NULL, b + 2 * done, OPITCH, NULL, 0));
        done += cuts[k];
    }
    CHECK(done == N && memcmp(a, b, sizeof(float) * 2 * R * OPITCH) == 0);
    float carry[WORDS];
    OK(hzsdr_equalizer_get_state(g, carry, WORDS));
    CHECK(memcmp(carry, z2, sizeof z2) == 0);
    /* in place, with counts: row 0 stops at 100 symbols, row 1 takes all (the count is clamped to n) */
    float *w = (float *)malloc(sizeof(float) * 2 * R * PITCH);
    memcpy(w, x, sizeof(float) * 2 * R * PITCH);
    uint32_t counts[R] = {100, N + 9};
    OK(hzsdr_equalizer_set_state(g, z, WORDS));
    OK(hzsdr_equalizer_push(g, w, N, PITCH, counts, w, PITCH, NULL, 0));
    CHECK(counts[0] == 100 && counts[1] == N + 9);
    CHECK(memcmp(w, a, sizeof(float) * 2 * 100) == 0 && memcmp(w + 2 * 100, x + 2 * 100, sizeof(float) * 2 * (PITCH - 100)) == 0);
    CHECK(memcmp(w + 2 * PITCH, a + 2 * OPITCH, sizeof(float) * 2 * N) == 0 && memcmp(w + 2 * (PITCH + N), x + 2 * (PITCH + N), sizeof(float) * 2 * (PITCH - N)) == 0);
    /* refused pushes change nothing */
    OK(hzsdr_equalizer_get_state(g, carry, WORDS));
    CHECK(hzsdr_equalizer_push(g, x, N, N - 1, NULL, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_push(g, x, N, PITCH, NULL, b, N - 1, NULL, 0) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_equalizer_push(g, x, N, PITCH, NULL, b, OPITCH, t, N - 1) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_equalizer_push(g, w, N, PITCH, NULL, w, PITCH - 1, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_push(g, NULL, N, PITCH, NULL, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_push(g, x, N, PITCH, NULL, NULL, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_push(NULL, x, N, PITCH, NULL, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_equalizer_set_params(g, fast) == HZSDR_ERR_INVALID_ARGUMENT && hzsdr_equalizer_set_params(g, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_equalizer_set_params(g, live));
    OK(hzsdr_equalizer_get_state(g, z2, WORDS));
    CHECK(memcmp(carry, z2, sizeof z2) == 0);
    OK(hzsdr_equalizer_free(g));
    OK(hzsdr_equalizer_free(f));
    /* one decision-directed update of a real row of two taps: w = (1, 0), history 0.25, x = 0.5, mu = 0.5, level 0.75:
     * y = 0.5, e = 0.25, g = 0.125: w = (1.0625, 0.03125), track 0.0625; per-row parameters, the second row held still */
    const float two[4] = {0.5f, 0.75f, 0.0f, 0.75f};
    float zr[6] = {1.0f, 0.0f, 0.25f, 1.0f, 0.0f, 0.25f}, xr[2] = {0.5f, 0.5f}, yr[2], tr[2];
    OK(hzsdr_equalizer_create(ctx, HZSDR_EQUALIZER_REAL_F32, HZSDR_EQUALIZER_DD_BPSK, 2, 0, two, 1, 2, &f));
    OK(hzsdr_equalizer_plan(f, &rows_per_wave, &tile, &form));
    CHECK(form == HZSDR_EQUALIZER_FORM_PER_ROW);
    OK(hzsdr_equalizer_set_state(f, zr, 6));
    OK(hzsdr_equalizer_push(f, xr, 1, 1, NULL, yr, 1, tr, 1));
    OK(hzsdr_equalizer_get_state(f, zr, 6));
    CHECK(yr[0] == 0.5f && yr[1] == 0.5f && tr[0] == 0.0625f && tr[1] == 0.0625f);
    CHECK(zr[0] == 1.0625f && zr[1] == 0.03125f && zr[2] == 0.5f && zr[3] == 1.0f && zr[4] == 0.0f && zr[5] == 0.5f);
    OK(hzsdr_equalizer_free(f));
    CHECK(hzsdr_equalizer_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    free(x), free(a), free(b), free(t), free(w);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("equalizer-abi ok\n");
    return 0;
}
