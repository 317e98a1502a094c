/* test_agc_abi.c -- the AGC bank (hzsdr_agc.h) exercised by a C compiler (gcc -std=c99) in a HOST context: with the loop
 * held still (no rates) the outputs of two pitched complex rows are the samples times g0 = 0.5, exactly, the track is
 * 0.5 and the columns behind the rows stay as they were; samples cut anywhere write what one push writes, the state
 * carries into a second object, in place equals out of place, a refused push changes nothing, new parameters keep the
 * gain, reset restores g0, a per-row bank gives its rows gains of their own; a live loop over real rows at the constant
 * level 4 halves its gain twice and stays at 0.25 exactly, whatever the signs.
 * Prints "agc-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_agc.h"

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

enum { N = 778, R = 2, PITCH = N + 5, OPITCH = N + 3, TPITCH = N + 2 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* ref, attack, decay, floor, g0, gmin, gmax */
    const float still[7] = {1.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.25f, 4.0f};
    const float live[7] = {1.0f, 0.5f, 0.5f, 0.0f, 1.0f, 0.125f, 8.0f};
    const float nonfinite[7] = {1.0f, (float)INFINITY, 0.0f, 0.0f, 1.0f, 0.5f, 2.0f};
    const float fast[7] = {1.0f, 0.6f, 0.0f, 0.0f, 1.0f, 0.5f, 2.0f};
    const float unordered[7] = {1.0f, 0.1f, 0.1f, 0.0f, 0.25f, 0.5f, 2.0f};
    float *x = (float *)calloc((size_t)R * PITCH * 2, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            x[(r * PITCH + i) * 2] = (float)(1 + (i * 7 + r * 3) % 23) * ((i + r) % 3 ? 1.0f : -1.0f);
            x[(r * PITCH + i) * 2 + 1] = (float)(2 + (i * 5 + r) % 19) * ((i + 2 * r) % 5 ? -1.0f : 1.0f);
        }
    hzsdr_agc *f = NULL, *g = NULL, *bad = NULL;
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, still, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, still, 0, HZSDR_AGC_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, NULL, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, nonfinite, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, fast, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, unordered, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_create(ctx, HZSDR_FMT_U8, still, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    CHECK(hzsdr_agc_create(ctx, -1, still, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    OK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, still, 0, R, &f));
    size_t rows_per_wave = 0, tile = 0;
    int form = -1;
    uint64_t pos = 9;
    OK(hzsdr_agc_plan(f, &rows_per_wave, &tile, &form));
    CHECK(rows_per_wave == 1 && tile == 256 && form == HZSDR_AGC_FORM_COMPLEX);
    float *a = (float *)malloc(sizeof(float) * 2 * R * OPITCH), *b = (float *)malloc(sizeof(float) * 2 * R * OPITCH);
    float *t = (float *)malloc(sizeof(float) * R * TPITCH);
    for (int i = 0; i < 2 * R * OPITCH; i++) a[i] = b[i] = -77.0f;
    for (int i = 0; i < R * TPITCH; i++) t[i] = -77.0f;
    OK(hzsdr_agc_push(f, x, N, PITCH, a, OPITCH, t, TPITCH));
    OK(hzsdr_agc_position(f, &pos));
    CHECK(pos == N);
    for (int r = 0; r < R; r++) {
        for (int i = 0; i < N; i++)
            CHECK(a[(r * OPITCH + i) * 2] == 0.5f * x[(r * PITCH + i) * 2] && a[(r * OPITCH + i) * 2 + 1] == 0.5f * x[(r * PITCH + i) * 2 + 1] &&
                  t[r * TPITCH + i] == 0.5f);
        for (int i = N; i < OPITCH; i++) CHECK(a[(r * OPITCH + i) * 2] == -77.0f && a[(r * OPITCH + i) * 2 + 1] == -77.0f);
        for (int i = N; i < TPITCH; i++) CHECK(t[r * TPITCH + i] == -77.0f);
    }
    float z[R], z2[R];
    CHECK(hzsdr_agc_get_state(f, z, R - 1) == HZSDR_ERR_DST_TOO_SMALL);
    OK(hzsdr_agc_get_state(f, z, R));
    for (int r = 0; r < R; r++) CHECK(z[r] == 0.5f);
    /* cut anywhere, the second part by a second object that takes the first one's state; no track this time */
    OK(hzsdr_agc_reset(f));
    OK(hzsdr_agc_position(f, &pos));
    CHECK(pos == 0);
    OK(hzsdr_agc_push(f, x, 257, PITCH, b, OPITCH, NULL, 0));
    OK(hzsdr_agc_push(f, x, 0, PITCH, b, OPITCH, NULL, 0));
    OK(hzsdr_agc_get_state(f, z2, R));
    OK(hzsdr_agc_position(f, &pos));
    OK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, still, 0, R, &g));
    CHECK(hzsdr_agc_set_state(g, z2, R + 1, pos) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_agc_set_state(g, z2, R, pos));
    OK(hzsdr_agc_push(g, x + 2 * 257, N - 257, PITCH, b + 2 * 257, OPITCH, NULL, 0));
    OK(hzsdr_agc_position(g, &pos));
    OK(hzsdr_agc_get_state(g, z2, R));
    CHECK(pos == N && memcmp(z, z2, sizeof z) == 0 && memcmp(a, b, sizeof(float) * 2 * R * OPITCH) == 0);
    /* refused pushes change nothing */
    CHECK(hzsdr_agc_push(g, x, N, N - 1, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_push(g, x, N, PITCH, b, N - 1, NULL, 0) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_agc_push(g, x, N, PITCH, b, OPITCH, t, N - 1) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_agc_push(g, NULL, N, PITCH, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_push(g, x, N, PITCH, NULL, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_push(g, x, N, PITCH, x, PITCH - 1, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT); /* in place, two pitches */
    OK(hzsdr_agc_get_state(g, z2, R));
    OK(hzsdr_agc_position(g, &pos));
    CHECK(pos == N && memcmp(z, z2, sizeof z) == 0 && memcmp(a, b, sizeof(float) * 2 * R * OPITCH) == 0);
    /* new parameters keep the gain; refused ones change nothing; reset restores g0 of the parameters in force */
    CHECK(hzsdr_agc_set_params(g, fast) == HZSDR_ERR_INVALID_ARGUMENT && hzsdr_agc_set_params(g, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_agc_set_params(g, live));
    OK(hzsdr_agc_get_state(g, z2, R));
    CHECK(memcmp(z, z2, sizeof z) == 0);
    OK(hzsdr_agc_reset(g));
    OK(hzsdr_agc_get_state(g, z2, R));
    CHECK(z2[0] == 1.0f && z2[1] == 1.0f);
    /* in place: the rows where they lie, the columns behind them as they were */
    float *w = (float *)malloc(sizeof(float) * 2 * R * PITCH);
    memcpy(w, x, sizeof(float) * 2 * R * PITCH);
    for (int r = 0; r < R; r++)
        for (int i = N; i < PITCH; i++) w[(r * PITCH + i) * 2] = w[(r * PITCH + i) * 2 + 1] = -55.0f;
    OK(hzsdr_agc_reset(f));
    OK(hzsdr_agc_push(f, w, N, PITCH, w, PITCH, NULL, 0));
    for (int r = 0; r < R; r++) {
        CHECK(memcmp(&w[r * PITCH * 2], &a[r * OPITCH * 2], sizeof(float) * 2 * N) == 0);
        for (int i = N; i < PITCH; i++) CHECK(w[(r * PITCH + i) * 2] == -55.0f && w[(r * PITCH + i) * 2 + 1] == -55.0f);
    }
    /* a set per row: the second row's gain is 2 */
    const float two[14] = {1.0f, 0.0f, 0.0f, 0.0f, 0.5f, 0.25f, 4.0f, 1.0f, 0.0f, 0.0f, 0.0f, 2.0f, 0.25f, 4.0f};
    hzsdr_agc *p = NULL;
    OK(hzsdr_agc_create(ctx, HZSDR_FMT_C64, two, 1, R, &p));
    OK(hzsdr_agc_plan(p, NULL, NULL, &form));
    CHECK(form == HZSDR_AGC_FORM_PER_ROW + HZSDR_AGC_FORM_COMPLEX);
    OK(hzsdr_agc_push(p, x, N, PITCH, b, OPITCH, t, TPITCH));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            const float g0 = r ? 2.0f : 0.5f;
            CHECK(b[(r * OPITCH + i) * 2] == g0 * x[(r * PITCH + i) * 2] && b[(r * OPITCH + i) * 2 + 1] == g0 * x[(r * PITCH + i) * 2 + 1] &&
                  t[r * TPITCH + i] == g0);
        }
    /* a live loop over real rows at the level 4: e = -3 clipped to -1, g = 0.5; e = -1, g = 0.25; e = 0 from then on */
    hzsdr_agc *q = NULL;
    float *xr = (float *)malloc(sizeof(float) * R * PITCH), *yr = (float *)malloc(sizeof(float) * R * OPITCH);
    for (int r = 0; r < R; r++)
        for (int i = 0; i < PITCH; i++) xr[r * PITCH + i] = (i * 3 + r) % 5 < 2 ? -4.0f : 4.0f;
    OK(hzsdr_agc_create(ctx, HZSDR_AGC_REAL_F32, live, 0, R, &q));
    OK(hzsdr_agc_plan(q, NULL, NULL, &form));
    CHECK(form == 0);
    OK(hzsdr_agc_push(q, xr, N, PITCH, yr, OPITCH, t, TPITCH));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            const float gain = i == 0 ? 1.0f : i == 1 ? 0.5f : 0.25f;
            CHECK(t[r * TPITCH + i] == gain && yr[r * OPITCH + i] == gain * xr[r * PITCH + i]);
        }
    OK(hzsdr_agc_get_state(q, z2, R));
    CHECK(z2[0] == 0.25f && z2[1] == 0.25f);
    CHECK(hzsdr_agc_push(NULL, x, N, PITCH, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_agc_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_agc_free(q));
    OK(hzsdr_agc_free(p));
    OK(hzsdr_agc_free(g));
    OK(hzsdr_agc_free(f));
    free(yr), free(xr), free(w), free(t), free(b), free(a), free(x);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("agc-abi ok\n");
    return 0;
}
