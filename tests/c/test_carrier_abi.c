/* test_carrier_abi.c -- the carrier recovery bank (hzsdr_carrier.h) exercised by a C compiler (gcc -std=c99) in a HOST
 * context: with the loop held still (no gains) and the frequency a quarter turn per sample, the oscillator stays on the
 * four axes, where it is exact: the outputs of two pitched rows are the samples times (-i)^n, the track is 0.25, the
 * columns behind the rows stay as they were; samples cut anywhere write what one push writes, the state carries into a
 * second object, in place equals out of place, a refused push changes nothing, new parameters keep theta and F, reset
 * restores F0, a per-row bank turns its rows either way.
 * Prints "carrier-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_carrier.h"

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

/* x * (-i)^n (dir = 1) or x * i^n (dir = -1), exactly */
static void turned(const float *x, int n, int dir, float *re, float *im) {
    const int q = ((n * dir) % 4 + 4) % 4;
    const float a = x[0], b = x[1];
    *re = q == 0 ? a : q == 1 ? b : q == 2 ? -a : -b;
    *im = q == 0 ? b : q == 1 ? -a : q == 2 ? -b : a;
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* alpha, beta, f0, fmin, fmax */
    const float still[5] = {0.0f, 0.0f, 0.25f, 0.25f, 0.25f};
    const float loop[5] = {0.01f, 0.0002f, 0.0f, -0.25f, 0.25f};
    const float nonfinite[5] = {0.0f, (float)INFINITY, 0.0f, 0.0f, 0.0f};
    const float strong[5] = {0.13f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float unordered[5] = {0.0f, 0.0f, 0.1f, 0.0f, 0.05f};
    float *x = (float *)calloc((size_t)R * PITCH * 2, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            x[(r * PITCH + i) * 2] = (float)(1 + (i * 7 + r * 3) % 23) * ((i + r) % 3 ? 1.0f : -1.0f);
            x[(r * PITCH + i) * 2 + 1] = (float)(2 + (i * 5 + r) % 19) * ((i + 2 * r) % 5 ? -1.0f : 1.0f);
        }
    hzsdr_carrier *f = NULL, *g = NULL, *bad = NULL;
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, still, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, still, 0, HZSDR_CARRIER_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, NULL, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, nonfinite, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, strong, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_TONE, unordered, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_create(ctx, 3, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT && bad == NULL);
    CHECK(hzsdr_carrier_create(ctx, -1, still, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT && bad == NULL);
    OK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_QPSK, still, 0, R, &f));
    size_t rows_per_wave = 0, tile = 0;
    int form = -1;
    uint64_t pos = 9;
    OK(hzsdr_carrier_plan(f, &rows_per_wave, &tile, &form));
    CHECK(rows_per_wave == 1 && tile == 256 && form == HZSDR_CARRIER_QPSK * HZSDR_CARRIER_FORM_MODE);
    float *a = (float *)malloc(sizeof(float) * 2 * R * OPITCH), *b = (float *)malloc(sizeof(float) * 2 * R * OPITCH);
    float *t = (float *)malloc(sizeof(float) * R * TPITCH);
    for (int i = 0; i < 2 * R * OPITCH; i++) a[i] = b[i] = -77.0f;
    for (int i = 0; i < R * TPITCH; i++) t[i] = -77.0f;
    OK(hzsdr_carrier_push(f, x, N, PITCH, a, OPITCH, t, TPITCH));
    OK(hzsdr_carrier_position(f, &pos));
    CHECK(pos == N);
    for (int r = 0; r < R; r++) {
        for (int i = 0; i < N; i++) {
            float re, im;
            turned(&x[(r * PITCH + i) * 2], i, 1, &re, &im);
            CHECK(a[(r * OPITCH + i) * 2] == re && a[(r * OPITCH + i) * 2 + 1] == im && t[r * TPITCH + i] == 0.25f);
        }
        for (int i = N; i < OPITCH; i++) CHECK(a[(r * OPITCH + i) * 2] == -77.0f && a[(r * OPITCH + i) * 2 + 1] == -77.0f);
        for (int i = N; i < TPITCH; i++) CHECK(t[r * TPITCH + i] == -77.0f);
    }
    uint32_t z[2 * R], z2[2 * R];
    CHECK(hzsdr_carrier_get_state(f, z, 2 * R - 1) == HZSDR_ERR_DST_TOO_SMALL);
    OK(hzsdr_carrier_get_state(f, z, 2 * R));
    for (int r = 0; r < R; r++) CHECK(z[2 * r] == (uint32_t)N << 30 && z[2 * r + 1] == 1u << 30);
    /* cut anywhere, the second part by a second object that takes the first one's state; no track this time */
    OK(hzsdr_carrier_reset(f));
    OK(hzsdr_carrier_position(f, &pos));
    OK(hzsdr_carrier_get_state(f, z2, 2 * R));
    CHECK(pos == 0 && z2[0] == 0 && z2[1] == 1u << 30 && z2[2] == 0 && z2[3] == 1u << 30);
    OK(hzsdr_carrier_push(f, x, 257, PITCH, b, OPITCH, NULL, 0));
    OK(hzsdr_carrier_push(f, x, 0, PITCH, b, OPITCH, NULL, 0));
    OK(hzsdr_carrier_get_state(f, z2, 2 * R));
    OK(hzsdr_carrier_position(f, &pos));
    OK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_QPSK, still, 0, R, &g));
    CHECK(hzsdr_carrier_set_state(g, z2, 2 * R + 1, pos) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_carrier_set_state(g, z2, 2 * R, pos));
    OK(hzsdr_carrier_push(g, x + 2 * 257, N - 257, PITCH, b + 2 * 257, OPITCH, NULL, 0));
    OK(hzsdr_carrier_position(g, &pos));
    OK(hzsdr_carrier_get_state(g, z2, 2 * R));
    CHECK(pos == N && memcmp(z, z2, sizeof z) == 0 && memcmp(a, b, sizeof(float) * 2 * R * OPITCH) == 0);
    /* refused pushes change nothing */
    CHECK(hzsdr_carrier_push(g, x, N, N - 1, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_push(g, x, N, PITCH, b, N - 1, NULL, 0) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_carrier_push(g, x, N, PITCH, b, OPITCH, t, N - 1) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_carrier_push(g, NULL, N, PITCH, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_push(g, x, N, PITCH, NULL, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_push(g, x, N, PITCH, x, PITCH - 1, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT); /* in place, two pitches */
    OK(hzsdr_carrier_get_state(g, z2, 2 * R));
    OK(hzsdr_carrier_position(g, &pos));
    CHECK(pos == N && memcmp(z, z2, sizeof z) == 0 && memcmp(a, b, sizeof(float) * 2 * R * OPITCH) == 0);
    /* new parameters keep theta and F; refused ones change nothing */
    CHECK(hzsdr_carrier_set_params(g, strong) == HZSDR_ERR_INVALID_ARGUMENT && hzsdr_carrier_set_params(g, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_carrier_set_params(g, loop));
    OK(hzsdr_carrier_get_state(g, z2, 2 * R));
    CHECK(memcmp(z, z2, sizeof z) == 0);
    OK(hzsdr_carrier_reset(g));
    OK(hzsdr_carrier_get_state(g, z2, 2 * R));
    CHECK(z2[0] == 0 && z2[1] == 0 && z2[2] == 0 && z2[3] == 0); /* F0 of the parameters in force */
    /* in place: the rows where they lie, the columns behind them as they were */
    float *w = (float *)malloc(sizeof(float) * 2 * R * PITCH);
    memcpy(w, x, sizeof(float) * 2 * R * PITCH);
    for (int r = 0; r < R; r++)
        for (int i = N; i < PITCH; i++) w[(r * PITCH + i) * 2] = w[(r * PITCH + i) * 2 + 1] = -55.0f;
    OK(hzsdr_carrier_reset(f));
    OK(hzsdr_carrier_push(f, w, N, PITCH, w, PITCH, NULL, 0));
    for (int r = 0; r < R; r++) {
        CHECK(memcmp(&w[r * PITCH * 2], &a[r * OPITCH * 2], sizeof(float) * 2 * N) == 0);
        for (int i = N; i < PITCH; i++) CHECK(w[(r * PITCH + i) * 2] == -55.0f && w[(r * PITCH + i) * 2 + 1] == -55.0f);
    }
    /* a set per row: the second row turns the other way */
    const float two[10] = {0.0f, 0.0f, 0.25f, 0.25f, 0.25f, 0.0f, 0.0f, -0.25f, -0.25f, -0.25f};
    hzsdr_carrier *p = NULL;
    OK(hzsdr_carrier_create(ctx, HZSDR_CARRIER_BPSK, two, 1, R, &p));
    OK(hzsdr_carrier_plan(p, NULL, NULL, &form));
    CHECK(form == HZSDR_CARRIER_FORM_PER_ROW + HZSDR_CARRIER_BPSK * HZSDR_CARRIER_FORM_MODE);
    OK(hzsdr_carrier_push(p, x, N, PITCH, b, OPITCH, t, TPITCH));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            float re, im;
            turned(&x[(r * PITCH + i) * 2], i, r ? -1 : 1, &re, &im);
            CHECK(b[(r * OPITCH + i) * 2] == re && b[(r * OPITCH + i) * 2 + 1] == im && t[r * TPITCH + i] == (r ? -0.25f : 0.25f));
        }
    CHECK(hzsdr_carrier_push(NULL, x, N, PITCH, b, OPITCH, NULL, 0) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_carrier_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_carrier_free(p));
    OK(hzsdr_carrier_free(g));
    OK(hzsdr_carrier_free(f));
    free(w), free(t), free(b), free(a), free(x);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("carrier-abi ok\n");
    return 0;
}
