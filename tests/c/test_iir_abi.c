/* test_iir_abi.c -- the IIR bank (hzsdr_iir.h) exercised by a C compiler (gcc -std=c99) in a HOST context: a two-section
 * cascade over two pitched real rows against the definition evaluated here in double, samples cut anywhere writing the
 * bits one push writes, the state carried into a second object, a retune that keeps the state, a too-small destination
 * refused without a change of state, a complex row in place, a per-row bank equal to the shared one.
 * Prints "iir-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_iir.h"

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

enum { S = 2, N = 777, R = 2, PITCH = N + 5, OPITCH = N + 3 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* a DC blocker, then a resonant low-pass: b0 b1 b2 a1 a2 */
    const float sec[S * 5] = {1.0f, -1.0f, 0.0f, -0.95f, 0.0f, 0.02f, 0.04f, 0.02f, -1.56f, 0.64f};
    const float other[S * 5] = {1.0f, -1.0f, 0.0f, -0.90f, 0.0f, 0.05f, 0.10f, 0.05f, -1.20f, 0.40f};
    float *x = (float *)calloc((size_t)R * PITCH, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) x[r * PITCH + i] = (float)(0.5 + 0.4 * sin(0.05 * i * (r + 1)) + 0.1 * cos(1.3 * i + r));
    hzsdr_iir *f = NULL, *g = NULL, *bad = NULL;
    float nonfinite[S * 5];
    memcpy(nonfinite, sec, sizeof sec);
    nonfinite[7] = (float)INFINITY;
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, sec, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, sec, HZSDR_IIR_MAX_SECTIONS + 1, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, sec, S, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, sec, S, 0, HZSDR_IIR_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, NULL, S, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, nonfinite, S, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_iir_create(ctx, 9, sec, S, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    OK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, sec, S, 0, R, &f));
    size_t rows_per_wave = 0, tile = 0, got = 9;
    int form = -1;
    uint64_t pos = 9;
    OK(hzsdr_iir_plan(f, &rows_per_wave, &tile, &form));
    CHECK(rows_per_wave == 1 && tile == 256 && form == 0);
    float *a = (float *)malloc(sizeof(float) * R * OPITCH);
    memset(a, 0x7f, sizeof(float) * R * OPITCH);
    /* refused before anything runs: the position stays 0 */
    CHECK(hzsdr_iir_push(f, x, N, PITCH, a, N - 1, OPITCH, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    CHECK(hzsdr_iir_push(f, x, N, PITCH, a, OPITCH, N - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    CHECK(hzsdr_iir_push(f, x, N, N - 1, a, OPITCH, OPITCH, &got) == HZSDR_ERR_INVALID_ARGUMENT && got == 0);
    OK(hzsdr_iir_position(f, &pos));
    CHECK(pos == 0);
    OK(hzsdr_iir_push(f, x, N, PITCH, a, OPITCH, OPITCH, &got));
    CHECK(got == N);
    OK(hzsdr_iir_position(f, &pos));
    CHECK(pos == N);
    /* the definition in double, direct form I */
    for (int r = 0; r < R; r++) {
        double v[N], w[N];
        for (int i = 0; i < N; i++) v[i] = x[r * PITCH + i];
        for (int s = 0; s < S; s++) {
            const float *c = sec + 5 * s;
            for (int i = 0; i < N; i++)
                w[i] = c[0] * v[i] + (i > 0 ? c[1] * v[i - 1] - c[3] * w[i - 1] : 0.0) + (i > 1 ? c[2] * v[i - 2] - c[4] * w[i - 2] : 0.0);
            memcpy(v, w, sizeof v);
        }
        for (int i = 0; i < N; i++) CHECK(fabs(a[r * OPITCH + i] - v[i]) <= 2e-5);
        for (int k = N; k < OPITCH; k++) {
            uint32_t u;
            memcpy(&u, a + r * OPITCH + k, 4);
            CHECK(u == 0x7f7f7f7fu);
        }
    }
    /* the same samples in five pushes (one empty, one of a single sample), the state moved to a second object in the
     * middle */
    float *b = (float *)calloc((size_t)R * OPITCH, sizeof(float));
    float z[R * S * 2];
    const size_t cuts[6] = {0, 3, 3, 4, 611, N};
    OK(hzsdr_iir_reset(f));
    OK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, other, S, 0, R, &g));
    hzsdr_iir *cur = f;
    for (int i = 0; i < 5; i++) {
        OK(hzsdr_iir_push(cur, x + cuts[i], cuts[i + 1] - cuts[i], PITCH, b + cuts[i], OPITCH - cuts[i], OPITCH, &got));
        CHECK(got == cuts[i + 1] - cuts[i]);
        if (i == 3) {
            CHECK(hzsdr_iir_get_state(f, z, R * S * 2 - 1) == HZSDR_ERR_DST_TOO_SMALL);
            OK(hzsdr_iir_get_state(f, z, R * S * 2));
            OK(hzsdr_iir_position(f, &pos));
            CHECK(hzsdr_iir_set_state(g, z, R * S * 2 - 1, pos) == HZSDR_ERR_INVALID_ARGUMENT);
            OK(hzsdr_iir_set_state(g, z, R * S * 2, pos));
            CHECK(hzsdr_iir_set_sections(g, sec, S + 1) == HZSDR_ERR_INVALID_ARGUMENT);
            CHECK(hzsdr_iir_set_sections(g, nonfinite, S) == HZSDR_ERR_INVALID_ARGUMENT);
            OK(hzsdr_iir_set_sections(g, sec, S)); /* g was made with other coefficients: retuned, the state kept */
            cur = g;
        }
    }
    OK(hzsdr_iir_position(g, &pos));
    CHECK(pos == N);
    for (int r = 0; r < R; r++) CHECK(memcmp(a + r * OPITCH, b + r * OPITCH, sizeof(float) * N) == 0);
    OK(hzsdr_iir_free(g));
    /* one cascade per row with equal values: the shared form's bits */
    float both[R * S * 5];
    memcpy(both, sec, sizeof sec);
    memcpy(both + S * 5, sec, sizeof sec);
    OK(hzsdr_iir_create(ctx, HZSDR_IIR_REAL_F32, both, S, 1, R, &g));
    OK(hzsdr_iir_plan(g, NULL, NULL, &form));
    CHECK(form == HZSDR_IIR_FORM_PER_ROW);
    OK(hzsdr_iir_push(g, x, N, PITCH, b, OPITCH, OPITCH, &got));
    for (int r = 0; r < R; r++) CHECK(memcmp(a + r * OPITCH, b + r * OPITCH, sizeof(float) * N) == 0);
    OK(hzsdr_iir_free(g));
    OK(hzsdr_iir_free(f));
    /* a complex row, in place: re and im are two real runs of the same cascade */
    float *c = (float *)malloc(sizeof(float) * 2 * N);
    for (int i = 0; i < N; i++) {
        c[2 * i] = x[i];
        c[2 * i + 1] = x[PITCH + i];
    }
    OK(hzsdr_iir_create(ctx, HZSDR_FMT_C64, sec, S, 0, 1, &f));
    OK(hzsdr_iir_plan(f, NULL, NULL, &form));
    CHECK(form == HZSDR_IIR_FORM_COMPLEX);
    OK(hzsdr_iir_push(f, c, N, 0, c, N, 0, &got));
    CHECK(got == N);
    for (int i = 0; i < N; i++) CHECK(c[2 * i] == a[i] && c[2 * i + 1] == a[OPITCH + i]);
    OK(hzsdr_iir_free(f));
    free(x);
    free(a);
    free(b);
    free(c);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("iir-abi ok\n");
    return 0;
}
