/* test_symsync_abi.c -- the symbol-timing recovery bank (hzsdr_symsync.h) exercised by a C compiler (gcc -std=c99) in a
 * HOST context: with the loop held still (no gains, no range) and 4 samples per symbol, the symbols of two pitched real
 * rows are samples read out, the columns behind a row's count stay as they were, samples cut anywhere write the symbols
 * one push writes, the state carries into a second object, a capacity below the bound is refused without a change of
 * state, new parameters keep the state, a per-row bank with two clocks writes two counts, a complex row is two real ones.
 * Prints "symsync-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_symsync.h"

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

enum { N = 778, R = 2, PITCH = N + 5, SYMS = N / 4 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* sps, limit, g_mu, g_omega */
    const float still[4] = {4.0f, 0.0f, 0.0f, 0.0f};
    const float loop[4] = {4.0f, 0.01f, 0.09f, 0.0013f};
    const float nonfinite[4] = {4.0f, 0.0f, (float)INFINITY, 0.0f};
    const float crowded[4] = {2.25f, 0.0f, 0.13f, 0.0f}; /* hmin - g_mu = 0.995: two strobes could share a sample */
    float *x = (float *)calloc((size_t)R * PITCH, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) x[r * PITCH + i] = (float)(1 + (i * 7 + r * 3) % 23) * ((i + r) % 3 ? 1.0f : -1.0f);
    hzsdr_symsync *f = NULL, *g = NULL, *bad = NULL;
    CHECK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, still, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, still, 0, HZSDR_SYMSYNC_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, NULL, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, nonfinite, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, crowded, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_symsync_create(ctx, HZSDR_FMT_U8, still, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    CHECK(hzsdr_symsync_create(ctx, 9, still, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && bad == NULL);
    OK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, still, 0, R, &f));
    size_t rows_per_wave = 0, tile = 0, bound = 0, most = 9;
    int form = -1;
    uint64_t pos = 9;
    OK(hzsdr_symsync_plan(f, &rows_per_wave, &tile, &form));
    CHECK(rows_per_wave == 1 && tile == 256 && form == 0);
    OK(hzsdr_symsync_max_symbols(f, N, &bound));
    CHECK(bound == N / 4 + 2); /* amin = 2: floor(N / 4) + 2 */
    OK(hzsdr_symsync_max_symbols(f, 0, &bound));
    CHECK(bound == 0);
    OK(hzsdr_symsync_max_symbols(f, N, &bound));
    const size_t opitch = bound + 3;
    float *a = (float *)malloc(sizeof(float) * R * opitch);
    memset(a, 0x7f, sizeof(float) * R * opitch);
    uint32_t counts[R] = {77, 77};
    /* refused before anything runs: the position stays 0 */
    CHECK(hzsdr_symsync_push(f, x, N, PITCH, a, bound - 1, opitch, counts, &most) == HZSDR_ERR_DST_TOO_SMALL && most == 0);
    CHECK(hzsdr_symsync_push(f, x, N, PITCH, a, opitch, bound - 1, counts, &most) == HZSDR_ERR_DST_TOO_SMALL && most == 0);
    CHECK(hzsdr_symsync_push(f, x, N, N - 1, a, opitch, opitch, counts, &most) == HZSDR_ERR_INVALID_ARGUMENT && most == 0);
    CHECK(hzsdr_symsync_push(f, x, N, PITCH, a, opitch, opitch, NULL, &most) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_symsync_position(f, &pos));
    CHECK(pos == 0 && counts[0] == 77);
    OK(hzsdr_symsync_push(f, x, N, PITCH, a, opitch, opitch, counts, &most));
    OK(hzsdr_symsync_position(f, &pos));
    CHECK(pos == N && most == SYMS && counts[0] == SYMS && counts[1] == SYMS);
    /* the loop held still at 4 samples per symbol: symbol k is sample 4 k of its row; behind the count, nothing */
    for (int r = 0; r < R; r++) {
        for (int k = 0; k < SYMS; k++) CHECK(a[r * opitch + k] == x[r * PITCH + 4 * k]);
        for (size_t k = SYMS; k < opitch; k++) {
            uint32_t u;
            memcpy(&u, a + r * opitch + k, 4);
            CHECK(u == 0x7f7f7f7fu);
        }
    }
    /* the same samples in five pushes (one empty, one of a single sample), the state moved to a second object in the
     * middle, which was made with other parameters and is given these */
    float *b = (float *)calloc((size_t)R * opitch, sizeof(float));
    float z[R * 8];
    const size_t cuts[6] = {0, 3, 3, 4, 611, N};
    size_t done[R] = {0, 0};
    OK(hzsdr_symsync_reset(f));
    OK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, loop, 0, R, &g));
    hzsdr_symsync *cur = f;
    for (int i = 0; i < 5; i++) {
        const size_t n = cuts[i + 1] - cuts[i];
        size_t cap = 0;
        uint32_t c[R] = {5, 5};
        float *part = (float *)malloc(sizeof(float) * R * (N / 2 + 2));
        OK(hzsdr_symsync_max_symbols(cur, n, &cap));
        OK(hzsdr_symsync_push(cur, x + cuts[i], n, PITCH, part, cap, cap, c, NULL));
        for (int r = 0; r < R; r++) {
            CHECK(c[r] <= cap);
            memcpy(b + r * opitch + done[r], part + r * cap, sizeof(float) * c[r]);
            done[r] += c[r];
        }
        free(part);
        if (i == 3) {
            CHECK(hzsdr_symsync_get_state(f, z, R * 8 - 1) == HZSDR_ERR_DST_TOO_SMALL);
            OK(hzsdr_symsync_get_state(f, z, R * 8));
            CHECK(z[1] == 2.0f && z[8 + 1] == 2.0f); /* h = sps / 2 */
            OK(hzsdr_symsync_position(f, &pos));
            CHECK(hzsdr_symsync_set_state(g, z, R * 8 - 1, pos) == HZSDR_ERR_INVALID_ARGUMENT);
            OK(hzsdr_symsync_set_state(g, z, R * 8, pos));
            CHECK(hzsdr_symsync_set_params(g, nonfinite) == HZSDR_ERR_INVALID_ARGUMENT);
            CHECK(hzsdr_symsync_set_params(g, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
            OK(hzsdr_symsync_set_params(g, still));
            cur = g;
        }
    }
    OK(hzsdr_symsync_position(g, &pos));
    CHECK(pos == N);
    for (int r = 0; r < R; r++) CHECK(done[r] == SYMS && memcmp(a + r * opitch, b + r * opitch, sizeof(float) * SYMS) == 0);
    OK(hzsdr_symsync_free(g));
    /* one set per row: 4 and 8 samples per symbol give SYMS and about half as many */
    const float both[R * 4] = {4.0f, 0.0f, 0.0f, 0.0f, 8.0f, 0.0f, 0.0f, 0.0f};
    OK(hzsdr_symsync_create(ctx, HZSDR_SYMSYNC_REAL_F32, both, 1, R, &g));
    OK(hzsdr_symsync_plan(g, NULL, NULL, &form));
    CHECK(form == HZSDR_SYMSYNC_FORM_PER_ROW);
    OK(hzsdr_symsync_push(g, x, N, PITCH, b, opitch, opitch, counts, &most));
    CHECK(counts[0] == SYMS && counts[1] == (N - 1 - 4) / 8 + 1 && most == SYMS); /* symbol k is found at sample 8 k + 4 */
    CHECK(memcmp(a, b, sizeof(float) * SYMS) == 0);
    for (uint32_t k = 0; k < counts[1]; k++) CHECK(b[opitch + k] == x[PITCH + 8 * k + 2]);
    OK(hzsdr_symsync_free(g));
    OK(hzsdr_symsync_free(f));
    /* a complex row: with the loop held still re and im are two real runs */
    float *c = (float *)malloc(sizeof(float) * 2 * N), *d = (float *)malloc(sizeof(float) * 2 * (N / 2 + 2));
    for (int i = 0; i < N; i++) {
        c[2 * i] = x[i];
        c[2 * i + 1] = x[PITCH + i];
    }
    OK(hzsdr_symsync_create(ctx, HZSDR_FMT_C64, still, 0, 1, &f));
    OK(hzsdr_symsync_plan(f, NULL, NULL, &form));
    CHECK(form == HZSDR_SYMSYNC_FORM_COMPLEX);
    OK(hzsdr_symsync_push(f, c, N, 0, d, bound, 0, counts, &most));
    CHECK(most == SYMS && counts[0] == SYMS);
    for (int k = 0; k < SYMS; k++) CHECK(d[2 * k] == a[k] && d[2 * k + 1] == a[opitch + k]);
    OK(hzsdr_symsync_free(f));
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
    printf("symsync-abi ok\n");
    return 0;
}
