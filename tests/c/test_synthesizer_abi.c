/* test_synthesizer_abi.c -- the polyphase synthesis bank (hzsdr_synthesizer.h) exercised by a C compiler
 * (gcc -std=c99) in a HOST context: two channels fed with constants come out as the two tones the definition gives,
 * frames cut anywhere write the bits one push writes, channel-major NegativeFirst input with a pitch equals
 * frame-major ZeroFirst input, a too-small destination is refused without a change of state, and the u8 destination
 * is the conversion of the complex64 one.  Prints "synthesizer-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_synthesizer.h"

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

enum { M = 256, P = 4, L = P * M, HOP = 192, FRAMES = 12, LEN = (FRAMES - 1) * HOP + L, HELD = L - HOP, K0 = M - 3, K1 = 5, PADC = 5 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    const double pi = 3.14159265358979323846;
    /* a Hann prototype whose hop-spaced copies sum to about 0.1; channel K0 carries 1, channel K1 carries -0.5i */
    float *g = (float *)malloc(sizeof(float) * L);
    for (int i = 0; i < L; i++) g[i] = (float)(0.1 * HOP * (1.0 - cos(2.0 * pi * (i + 0.5) / L)) / L);
    float *y = (float *)calloc((size_t)FRAMES * M * 2, sizeof(float));
    for (int f = 0; f < FRAMES; f++) {
        y[2 * (f * M + K0)] = 1.0f;
        y[2 * (f * M + K1) + 1] = -0.5f;
    }
    hzsdr_synthesizer *z = NULL, *n = NULL, *b8 = NULL, *bad = NULL;
    CHECK(hzsdr_synthesizer_create(ctx, HZSDR_FMT_C64, 100, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_synthesizer_create(ctx, HZSDR_FMT_C64, M, g, L, M + 1, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_synthesizer_create(ctx, 9, M, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    OK(hzsdr_synthesizer_create(ctx, HZSDR_FMT_C64, M, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &z));
    OK(hzsdr_synthesizer_create(ctx, HZSDR_FMT_C64, M, g, L, HOP, HZSDR_ORDER_NEGATIVE_FIRST, HZSDR_CHANNELIZER_CHANNEL_MAJOR, &n));
    OK(hzsdr_synthesizer_create(ctx, HZSDR_FMT_U8, M, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &b8));
    size_t got = 0, held = 0, group = 0;
    uint64_t next = 0;
    OK(hzsdr_synthesizer_group_frames(z, &group));
    CHECK(group >= 1);
    float *a = (float *)calloc((size_t)LEN * 2, sizeof(float));
    /* a destination one sample short: refused, nothing consumed */
    CHECK(hzsdr_synthesizer_push(z, y, FRAMES, 0, a, (size_t)FRAMES * HOP - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_synthesizer_pending(z, &held, &next));
    CHECK(held == 0 && next == 0);
    OK(hzsdr_synthesizer_push(z, y, FRAMES, 0, a, (size_t)FRAMES * HOP, &got));
    CHECK(got == (size_t)FRAMES * HOP);
    OK(hzsdr_synthesizer_pending(z, &held, &next));
    CHECK(held == HELD && next == FRAMES);
    CHECK(hzsdr_synthesizer_flush(z, a + 2 * FRAMES * HOP, HELD - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_synthesizer_pending(z, &held, &next));
    CHECK(held == HELD && next == FRAMES);
    OK(hzsdr_synthesizer_flush(z, a + 2 * FRAMES * HOP, HELD, &got));
    CHECK(got == HELD);
    OK(hzsdr_synthesizer_pending(z, &held, &next));
    CHECK(held == 0 && next == 0);
    /* the definition: x^[t] = c[t] * (exp(2 pi i K0 t / M) - 0.5i exp(2 pi i K1 t / M)), c[t] = sum_j g[t - jD] */
    for (int t = 0; t < LEN; t++) {
        double c = 0.0;
        for (int j = 0; j < FRAMES; j++)
            if (t - j * HOP >= 0 && t - j * HOP < L) c += (double)g[t - j * HOP];
        const double p0 = 2.0 * pi * (double)((K0 * t) % M) / M, p1 = 2.0 * pi * (double)((K1 * t) % M) / M;
        const double re = c * (cos(p0) + 0.5 * sin(p1)), im = c * (sin(p0) - 0.5 * cos(p1));
        CHECK(fabs(a[2 * t] - re) <= 1e-5 * c + 1e-12 && fabs(a[2 * t + 1] - im) <= 1e-5 * c + 1e-12);
    }
    /* the same frames in four pushes (one empty, one of a single frame), channel-major NegativeFirst with a pitch of
     * FRAMES + PADC: channel k's stream is row (k + M/2) mod M; the bits are those of the one push */
    const size_t stride = FRAMES + PADC;
    float *yc = (float *)calloc(2 * M * stride, sizeof(float));
    for (int k = 0; k < M; k++)
        for (int f = 0; f < FRAMES; f++) memcpy(yc + 2 * ((size_t)((k + M / 2) % M) * stride + f), y + 2 * (f * M + k), 2 * sizeof(float));
    float *b = (float *)calloc((size_t)LEN * 2, sizeof(float));
    /* a pitch below the frames of the push: refused */
    CHECK(hzsdr_synthesizer_push(n, yc, FRAMES, FRAMES - 1, b, LEN, &got) == HZSDR_ERR_INVALID_ARGUMENT && got == 0);
    const size_t cuts[5] = {0, 1, 1, 8, FRAMES};
    size_t done = 0;
    for (int i = 0; i < 4; i++) {
        size_t w = 0;
        OK(hzsdr_synthesizer_push(n, yc + 2 * cuts[i], cuts[i + 1] - cuts[i], stride, b + 2 * done, LEN - done, &w));
        CHECK(w == (cuts[i + 1] - cuts[i]) * HOP);
        done += w;
    }
    OK(hzsdr_synthesizer_flush(n, b + 2 * done, LEN - done, &got));
    CHECK(done + got == LEN);
    CHECK(memcmp(a, b, sizeof(float) * 2 * LEN) == 0);
    /* the u8 destination is hzsdr_convert of the complex64 stream */
    uint8_t *u = (uint8_t *)malloc(2 * LEN), *v = (uint8_t *)malloc(2 * LEN);
    OK(hzsdr_synthesizer_push(b8, y, FRAMES, 0, u, LEN, &got));
    OK(hzsdr_synthesizer_flush(b8, u + 2 * got, LEN - got, &done));
    CHECK(got + done == LEN);
    OK(hzsdr_convert(ctx, HZSDR_FMT_U8, v, LEN, HZSDR_FMT_C64, a, LEN, &got));
    CHECK(got == LEN && memcmp(u, v, 2 * LEN) == 0);
    /* reset mid-stream */
    OK(hzsdr_synthesizer_push(n, yc, 3, stride, b, LEN, &got));
    OK(hzsdr_synthesizer_reset(n));
    OK(hzsdr_synthesizer_pending(n, &held, &next));
    CHECK(held == 0 && next == 0);
    OK(hzsdr_synthesizer_free(z));
    OK(hzsdr_synthesizer_free(n));
    OK(hzsdr_synthesizer_free(b8));
    free(g);
    free(y);
    free(yc);
    free(a);
    free(b);
    free(u);
    free(v);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("synthesizer-abi ok\n");
    return 0;
}
