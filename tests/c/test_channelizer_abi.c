/* test_channelizer_abi.c -- the polyphase channelizer (hzsdr_channelizer.h) exercised by a C compiler (gcc -std=c99)
 * in a HOST context: a tone between two channel centres lands in its channel in both orders and layouts, a stream cut
 * anywhere writes the bits one push writes, a too-small destination is refused without a change of state, and the
 * channel-major columns past the frames written stay as they were.  Prints "channelizer-abi ok" and exits 0. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_channelizer.h"

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

enum { M = 256, P = 4, L = P * M, HOP = 192, FRAMES = 12, LEN = (FRAMES - 1) * HOP + L + 50, K0 = M - 3, PADC = 5 };

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    const double pi = 3.14159265358979323846;
    /* a tone at (K0 + 0.1) fs / M and a Hann prototype of DC gain 1 */
    float *x = (float *)malloc(sizeof(float) * 2 * LEN);
    for (int t = 0; t < LEN; t++) {
        const double ph = 2.0 * pi * fmod((K0 + 0.1) * (double)t, (double)M) / M;
        x[2 * t] = (float)cos(ph);
        x[2 * t + 1] = (float)sin(ph);
    }
    float *g = (float *)malloc(sizeof(float) * L);
    for (int i = 0; i < L; i++) g[i] = (float)((1.0 - cos(2.0 * pi * (i + 0.5) / L)) / L);
    hzsdr_channelizer *z = NULL, *n = NULL, *bad = NULL;
    CHECK(hzsdr_channelizer_create(ctx, HZSDR_FMT_C64, 100, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_channelizer_create(ctx, HZSDR_FMT_C64, M, g, L, M + 1, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_channelizer_create(ctx, HZSDR_FMT_C64, M, g, L, HOP, HZSDR_ORDER_ZERO_FIRST, HZSDR_CHANNELIZER_FRAME_MAJOR, &z));
    OK(hzsdr_channelizer_create(ctx, HZSDR_FMT_C64, M, g, L, HOP, HZSDR_ORDER_NEGATIVE_FIRST, HZSDR_CHANNELIZER_CHANNEL_MAJOR, &n));
    size_t frames = 0, got = 0, held = 0;
    uint64_t next = 0;
    OK(hzsdr_channelizer_frames_for(z, LEN, &frames));
    CHECK(frames == FRAMES);
    float *a = (float *)calloc((size_t)FRAMES * M * 2, sizeof(float));
    /* a destination of FRAMES - 1 rows: refused, nothing consumed */
    CHECK(hzsdr_channelizer_push(z, x, LEN, a, FRAMES - 1, 0, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    OK(hzsdr_channelizer_pending(z, &held, &next));
    CHECK(held == 0 && next == 0);
    /* a push above 2^62 samples: refused before a count is formed, by push and by frames_for alike */
    CHECK(hzsdr_channelizer_push(z, x, ((size_t)1 << 62) + 1, a, FRAMES, 0, &got) == HZSDR_ERR_INVALID_ARGUMENT && got == 0);
    CHECK(hzsdr_channelizer_frames_for(z, ((size_t)1 << 62) + 1, &frames) == HZSDR_ERR_INVALID_ARGUMENT);
    OK(hzsdr_channelizer_push(z, x, LEN, a, FRAMES, 0, &got));
    CHECK(got == FRAMES);
    OK(hzsdr_channelizer_pending(z, &held, &next));
    CHECK(held == LEN - (size_t)FRAMES * HOP && next == FRAMES);
    /* the tone peaks in channel K0 of every frame; its phase advances by 2 pi 0.1 HOP / M per frame */
    for (int f = 0; f < FRAMES; f++) {
        int best = 0;
        for (int k = 1; k < M; k++)
            if (hypotf(a[2 * (f * M + k)], a[2 * (f * M + k) + 1]) > hypotf(a[2 * (f * M + best)], a[2 * (f * M + best) + 1])) best = k;
        CHECK(best == K0);
        if (f) {
            const float *u = a + 2 * ((f - 1) * M + K0), *v = a + 2 * (f * M + K0);
            const double d = atan2(v[1] * u[0] - v[0] * u[1], v[0] * u[0] + v[1] * u[1]);
            CHECK(fabs(d - 2.0 * pi * 0.1 * HOP / M) < 1e-4);
        }
    }
    /* the same stream in four pushes (one empty, one shorter than the hop), channel-major NegativeFirst with a
     * pitch of FRAMES + PADC: channel k's stream is row (k + M/2) mod M; the bits are those of the one push */
    const size_t stride = FRAMES + PADC;
    float *b = (float *)malloc(sizeof(float) * 2 * M * stride);
    for (size_t i = 0; i < 2 * M * stride; i++) b[i] = -7.0f;
    /* a pitch below the frames of the push: refused */
    CHECK(hzsdr_channelizer_push(n, x, LEN, b, FRAMES, FRAMES - 1, &got) == HZSDR_ERR_DST_TOO_SMALL && got == 0);
    const size_t cuts[5] = {0, 100, 100, 100 + L + 3 * HOP, LEN};
    size_t done = 0;
    for (int i = 0; i < 4; i++) {
        size_t w = 0, want = 0;
        OK(hzsdr_channelizer_frames_for(n, cuts[i + 1] - cuts[i], &want));
        OK(hzsdr_channelizer_push(n, x + 2 * cuts[i], cuts[i + 1] - cuts[i], b + 2 * done, stride - done, stride, &w));
        CHECK(w == want);
        done += w;
    }
    CHECK(done == FRAMES);
    for (int k = 0; k < M; k++) {
        const size_t row = (size_t)((k + M / 2) % M);
        for (int f = 0; f < FRAMES; f++) CHECK(memcmp(b + 2 * (row * stride + f), a + 2 * (f * M + k), 2 * sizeof(float)) == 0);
        for (size_t f = FRAMES; f < stride; f++) CHECK(b[2 * (row * stride + f)] == -7.0f && b[2 * (row * stride + f) + 1] == -7.0f);
    }
    OK(hzsdr_channelizer_reset(n));
    OK(hzsdr_channelizer_pending(n, &held, &next));
    CHECK(held == 0 && next == 0);
    OK(hzsdr_channelizer_free(z));
    OK(hzsdr_channelizer_free(n));
    free(x);
    free(g);
    free(a);
    free(b);
    OK(hzsdr_close(ctx));
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("channelizer-abi ok\n");
    return 0;
}
