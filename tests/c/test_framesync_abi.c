/* test_framesync_abi.c -- the frame sync bank (hzsdr_framesync.h) exercised by a C compiler (gcc -std=c99) in a HOST
 * context: two pitched real rows that carry the text "hello, frame" behind a 16-bit word, the second row inverted, read
 * back as the bytes written with their positions, distances and hypotheses; the slots behind a row's count and the
 * columns behind cap frames stay as they were; the stream cut anywhere finds what one push finds, each frame in the push
 * that delivers its last bit; the state carries into a second object; in_counts are obeyed and clamped; a refused push
 * changes nothing; reset starts over; configurations out of bounds are refused.
 * Prints "framesync-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_framesync.h"

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

enum { N = 400, R = 2, PITCH = N + 5, W = 16, P = 96, FB = 12, CAP = 3, OPITCH = CAP * FB + 7, AT = 150, HB = (W + P - 1 + 7) / 8 };
static const char text[FB + 1] = "hello, frame";

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    const uint64_t words[2] = {0xEB90u, 0x146Fu};
    const unsigned maps[2] = {0, 1}, maps_bad[2] = {0, 2};
    /* the rows: zeros but for the word at bit AT and the text behind it; row 1 inverted; magnitudes that vary */
    float *x = (float *)calloc((size_t)R * PITCH, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            int bit = 0;
            if (i >= AT && i < AT + W) bit = (int)((words[0] >> (W - 1 - (i - AT))) & 1u);
            if (i >= AT + W && i < AT + W + P) bit = (text[(i - AT - W) / 8] >> (7 - (i - AT - W) % 8)) & 1;
            x[r * PITCH + i] = (float)(1 + i % 7) * ((bit ^ r) ? 0.5f : -0.5f);
        }
    hzsdr_framesync *f = NULL, *g = NULL, *bad = NULL;
    const uint64_t mask = 0xFFFFu;
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, P, 0, 50, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, P, 0, 50, HZSDR_FRAMESYNC_MAX_ROWS + 1, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, 7, 1, W, mask, 1, 2, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 2, W, mask, 1, 2, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, 65, mask, 1, 2, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 16, 2, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, 0x1FFFFu, 1, 2, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 5, words, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps_bad, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, 8200, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, P, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, NULL, maps, P, 0, 50, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(bad == NULL);
    OK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, P, 0, 50, R, &f));
    OK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, mask, 1, 2, words, maps, P, 0, 50, R, &g));
    size_t rpw = 0, tile = 0, ring = 0;
    int form = -1;
    OK(hzsdr_framesync_plan(f, &rpw, &tile, &ring, &form));
    CHECK(rpw == 1 && tile == 64 && ring == 32 && form == 0);

    uint8_t out[R * OPITCH], one[R * OPITCH];
    uint64_t pos[R * CAP], pos1[R * CAP], where[R], holds[R];
    uint32_t info[R * CAP], info1[R * CAP], counts[R];
    uint8_t hist[R * HB], last[R], hist1[R * HB], last1[R];
    size_t most = 99;
    memset(one, 0xA5, sizeof one), memset(pos1, 0xA5, sizeof pos1), memset(info1, 0xA5, sizeof info1);
    OK(hzsdr_framesync_push(f, x, N, PITCH, NULL, one, CAP, OPITCH, pos1, info1, counts, &most));
    CHECK(most == 1 && counts[0] == 1 && counts[1] == 1);
    for (int r = 0; r < R; r++) {
        CHECK(memcmp(one + r * OPITCH, text, FB) == 0);
        CHECK(pos1[r * CAP] == AT + W && info1[r * CAP] == (uint32_t)(r << 8));
        for (int i = FB; i < OPITCH; i++) CHECK(one[r * OPITCH + i] == 0xA5);
        CHECK(pos1[r * CAP + 1] == 0xA5A5A5A5A5A5A5A5ull && info1[r * CAP + 2] == 0xA5A5A5A5u);
    }
    OK(hzsdr_framesync_positions(f, where, R));
    OK(hzsdr_framesync_get_state(f, where, holds, hist1, last1, R));
    CHECK(where[0] == N && where[1] == N && holds[0] == AT + W + 50 && holds[1] == holds[0]);
    CHECK(hzsdr_framesync_get_state(f, where, holds, hist1, last1, R - 1) == HZSDR_ERR_DST_TOO_SMALL);

    /* every cut: the frame comes with the push that delivers bit AT + W + P - 1; the state equals the one push's */
    for (int cut = 0; cut <= N; cut += (cut > 140 && cut < 270) ? 1 : 37) {
        OK(hzsdr_framesync_reset(f));
        memset(out, 0xA5, sizeof out);
        OK(hzsdr_framesync_push(f, x, (size_t)cut, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL));
        const int first = cut >= AT + W + P;
        CHECK(counts[0] == (uint32_t)first && counts[1] == (uint32_t)first);
        if (!first) CHECK(out[0] == 0xA5 && out[OPITCH] == 0xA5);
        /* the second half from the second object, which takes the first one's state */
        OK(hzsdr_framesync_get_state(f, where, holds, hist, last, R));
        CHECK(where[0] == (uint64_t)cut);
        OK(hzsdr_framesync_set_state(g, where, holds, hist, last, R));
        OK(hzsdr_framesync_push(g, x + cut, (size_t)(N - cut), PITCH, NULL, first ? out + FB : out, CAP - 1, OPITCH, pos + 1, info + 1, counts, &most));
        CHECK(counts[0] == (uint32_t)!first && most == (size_t)!first);
        if (!first) CHECK(memcmp(out, text, FB) == 0 && memcmp(out + OPITCH, text, FB) == 0 && pos[1] == AT + W && info[1 + (CAP - 1)] == 256);
        OK(hzsdr_framesync_get_state(g, where, holds, hist, last, R));
        CHECK(where[1] == N && holds[1] == AT + W + 50 && memcmp(hist, hist1, sizeof hist) == 0 && memcmp(last, last1, sizeof last) == 0);
    }

    /* in_counts: row 0 takes all, row 1 nothing; then row 1 takes a count above n, clamped */
    OK(hzsdr_framesync_reset(f));
    uint32_t ic[R] = {N, 0};
    OK(hzsdr_framesync_push(f, x, N, PITCH, ic, out, CAP, OPITCH, pos, info, counts, &most));
    CHECK(counts[0] == 1 && counts[1] == 0 && most == 1);
    OK(hzsdr_framesync_positions(f, where, R));
    CHECK(where[0] == N && where[1] == 0);
    ic[0] = 0, ic[1] = 0xFFFFFFFFu;
    OK(hzsdr_framesync_push(f, x, N, PITCH, ic, out, CAP, OPITCH, pos, info, counts, NULL));
    CHECK(counts[0] == 0 && counts[1] == 1);
    OK(hzsdr_framesync_positions(f, where, R));
    CHECK(where[0] == N && where[1] == N);

    /* refused before anything runs */
    OK(hzsdr_framesync_get_state(f, where, holds, hist, last, R));
    CHECK(hzsdr_framesync_push(f, x, N, N - 1, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_push(f, x, N, PITCH, NULL, out, CAP, CAP * FB - 1, pos, info, counts, NULL) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_framesync_push(f, NULL, N, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_push(f, x, N, PITCH, NULL, NULL, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_push(f, x, N, PITCH, NULL, out, CAP, OPITCH, pos, info, NULL, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_push(NULL, x, N, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_framesync_set_state(f, where, holds, hist, last, R + 1) == HZSDR_ERR_INVALID_ARGUMENT);
    uint64_t where2[R], holds2[R];
    OK(hzsdr_framesync_get_state(f, where2, holds2, hist1, last1, R));
    CHECK(memcmp(where, where2, sizeof where) == 0 && memcmp(holds, holds2, sizeof holds) == 0 && memcmp(hist, hist1, sizeof hist) == 0);
    /* cap 0: counted only, null destinations */
    OK(hzsdr_framesync_reset(f));
    OK(hzsdr_framesync_push(f, x, N, PITCH, NULL, NULL, 0, 0, NULL, NULL, counts, &most));
    CHECK(counts[0] == 1 && counts[1] == 1 && most == 1);

    OK(hzsdr_framesync_free(f));
    OK(hzsdr_framesync_free(g));
    free(x);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("framesync-abi ok\n");
    return 0;
}
