/* test_hdlc_abi.c -- the HDLC deframer bank (hzsdr_hdlc.h) exercised by a C compiler (gcc -std=c99) in a HOST context:
 * two pitched real rows that carry the text "hello, hdlc \xff\xff" between flags, stuffed, with its CRC-16/X.25 behind it,
 * the second row with a bit error; the good frame comes back as the bytes written with its position and
 * verdict, the bad one only under keep_bad; slot tails, the slots behind a row's count and the columns behind cap frames
 * stay as they were; the stream cut anywhere finds what one push finds, in the push that delivers the closing flag's
 * last bit; the state carries into a second object; in_counts are obeyed and clamped; a refused push changes nothing;
 * reset starts over; configurations out of bounds are refused.
 * Prints "hdlc-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_hdlc.h"

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

enum { N = 400, R = 2, PITCH = N + 5, TEXT = 14, FRAME = TEXT + 2, MAXB = 20, CAP = 3, OPITCH = CAP * MAXB + 7, AT = 50,
       HB = (8 * MAXB + 8 * MAXB / 5 + 8 + 7) / 8 };
static const uint8_t text[TEXT + 1] = "hello, hdlc \xff\xff";

static int put(int *bits, int at, int bit) {
    bits[at] = bit;
    return at + 1;
}
static int put_flag(int *bits, int at) {
    static const int f[8] = {0, 1, 1, 1, 1, 1, 1, 0};
    for (int k = 0; k < 8; k++) at = put(bits, at, f[k]);
    return at;
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* the frame's bytes: the text and its FCS, least significant byte first */
    uint8_t frame[FRAME];
    uint32_t c = 0xFFFFu;
    memcpy(frame, text, TEXT);
    for (int k = 0; k < 8 * TEXT; k++) c = (c >> 1) ^ (((c ^ (uint32_t)(text[k / 8] >> (k % 8))) & 1u) ? 0x8408u : 0u);
    c ^= 0xFFFFu;
    frame[TEXT] = (uint8_t)c, frame[TEXT + 1] = (uint8_t)(c >> 8);
    /* the stream: zeros, a flag at bit AT, the frame stuffed, a flag, zeros */
    int bits[N] = {0}, at = AT, ones = 0, first_bit, done;
    at = put_flag(bits, at);
    first_bit = at;
    for (int k = 0; k < 8 * FRAME; k++) {
        const int bit = (frame[k / 8] >> (k % 8)) & 1;
        at = put(bits, at, bit);
        ones = bit ? ones + 1 : 0;
        if (ones == 5) at = put(bits, at, 0), ones = 0;
    }
    CHECK(at > first_bit + 8 * FRAME + 2); /* (something was stuffed) */
    at = put_flag(bits, at);
    done = at; /* the push that delivers bit done - 1 emits the frame */
    float *x = (float *)calloc((size_t)R * PITCH, sizeof(float));
    for (int r = 0; r < R; r++)
        for (int i = 0; i < N; i++) {
            const int bit = bits[i] ^ (r == 1 && i == first_bit + 17); /* (a flip that leaves the stuffing alone) */
            x[r * PITCH + i] = (float)(1 + i % 7) * (bit ? 0.5f : -0.5f);
        }
    hzsdr_hdlc *f = NULL, *g = NULL, *bad = NULL;
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 0, HZSDR_HDLC_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, 7, 0, 16, 3, MAXB, 0, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 3, 16, 3, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, -1, 16, 3, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 8, 3, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 2, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 32, 4, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 0, 0, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, MAXB + 1, MAXB, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, HZSDR_HDLC_MAX_BYTES + 1, 0, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 2, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 2, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(bad == NULL);
    OK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 0, R, &f));
    OK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 1, R, &g)); /* keep_bad */
    size_t rpw = 0, tile = 0, ring = 0;
    int form = -1;
    OK(hzsdr_hdlc_plan(f, &rpw, &tile, &ring, &form));
    CHECK(rpw == 1 && tile == 64 && ring == 32 && form == HZSDR_HDLC_FORM_FCS16);
    OK(hzsdr_hdlc_plan(g, NULL, NULL, NULL, &form));
    CHECK(form == (HZSDR_HDLC_FORM_FCS16 | HZSDR_HDLC_FORM_KEEP_BAD));

    uint8_t out[R * OPITCH], one[R * OPITCH];
    uint64_t pos[R * CAP], pos1[R * CAP], where[R], events[R], events1[R];
    uint32_t info[R * CAP], info1[R * CAP], counts[R];
    uint8_t hist[R * HB], last[R], kinds[R], hist1[R * HB], last1[R], kinds1[R];
    size_t most = 99;
    memset(one, 0xA5, sizeof one), memset(pos1, 0xA5, sizeof pos1), memset(info1, 0xA5, sizeof info1);
    OK(hzsdr_hdlc_push(f, x, N, PITCH, NULL, one, CAP, OPITCH, pos1, info1, counts, &most));
    CHECK(most == 1 && counts[0] == 1 && counts[1] == 0);
    CHECK(memcmp(one, frame, FRAME) == 0 && pos1[0] == (uint64_t)first_bit && info1[0] == (FRAME | 0x80000000u));
    for (int i = FRAME; i < OPITCH; i++) CHECK(one[i] == 0xA5); /* the slot's tail, the other slots, the pad */
    for (int i = 0; i < OPITCH; i++) CHECK(one[OPITCH + i] == 0xA5);
    CHECK(pos1[1] == 0xA5A5A5A5A5A5A5A5ull && info1[2] == 0xA5A5A5A5u && pos1[CAP] == 0xA5A5A5A5A5A5A5A5ull);
    OK(hzsdr_hdlc_get_state(f, where, events1, kinds1, hist1, last1, R));
    CHECK(where[0] == N && where[1] == N && events1[0] == (uint64_t)done && events1[1] == (uint64_t)done && kinds1[0] == HZSDR_HDLC_EVENT_FLAG);
    CHECK(hzsdr_hdlc_get_state(f, where, events1, kinds1, hist1, last1, R - 1) == HZSDR_ERR_DST_TOO_SMALL);
    /* keep_bad: row 1's frame comes out too, marked */
    memset(out, 0xA5, sizeof out);
    OK(hzsdr_hdlc_push(g, x, N, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, &most));
    CHECK(counts[0] == 1 && counts[1] == 1 && info[0] == (FRAME | 0x80000000u) && info[CAP] == FRAME && pos[CAP] == (uint64_t)first_bit);
    CHECK(memcmp(out, frame, FRAME) == 0 && memcmp(out + OPITCH, frame, FRAME) != 0 && out[OPITCH + FRAME] == 0xA5);
    OK(hzsdr_hdlc_free(g));
    OK(hzsdr_hdlc_create(ctx, HZSDR_SYMSYNC_REAL_F32, 0, 16, 3, MAXB, 0, 0, R, &g));

    /* every cut: the frame comes with the push that delivers bit done - 1; the state equals the one push's */
    for (int cut = 0; cut <= N; cut += (cut > done - 70 && cut < done + 70) ? 1 : 37) {
        OK(hzsdr_hdlc_reset(f));
        memset(out, 0xA5, sizeof out);
        OK(hzsdr_hdlc_push(f, x, (size_t)cut, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL));
        const int first = cut >= done;
        CHECK(counts[0] == (uint32_t)first && counts[1] == 0);
        if (!first) CHECK(out[0] == 0xA5);
        OK(hzsdr_hdlc_get_state(f, where, events, kinds, hist, last, R));
        CHECK(where[0] == (uint64_t)cut);
        OK(hzsdr_hdlc_set_state(g, where, events, kinds, hist, last, R));
        OK(hzsdr_hdlc_push(g, x + cut, (size_t)(N - cut), PITCH, NULL, out, CAP, OPITCH, pos, info, counts, &most));
        CHECK(counts[0] == (uint32_t)!first && most == (size_t)!first);
        CHECK(memcmp(out, frame, FRAME) == 0 && out[FRAME] == 0xA5 && pos[0] == (uint64_t)first_bit);
        OK(hzsdr_hdlc_get_state(g, where, events, kinds, hist, last, R));
        CHECK(where[1] == N && events[0] == events1[0] && kinds[1] == kinds1[1] && memcmp(hist, hist1, sizeof hist) == 0 && memcmp(last, last1, sizeof last) == 0);
    }

    /* in_counts: row 0 takes all, row 1 nothing; then row 0 nothing and row 1 a count above n, clamped */
    OK(hzsdr_hdlc_reset(f));
    uint32_t ic[R] = {N, 0};
    OK(hzsdr_hdlc_push(f, x, N, PITCH, ic, out, CAP, OPITCH, pos, info, counts, &most));
    CHECK(counts[0] == 1 && counts[1] == 0 && most == 1);
    OK(hzsdr_hdlc_positions(f, where, R));
    CHECK(where[0] == N && where[1] == 0);
    ic[0] = 0, ic[1] = 0xFFFFFFFFu;
    OK(hzsdr_hdlc_push(f, x, N, PITCH, ic, out, CAP, OPITCH, pos, info, counts, NULL));
    CHECK(counts[0] == 0 && counts[1] == 0);
    OK(hzsdr_hdlc_positions(f, where, R));
    CHECK(where[0] == N && where[1] == N);

    /* refused before anything runs */
    OK(hzsdr_hdlc_get_state(f, where, events, kinds, hist, last, R));
    CHECK(hzsdr_hdlc_push(f, x, N, N - 1, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_push(f, x, N, PITCH, NULL, out, CAP, CAP * MAXB - 1, pos, info, counts, NULL) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_hdlc_push(f, NULL, N, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_push(f, x, N, PITCH, NULL, NULL, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_push(f, x, N, PITCH, NULL, out, CAP, OPITCH, pos, info, NULL, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_push(NULL, x, N, PITCH, NULL, out, CAP, OPITCH, pos, info, counts, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_hdlc_set_state(f, where, events, kinds, hist, last, R + 1) == HZSDR_ERR_INVALID_ARGUMENT);
    events[0] = where[0] + 1; /* an event the stream has not reached */
    CHECK(hzsdr_hdlc_set_state(f, where, events, kinds, hist, last, R) == HZSDR_ERR_INVALID_ARGUMENT);
    events[0] = where[0], kinds[1] = 2;
    CHECK(hzsdr_hdlc_set_state(f, where, events, kinds, hist, last, R) == HZSDR_ERR_INVALID_ARGUMENT);
    uint64_t where2[R], events2[R];
    OK(hzsdr_hdlc_get_state(f, where2, events2, kinds1, hist1, last1, R));
    CHECK(memcmp(where, where2, sizeof where) == 0 && events2[1] == events[1] && memcmp(hist, hist1, sizeof hist) == 0);
    /* cap 0: counted only, null destinations */
    OK(hzsdr_hdlc_reset(f));
    OK(hzsdr_hdlc_push(f, x, N, PITCH, NULL, NULL, 0, 0, NULL, NULL, counts, &most));
    CHECK(counts[0] == 1 && counts[1] == 0 && most == 1);

    OK(hzsdr_hdlc_free(f));
    OK(hzsdr_hdlc_free(g));
    free(x);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("hdlc-abi ok\n");
    return 0;
}
