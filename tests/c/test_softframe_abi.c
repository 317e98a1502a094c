/* test_softframe_abi.c -- the soft frame bank (hzsdr_softframe.h) exercised by a C compiler (gcc -std=c99) in a HOST
 * context beside a frame sync bank: two pitched rows of real soft symbols, the second received inverted, each with two
 * frames of a 16-bit word and a 24-bit payload whose floats include a NaN with payload bits, -0 and an infinity; the stream
 * goes through both banks in three pushes that cut a payload; every frame's floats are the stream's floats (row 1: with
 * the sign bit flipped) bit for bit, their signs are the bits the frame sync bank packed, the slots behind a row's count
 * and the row padding stay as they were; a forged position and a forged hypothesis give quiet NaNs and their status; the
 * state moves into a second bank; plan, positions, reset; refused calls write nothing; configurations out of bounds
 * are refused.  Prints "softframe-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_framesync.h"
#include "hzsdr_softframe.h"

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

enum { W = 16, P = 24, R = 2, CAP = 3, N = 120, PITCH = N + 5, OSTRIDE = CAP * P + 7, HF = P - 1 };
#define WORD 0xEB90u
#define SENT 0xA5A5A5A5u
#define QNAN 0x7FC00000u

static uint32_t bits_of(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

static float float_of(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}

static uint32_t lcg = 12345u;
static unsigned coin(void) {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 16) & 1u;
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;

    /* the rows: +-1 by coin, two frames each; row 1 is row 0's pattern inverted, its frames three symbols later */
    static float x[R * PITCH];
    static uint32_t sent[R][2][P]; /* the payload floats as sent into the row, as bit patterns */
    const size_t at[R][2] = {{10, 62}, {13, 65}};
    for (int r = 0; r < R; r++) {
        for (int i = 0; i < PITCH; i++) x[r * PITCH + i] = coin() ? 1.0f : -1.0f;
        for (int f = 0; f < 2; f++) {
            for (int k = 0; k < W; k++) {
                const unsigned b = ((WORD >> (W - 1 - k)) & 1u) ^ (unsigned)r;
                x[r * PITCH + at[r][f] + k] = b ? 0.75f : -0.75f;
            }
            float *pay = x + r * PITCH + at[r][f] + W;
            pay[3] = float_of((bits_of(pay[3]) & 0x80000000u) | 0x7FC12345u); /* a NaN with payload bits */
            pay[4] = float_of(bits_of(pay[4]) & 0x80000000u);                 /* +-0 */
            pay[9] = float_of((bits_of(pay[9]) & 0x80000000u) | 0x7F800000u); /* +-inf */
            for (int k = 0; k < P; k++) sent[r][f][k] = bits_of(pay[k]);
        }
    }

    const uint64_t words[2] = {WORD, WORD ^ 0xFFFFu};
    const unsigned maps[2] = {0, 1};
    hzsdr_framesync *fs = NULL;
    hzsdr_softframe *sf = NULL, *sf2 = NULL;
    OK(hzsdr_framesync_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, W, 0xFFFFu, 0, 2, words, maps, P, 0, W + P, R, &fs));
    OK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 2, maps, R, &sf));
    OK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 2, maps, R, &sf2));
    size_t step = 0, hf = 0;
    int form = -1;
    OK(hzsdr_softframe_plan(sf, &step, &hf, &form));
    CHECK(step == 256 && hf == HF && form == 0);

    /* three pushes: 0 ... 39 (inside frame 0's payload), 40 ... 39 (nothing), 40 ... N - 1 */
    const size_t cuts[4] = {0, 40, 40, N};
    int seen[R] = {0, 0};
    static uint64_t mid_pos[R];
    static float mid_hist[R * HF];
    for (int p = 0; p < 3; p++) {
        const size_t n = cuts[p + 1] - cuts[p];
        static uint8_t frames[R * CAP * 3];
        uint64_t pos[R * CAP];
        uint32_t info[R * CAP], counts[R], status[R * CAP];
        static uint32_t out[R * OSTRIDE];
        for (int i = 0; i < R * OSTRIDE; i++) out[i] = SENT;
        for (int i = 0; i < R * CAP; i++) status[i] = SENT;
        OK(hzsdr_framesync_push(fs, n ? x + cuts[p] : NULL, n, PITCH, NULL, frames, CAP, CAP * 3, pos, info, counts, NULL));
        OK(hzsdr_softframe_push(sf, n ? x + cuts[p] : NULL, n, PITCH, NULL, pos, info, counts, CAP, (float *)out, OSTRIDE, status));
        if (p == 0) OK(hzsdr_softframe_get_state(sf, mid_pos, mid_hist, R));
        if (p == 2) { /* the same push through the bank that got the state */
            static uint32_t out2[R * OSTRIDE];
            uint32_t status2[R * CAP];
            for (int i = 0; i < R * OSTRIDE; i++) out2[i] = SENT;
            for (int i = 0; i < R * CAP; i++) status2[i] = SENT;
            OK(hzsdr_softframe_set_state(sf2, mid_pos, mid_hist, R));
            OK(hzsdr_softframe_push(sf2, x + cuts[p], n, PITCH, NULL, pos, info, counts, CAP, (float *)out2, OSTRIDE, status2));
            CHECK(memcmp(out, out2, sizeof out) == 0 && memcmp(status, status2, sizeof status) == 0);
        }
        for (int r = 0; r < R; r++) {
            CHECK(counts[r] == (p == 2 ? 2u : 0u));
            for (uint32_t f = 0; f < CAP; f++) {
                const uint32_t *y = out + r * OSTRIDE + f * P;
                if (f >= counts[r]) {
                    CHECK(status[r * CAP + f] == SENT);
                    for (int k = 0; k < P; k++) CHECK(y[k] == SENT);
                    continue;
                }
                CHECK(status[r * CAP + f] == HZSDR_SOFTFRAME_SERVED && pos[r * CAP + f] == at[r][seen[r]] + W && (info[r * CAP + f] >> 8) == (uint32_t)r);
                for (int k = 0; k < P; k++) {
                    CHECK(y[k] == (sent[r][seen[r]][k] ^ (r ? 0x80000000u : 0u)));
                    const unsigned bit = (frames[(r * CAP + f) * 3 + k / 8] >> (7 - k % 8)) & 1u;
                    CHECK(bit == ((y[k] >> 31) ^ 1u));
                }
                seen[r]++;
            }
            for (int i = CAP * P; i < OSTRIDE; i++) CHECK(out[r * OSTRIDE + i] == SENT);
        }
    }
    CHECK(seen[0] == 2 && seen[1] == 2 && mid_pos[0] == 40 && mid_pos[1] == 40);
    for (int k = 0; k < HF; k++) CHECK(bits_of(mid_hist[k]) == bits_of(x[40 - HF + k]) && bits_of(mid_hist[HF + k]) == bits_of(x[PITCH + 40 - HF + k]));
    uint64_t where[R] = {0, 0};
    OK(hzsdr_softframe_positions(sf, where, R));
    CHECK(where[0] == N && where[1] == N);

    /* forged arrays: before the window, behind it, a hypothesis the bank does not have, and one honest slot */
    {
        float more[R * 8];
        for (int i = 0; i < R * 8; i++) more[i] = 1.0f;
        uint64_t pos[R * CAP] = {N - HF - 1, N + 8 - P + 1, N, /* row 1 */ N + 8 - P, ~0ull, 3};
        uint32_t info[R * CAP] = {0, 0, 2u << 8, 1u << 8, 0, 0}, counts[R] = {3, 77}, status[R * CAP];
        static uint32_t out[R * CAP * P];
        OK(hzsdr_softframe_push(sf, more, 8, 8, NULL, pos, info, counts, CAP, (float *)out, CAP * P, status));
        CHECK(status[0] == HZSDR_SOFTFRAME_OUTSIDE && status[1] == HZSDR_SOFTFRAME_OUTSIDE && status[2] == HZSDR_SOFTFRAME_NO_HYPOTHESIS);
        CHECK(status[3] == HZSDR_SOFTFRAME_SERVED && status[4] == HZSDR_SOFTFRAME_OUTSIDE && status[5] == HZSDR_SOFTFRAME_OUTSIDE);
        for (int s = 0; s < R * CAP; s++)
            for (int k = 0; k < P; k++) {
                if (s != 3)
                    CHECK(out[s * P + k] == QNAN);
                else /* the last P symbols of row 1: P - 8 from the history, 8 ones, inverted */
                    CHECK(out[s * P + k] == ((k < P - 8 ? bits_of(x[PITCH + N - (P - 8) + k]) : bits_of(1.0f)) ^ 0x80000000u));
            }
    }

    /* refused calls write nothing and leave the state */
    {
        uint64_t pos[R * CAP] = {0};
        uint32_t info[R * CAP] = {0}, counts[R] = {1, 1}, status[R * CAP];
        static uint32_t out[R * OSTRIDE];
        for (int i = 0; i < R * OSTRIDE; i++) out[i] = SENT;
        for (int i = 0; i < R * CAP; i++) status[i] = SENT;
        CHECK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, pos, info, counts, CAP, (float *)out, CAP * P - 1, status) == HZSDR_ERR_DST_TOO_SMALL);
        CHECK(hzsdr_softframe_push(sf, x, 8, 7, NULL, pos, info, counts, CAP, (float *)out, OSTRIDE, status) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(sf, NULL, 8, PITCH, NULL, pos, info, counts, CAP, (float *)out, OSTRIDE, status) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, NULL, info, counts, CAP, (float *)out, OSTRIDE, status) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, pos, info, counts, CAP, NULL, OSTRIDE, status) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, pos, info, counts, CAP, (float *)out, OSTRIDE, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, pos, info, counts, (1u << 22) / R + 1, (float *)out, (size_t)1 << 40, status) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_push(NULL, x, 8, PITCH, NULL, pos, info, counts, CAP, (float *)out, OSTRIDE, status) == HZSDR_ERR_INVALID_ARGUMENT);
        for (int i = 0; i < R * OSTRIDE; i++) CHECK(out[i] == SENT);
        for (int i = 0; i < R * CAP; i++) CHECK(status[i] == SENT);
        OK(hzsdr_softframe_positions(sf, where, R));
        CHECK(where[0] == N + 8 && where[1] == N + 8);
        CHECK(hzsdr_softframe_positions(sf, where, 1) == HZSDR_ERR_DST_TOO_SMALL);
        OK(hzsdr_softframe_push(sf, x, 8, PITCH, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL)); /* cap = 0: the history only */
        OK(hzsdr_softframe_positions(sf, where, R));
        CHECK(where[0] == N + 16);
        OK(hzsdr_softframe_reset(sf));
        OK(hzsdr_softframe_get_state(sf, mid_pos, mid_hist, R));
        CHECK(mid_pos[0] == 0 && mid_pos[1] == 0);
        for (int k = 0; k < R * HF; k++) CHECK(bits_of(mid_hist[k]) == 0);
        mid_pos[1] = (uint64_t)1 << 62;
        CHECK(hzsdr_softframe_set_state(sf, mid_pos, mid_hist, R) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_set_state(sf, mid_pos, mid_hist, 1) == HZSDR_ERR_INVALID_ARGUMENT);
    }

    /* configurations out of bounds */
    {
        hzsdr_softframe *bad = NULL;
        const unsigned m4[4] = {0, 1, 2, 3}, m2[1] = {2};
        CHECK(hzsdr_softframe_create(ctx, HZSDR_FMT_U8, 1, P, 1, maps, 1, &bad) == HZSDR_ERR_FORMAT_UNKNOWN && !bad);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 2, P, 1, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, 0, 1, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, 8193, 1, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_FMT_C64, 2, 7, 1, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 0, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 5, maps, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 1, m2, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_FMT_C64, 1, P, 4, m4, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 1, maps, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 1, maps, 8193, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        CHECK(hzsdr_softframe_create(ctx, HZSDR_SYMSYNC_REAL_F32, 1, P, 1, NULL, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
        OK(hzsdr_softframe_create(ctx, HZSDR_FMT_C64, 2, 8192, 4, m4, 2, &bad));
        OK(hzsdr_softframe_plan(bad, &step, &hf, &form));
        CHECK(step == 512 && hf == 8190 && form == (HZSDR_SOFTFRAME_FORM_COMPLEX | HZSDR_SOFTFRAME_FORM_DIBIT));
        OK(hzsdr_softframe_free(bad));
    }
    OK(hzsdr_softframe_free(sf));
    OK(hzsdr_softframe_free(sf2));
    OK(hzsdr_framesync_free(fs));
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("softframe-abi ok\n");
    return 0;
}
