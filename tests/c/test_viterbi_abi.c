/* test_viterbi_abi.c -- the Viterbi decoder bank (hzsdr_viterbi.h) exercised by a C compiler (gcc -std=c99) in a HOST
 * context: the text "decoded on device" and its CRC-16 through an encoder written here from the header's definition
 * (K = 7, 0171 / 0133, the second output inverted, TAIL), two pitched rows of three frame slots; clean frames and
 * frames with up to four flipped bits come back as the text with the flips as the metric and the CRC ok; a fifth slot
 * with a damaged CRC is flagged; the slots behind a row's count, the info behind them and the columns behind cap frames
 * stay as they were; soft input of the same frames gives the same bytes; sizes and plan; refused calls write nothing;
 * configurations out of bounds are refused.  Prints "viterbi-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_viterbi.h"

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

enum { K = 7, TEXT = 17, D = 8 * TEXT + 16, T = D + K - 1, N = 2 * T, FB = (N + 7) / 8, DB = (D + 7) / 8, R = 2, CAP = 3, IPITCH = CAP * FB + 3,
       OPITCH = CAP * DB + 5, SENT = 0xA5 };
static const char text[TEXT + 1] = "decoded on device";
static const unsigned gens[2] = {0171, 0133};

static unsigned parity(unsigned v) {
    unsigned p = 0;
    for (; v; v >>= 1) p ^= v & 1u;
    return p;
}

/* data bits -> N code bits, by the header's definition */
static void encode(const uint8_t *u, uint8_t *code) {
    unsigned state = 0;
    for (int t = 0; t < T; t++) {
        const unsigned reg = ((t < D ? u[t] : 0u) << (K - 1)) | state;
        code[2 * t] = (uint8_t)parity(reg & gens[0]);
        code[2 * t + 1] = (uint8_t)(parity(reg & gens[1]) ^ 1u);
        state = reg >> 1;
    }
}

static void pack(const uint8_t *bits, int n, uint8_t *bytes) {
    memset(bytes, 0, (size_t)(n + 7) / 8);
    for (int k = 0; k < n; k++)
        if (bits[k]) bytes[k / 8] |= (uint8_t)(0x80u >> (k % 8));
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* the data: the text and its CRC-16/CCITT-FALSE, bit by bit */
    uint8_t u[D], code[N], hurt[N];
    unsigned reg = 0xFFFFu;
    for (int k = 0; k < 8 * TEXT; k++) {
        u[k] = (uint8_t)((text[k / 8] >> (7 - k % 8)) & 1);
        const unsigned top = ((reg >> 15) & 1u) ^ u[k];
        reg = (reg << 1) & 0xFFFFu;
        if (top) reg ^= 0x1021u;
    }
    for (int k = 0; k < 16; k++) u[8 * TEXT + k] = (uint8_t)((reg >> (15 - k)) & 1u);
    encode(u, code);

    hzsdr_viterbi *v = NULL, *bad = NULL;
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, HZSDR_VITERBI_MAX_ROWS + 1, &bad) ==
          HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_create(ctx, 7, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, 10, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, gens, 2, 4, 4, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x10000, 0xFFFF, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, NULL, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(bad == NULL);
    OK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_BITS, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &v));
    size_t n = 0, fb = 0, t = 0, db = 0, g = 0, spl = 0, dbytes = 0;
    int form = 0;
    OK(hzsdr_viterbi_sizes(v, &n, &fb, &t, &db));
    OK(hzsdr_viterbi_plan(v, &g, &spl, &dbytes, &form));
    CHECK(n == N && fb == FB && t == T && db == DB && g == 1 && spl == 1 && dbytes == (size_t)T * 8 && form == HZSDR_VITERBI_FORM_LDS);
    OK(hzsdr_viterbi_sizes(v, NULL, NULL, NULL, NULL));

    /* slot (r, f) gets r * CAP + f flips (0 ... 4); slot (1, 2) gets a data bit changed BEFORE encoding: a valid code word, a wrong CRC */
    uint8_t *in = (uint8_t *)calloc((size_t)R * IPITCH, 1), *out = (uint8_t *)malloc((size_t)R * OPITCH);
    float *soft = (float *)calloc((size_t)R * CAP * N, sizeof(float));
    uint32_t info[R * CAP], counts[R] = {CAP + 4, 2};
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            const int flips = r * CAP + f;
            memcpy(hurt, code, N);
            if (r == 1 && f == 2) {
                uint8_t w[D];
                memcpy(w, u, D);
                w[9] ^= 1;
                encode(w, hurt);
            } else {
                for (int k = 0; k < flips; k++) hurt[(37 * k + 11 * flips) % N] ^= 1;
            }
            pack(hurt, N, in + r * IPITCH + f * FB);
            for (int k = 0; k < N; k++) soft[(r * CAP + f) * N + k] = hurt[k] ? 3.0f : -3.0f;
        }
    memset(out, SENT, (size_t)R * OPITCH);
    memset(info, SENT, sizeof info);
    OK(hzsdr_viterbi_decode(v, in, IPITCH, counts, CAP, out, OPITCH, info));
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            const uint8_t *p = out + r * OPITCH + f * DB;
            if (f < (int)(counts[r] < CAP ? counts[r] : CAP)) {
                CHECK(memcmp(p, text, TEXT) == 0 && info[r * CAP + f] == ((uint32_t)(r * CAP + f) | 0x80000000u));
                CHECK(p[TEXT] == (uint8_t)(reg >> 8) && p[TEXT + 1] == (uint8_t)reg);
            } else {
                for (int b = 0; b < DB; b++) CHECK(p[b] == SENT);
                CHECK(info[r * CAP + f] == 0xA5A5A5A5u);
            }
        }
    for (int r = 0; r < R; r++)
        for (int b = CAP * DB; b < OPITCH; b++) CHECK(out[r * OPITCH + b] == SENT);
    /* every slot: the changed data bit comes back as sent, with metric 0 and the CRC not ok */
    OK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, CAP, out, OPITCH, info));
    {
        const uint8_t *p = out + 1 * OPITCH + 2 * DB;
        CHECK(p[1] == (uint8_t)(text[1] ^ 0x40) && p[0] == (uint8_t)text[0] && info[1 * CAP + 2] == 0);
        CHECK(memcmp(out + 1 * OPITCH + 1 * DB, text, TEXT) == 0 && info[1 * CAP + 1] == (4u | 0x80000000u));
    }
    /* refused calls write nothing */
    memset(out, SENT, (size_t)R * OPITCH);
    CHECK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, CAP, out, CAP * DB - 1, info) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_viterbi_decode(v, in, CAP * FB - 1, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, 0, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, HZSDR_VITERBI_MAX_FRAMES / R + 1, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(v, NULL, IPITCH, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, CAP, NULL, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(v, in, IPITCH, NULL, CAP, out, OPITCH, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_viterbi_decode(NULL, in, IPITCH, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    for (int b = 0; b < R * OPITCH; b++) CHECK(out[b] == SENT);
    OK(hzsdr_viterbi_free(v));

    /* the same frames as soft values of magnitude 3: the same bytes, and every flip costs 3 */
    hzsdr_viterbi *s = NULL;
    OK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_SOFT_F32, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 1.0f, 16, 0x1021, 0xFFFF, 0, R, &s));
    CHECK(hzsdr_viterbi_create(ctx, HZSDR_VITERBI_SOFT_F32, K, 2, gens, 2, 3, 2, HZSDR_VITERBI_TAIL, D, 0.0f, 16, 0x1021, 0xFFFF, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    memset(out, SENT, (size_t)R * OPITCH);
    OK(hzsdr_viterbi_decode(s, soft, CAP * N, NULL, CAP, out, OPITCH, info));
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            if (r == 1 && f == 2) continue;
            const uint32_t cost = 3u * (uint32_t)(r * CAP + f);
            CHECK(memcmp(out + r * OPITCH + f * DB, text, TEXT) == 0 && info[r * CAP + f] == (cost | 0x80000000u));
        }
    OK(hzsdr_viterbi_free(s));
    CHECK(hzsdr_viterbi_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    free(in), free(out), free(soft);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("viterbi-abi ok\n");
    return 0;
}
