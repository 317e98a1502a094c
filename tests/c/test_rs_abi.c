/* test_rs_abi.c -- the Reed-Solomon decoder bank (hzsdr_rs.h) exercised by a C compiler (gcc -std=c99) in a HOST context:
 * the text "corrected on the device, twice" through an encoder written here from the header's definition (the DVB field
 * 0x11D, fcr 0, prim 1, 8 parity symbols, n = 23, two codewords interleaved, a scramble sequence of 5 bytes), two
 * pitched rows of three frame slots; clean frames and frames with up to four wrong symbols per codeword come back as the
 * text with the errors counted; five wrong symbols in one codeword fail that codeword and pass it through; the slots
 * behind a row's count, the bytes behind the data in a slot and the info behind a count stay as they were; in place gives
 * the same bytes; sizes and plan; refused calls write nothing; configurations out of bounds are refused.
 * Prints "rs-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_rs.h"

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

enum { POLY = 0x11D, NROOTS = 8, N = 23, KK = N - NROOTS, I = 2, F = I * N, IK = I * KK, R = 2, CAP = 3, IPITCH = F + 3, OPITCH = IK + 2,
       ISTRIDE = CAP * IPITCH + 1, OSTRIDE = CAP * OPITCH + 5, SENT = 0xA5 };
static const char text[IK + 1] = "corrected on the device, twice";
static const uint8_t scramble[5] = {0xFF, 0x48, 0x0E, 0xC0, 0x9A};

static unsigned gf_mul(unsigned a, unsigned b) {
    unsigned r = 0;
    for (; b; b >>= 1) {
        if (b & 1u) r ^= a;
        a <<= 1;
        if (a & 0x100u) a ^= POLY;
    }
    return r;
}

/* KK data symbols -> N symbols: the remainder of data(x) x^NROOTS by prod_j (x - alpha^j), by the header's definition */
static void encode(const uint8_t *data, uint8_t *word) {
    unsigned g[NROOTS + 1] = {1}, root = 1;
    for (int j = 0; j < NROOTS; j++) {
        for (int i = j + 1; i > 0; i--) g[i] ^= gf_mul(g[i - 1], root); /* g <- g (x + root), g[i]: the coefficient of x^(deg - i) */
        root = gf_mul(root, 2);
    }
    memset(word, 0, N);
    memcpy(word, data, KK);
    uint8_t rem[N];
    memcpy(rem, word, N);
    for (int p = 0; p < KK; p++) {
        const unsigned lead = rem[p];
        for (int i = 1; i <= NROOTS; i++) rem[p + i] ^= (uint8_t)gf_mul(lead, g[i]);
    }
    memcpy(word + KK, rem + KK, NROOTS);
}

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;
    /* the frame as sent: two codewords interleaved, scrambled */
    uint8_t sent[F], data[IK];
    memcpy(data, text, IK);
    for (int i = 0; i < I; i++) {
        uint8_t d[KK], w[N];
        for (int p = 0; p < KK; p++) d[p] = data[i + p * I];
        encode(d, w);
        for (int p = 0; p < N; p++) sent[i + p * I] = w[p];
    }
    for (int m = 0; m < F; m++) sent[m] ^= scramble[m % 5];

    hzsdr_rs *rs = NULL;
    OK(hzsdr_rs_create(ctx, POLY, 0, 1, NROOTS, N, I, NULL, NULL, scramble, 5, R, &rs));
    size_t k = 0, t = 0, fb = 0, db = 0, waves = 0, lds = 0, per_cu = 0, groups = 0;
    OK(hzsdr_rs_sizes(rs, &k, &t, &fb, &db));
    CHECK(k == KK && t == 4 && fb == F && db == IK);
    OK(hzsdr_rs_plan(rs, &waves, &lds, &per_cu, &groups));
    CHECK(waves == I && lds > 1280 && lds < 8192 && per_cu == 16 && groups >= 1);

    /* slot (r, f) carries r * CAP + f wrong symbols in codeword 0 (0 ... 5) and one in codeword 1 where f is odd */
    static uint8_t in[R * ISTRIDE], out[R * OSTRIDE], keep[R * ISTRIDE];
    uint32_t info[R * CAP], counts[R] = {3, 7};
    memset(in, 0x3C, sizeof in);
    memset(out, SENT, sizeof out);
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            uint8_t *p = in + r * ISTRIDE + f * IPITCH;
            memcpy(p, sent, F);
            for (int e = 0; e < r * CAP + f; e++) p[0 + (3 * e + 1) * I] ^= (uint8_t)(0x01 + 0x33 * e);
            if (f & 1) p[1 + (N - 1) * I] ^= 0xFF;
            info[r * CAP + f] = 0x77777777u;
        }
    memcpy(keep, in, sizeof in);
    OK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, counts, CAP, out, OSTRIDE, OPITCH, info));
    CHECK(memcmp(in, keep, sizeof in) == 0);
    for (int r = 0; r < R; r++) {
        for (int f = 0; f < CAP; f++) {
            const uint8_t *p = out + r * OSTRIDE + f * OPITCH;
            const int e0 = r * CAP + f, e1 = f & 1;
            if (e0 <= 4) {
                CHECK(memcmp(p, text, IK) == 0);
                CHECK(info[r * CAP + f] == ((uint32_t)(e0 + e1) | 0x80000000u));
            } else { /* five errors: codeword 0 fails and passes through as received (descrambled), codeword 1 is corrected */
                CHECK(info[r * CAP + f] == ((uint32_t)e1 | 1u << 16));
                for (int m = 0; m < IK; m++)
                    CHECK(p[m] == ((m % I) ? (uint8_t)text[m] : (uint8_t)(keep[r * ISTRIDE + f * IPITCH + m] ^ scramble[m % 5])));
            }
            CHECK(p[IK] == SENT && p[IK + 1] == SENT);
        }
        for (int m = CAP * OPITCH; m < OSTRIDE; m++) CHECK(out[r * OSTRIDE + m] == SENT);
    }

    /* a count below cap: the slots and the info behind it stay */
    memset(out, SENT, sizeof out);
    counts[0] = 1, counts[1] = 0;
    for (int s = 0; s < R * CAP; s++) info[s] = 0x77777777u;
    OK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, counts, CAP, out, OSTRIDE, OPITCH, info));
    CHECK(memcmp(out, text, IK) == 0 && info[0] == 0x80000000u);
    for (int m = IK; m < R * OSTRIDE; m++) CHECK(out[m] == SENT);
    for (int s = 1; s < R * CAP; s++) CHECK(info[s] == 0x77777777u);

    /* in place */
    OK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, in, ISTRIDE, IPITCH, info));
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            const uint8_t *p = in + r * ISTRIDE + f * IPITCH;
            if (r * CAP + f <= 4) CHECK(memcmp(p, text, IK) == 0);
            CHECK(memcmp(p + IK, keep + r * ISTRIDE + f * IPITCH + IK, IPITCH - IK) == 0);
        }
    memcpy(in, keep, sizeof in);

    /* refused calls write nothing */
    memset(out, SENT, sizeof out);
    for (int s = 0; s < R * CAP; s++) info[s] = 0x77777777u;
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, out, CAP * OPITCH - 1, OPITCH, info) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_rs_decode(rs, in, CAP * IPITCH - 1, IPITCH, NULL, CAP, out, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, F - 1, NULL, CAP, out, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, out, OSTRIDE, IK - 1, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, 0, out, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, NULL, ISTRIDE, IPITCH, NULL, CAP, out, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, NULL, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, out, OSTRIDE, OPITCH, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, in + 1, ISTRIDE, IPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(rs, in, ISTRIDE, IPITCH, NULL, CAP, in, ISTRIDE + 2, IPITCH + 1, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_decode(NULL, in, ISTRIDE, IPITCH, NULL, CAP, out, OSTRIDE, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    for (size_t m = 0; m < sizeof out; m++) CHECK(out[m] == SENT);
    for (int s = 0; s < R * CAP; s++) CHECK(info[s] == 0x77777777u);
    CHECK(memcmp(in, keep, sizeof in) == 0);
    OK(hzsdr_rs_free(rs));

    /* configurations out of bounds */
    hzsdr_rs *bad = NULL;
    CHECK(hzsdr_rs_create(ctx, 0x11B, 0, 1, 8, 23, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT && bad == NULL); /* not primitive */
    CHECK(hzsdr_rs_create(ctx, 0x1D, 0, 1, 8, 23, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 255, 1, 8, 23, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 51, 8, 23, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 1, 23, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 65, 255, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 8, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 256, 1, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 23, 9, NULL, NULL, NULL, 0, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 23, 1, NULL, NULL, NULL, 3, 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 23, 1, NULL, NULL, NULL, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_create(ctx, POLY, 0, 1, 8, 23, 1, NULL, NULL, NULL, 0, HZSDR_RS_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_rs_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("rs-abi ok\n");
    return 0;
}
