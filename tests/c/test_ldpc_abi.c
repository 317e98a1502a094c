/* test_ldpc_abi.c -- the LDPC decoder bank (hzsdr_ldpc.h) exercised by a C compiler (gcc -std=c99) in a HOST context:
 * the Hamming (7, 4) matrix in compressed form, a nibble per frame through an encoder written here from the matrix, two
 * pitched rows of three frame slots; clean hard frames come back as their nibbles with iters = 0 and ok; the slots
 * behind a row's count, the info behind them and the columns behind cap frames stay as they were; soft frames with one
 * weak value of the wrong sign are put right in one iteration; sizes and plan; refused calls write nothing;
 * configurations out of bounds are refused.  Prints "ldpc-abi ok" and exits 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hzsdr_ldpc.h"

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

enum { NV = 7, M = 3, E = 12, D = 4, FB = 1, DB = 1, R = 2, CAP = 3, IPITCH = CAP * FB + 3, OPITCH = CAP * DB + 5, SENT = 0xA5 };
/* the checks: d0 d1 d3 p0; d0 d2 d3 p1; d1 d2 d3 p2 */
static const uint32_t row_ptr[M + 1] = {0, 4, 8, 12};
static const uint32_t col[E] = {0, 1, 3, 4, 0, 2, 3, 5, 1, 2, 3, 6};

/* a nibble (d0 its most significant bit) -> the 7 code bits */
static void encode(unsigned nibble, uint8_t *x) {
    for (int k = 0; k < 4; k++) x[k] = (uint8_t)((nibble >> (3 - k)) & 1u);
    x[4] = x[0] ^ x[1] ^ x[3], x[5] = x[0] ^ x[2] ^ x[3], x[6] = x[1] ^ x[2] ^ x[3];
}

static unsigned nibble_of(int r, int f) { return (unsigned)(r * CAP + f + 5) & 15u; }

int main(void) {
    int count = 0;
    if (hzsdr_device_count(&count) != HZSDR_OK || count < 1) {
        printf("no gfx950 device\n");
        return 2;
    }
    if (hzsdr_open(0, HZSDR_MEM_HOST, &ctx) != HZSDR_OK) return 3;

    hzsdr_ldpc *l = NULL, *bad = NULL;
    uint32_t far[E];
    memcpy(far, col, sizeof far);
    far[5] = NV;
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, 0, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, HZSDR_LDPC_MAX_ROWS + 1, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, 7, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_FORMAT_UNKNOWN);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, 0, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, NULL, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, NULL, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, far, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E - 1, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 1, NV, D, 1.0f, 8, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 0, 10, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 256, 16, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 17, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(bad == NULL);
    OK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_BITS, M, NV, row_ptr, col, E, 0, NV, D, 1.0f, 8, 10, 16, 0, R, &l));
    size_t n = 0, fb = 0, vars = 0, checks = 0, edges = 0, db = 0, g = 0, t = 0, bytes = 0;
    int form = 0;
    OK(hzsdr_ldpc_sizes(l, &n, &fb, &vars, &checks, &edges, &db));
    OK(hzsdr_ldpc_plan(l, &g, &t, &bytes, &form));
    CHECK(n == NV && fb == FB && vars == NV && checks == M && edges == E && db == DB);
    CHECK(g == 8 && t == 64 && bytes == 48 && form == HZSDR_LDPC_FORM_TABLES_LDS);
    OK(hzsdr_ldpc_sizes(l, NULL, NULL, NULL, NULL, NULL, NULL));

    uint8_t *in = (uint8_t *)calloc((size_t)R * IPITCH, 1), *out = (uint8_t *)malloc((size_t)R * OPITCH), x[NV];
    float soft[R * CAP * NV];
    uint32_t info[R * CAP], counts[R] = {CAP + 4, 2};
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            const int slot = r * CAP + f;
            encode(nibble_of(r, f), x);
            for (int k = 0; k < NV; k++) {
                if (x[k]) in[r * IPITCH + f * FB] |= (uint8_t)(0x80u >> k);
                soft[slot * NV + k] = x[k] ? 3.0f : -3.0f;
            }
            if (slot > 0) soft[slot * NV + slot % NV] = x[slot % NV] ? -0.2f : 0.2f;  /* one weak value of the wrong sign */
        }
    memset(out, SENT, (size_t)R * OPITCH);
    memset(info, SENT, sizeof info);
    OK(hzsdr_ldpc_decode(l, in, IPITCH, counts, CAP, out, OPITCH, info));
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++) {
            const uint8_t *p = out + r * OPITCH + f * DB;
            if (f < (int)(counts[r] < CAP ? counts[r] : CAP)) {
                CHECK(p[0] == (uint8_t)(nibble_of(r, f) << 4) && info[r * CAP + f] == 0x80000000u);
            } else {
                CHECK(p[0] == SENT && info[r * CAP + f] == 0xA5A5A5A5u);
            }
        }
    for (int r = 0; r < R; r++)
        for (int b = CAP * DB; b < OPITCH; b++) CHECK(out[r * OPITCH + b] == SENT);
    /* refused calls write nothing */
    memset(out, SENT, (size_t)R * OPITCH);
    CHECK(hzsdr_ldpc_decode(l, in, IPITCH, NULL, CAP, out, CAP * DB - 1, info) == HZSDR_ERR_DST_TOO_SMALL);
    CHECK(hzsdr_ldpc_decode(l, in, CAP * FB - 1, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(l, in, IPITCH, NULL, 0, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(l, in, IPITCH, NULL, HZSDR_LDPC_MAX_FRAMES / R + 1, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(l, NULL, IPITCH, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(l, in, IPITCH, NULL, CAP, NULL, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(l, in, IPITCH, NULL, CAP, out, OPITCH, NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    CHECK(hzsdr_ldpc_decode(NULL, in, IPITCH, NULL, CAP, out, OPITCH, info) == HZSDR_ERR_INVALID_ARGUMENT);
    for (int b = 0; b < R * OPITCH; b++) CHECK(out[b] == SENT);
    OK(hzsdr_ldpc_free(l));

    /* soft values of magnitude 3 under scale 5 (q = +-15), one of them +-0.2 on the wrong side (q = -+1): its checks
     * send it 15 * 12 / 16 = 11 each, the others get 1 * 12 / 16 = 0 from it: put right in one iteration */
    hzsdr_ldpc *s = NULL;
    OK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_SOFT_F32, M, NV, row_ptr, col, E, 0, NV, D, 5.0f, 0, 10, 12, 0, R, &s));
    CHECK(hzsdr_ldpc_create(ctx, HZSDR_LDPC_SOFT_F32, M, NV, row_ptr, col, E, 0, NV, D, 0.0f, 0, 10, 12, 0, R, &bad) == HZSDR_ERR_INVALID_ARGUMENT);
    memset(out, SENT, (size_t)R * OPITCH);
    OK(hzsdr_ldpc_decode(s, soft, CAP * NV, NULL, CAP, out, OPITCH, info));
    for (int r = 0; r < R; r++)
        for (int f = 0; f < CAP; f++)
            CHECK(out[r * OPITCH + f * DB] == (uint8_t)(nibble_of(r, f) << 4) && info[r * CAP + f] == (0x80000000u | (r * CAP + f > 0 ? 1u << 16 : 0u)));
    OK(hzsdr_ldpc_free(s));
    CHECK(hzsdr_ldpc_free(NULL) == HZSDR_ERR_INVALID_ARGUMENT);
    free(in), free(out);
    hzsdr_close(ctx);
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("ldpc-abi ok\n");
    return 0;
}
