// hz_rs_math.h -- the arithmetic of the Reed-Solomon decoder bank (include/hzsdr_rs.h), shared by the kernel (hz_rs.hip)
// and the host restatement (tests/host/rs_ref.cpp): the field GF(2^8) over a 9-bit polynomial (table construction,
// multiply, inverse), the code's roots and the position-to-locator map, and the decoder's steps -- a syndrome step, a
// Berlekamp-Massey coefficient update, the evaluator's coefficients, the locator's value at a position and Forney's error
// value -- each written once, for one element.  decode_word() at the end strings them together one element after the
// other: the plain statement of what the kernel does lane-wide.  Integer arithmetic throughout; HIP-free.
//
// Conventions.  alpha = 0x02.  Symbol p of a word is the coefficient of x^(n-1-p); its locator is X_p = alpha^(prim (n-1-p)).
// Root j is beta_j = alpha^(prim (fcr + j)), so the syndrome S_j = r(beta_j) = sum over the errors of (e X^fcr) X^j.  The
// locator polynomial is Lambda(z) = prod (1 - X z), Lambda_0 = 1, with sum_{c = 0 ... L} Lambda_c S_{r-c} = 0; the
// evaluator Omega = S Lambda mod z^L; an error at X has the value e = Omega(1/X) / Lambda'(1/X) * X^(1 - fcr).
#pragma once
#include <stdint.h>

#include "hz_plan.h"

namespace hz {
namespace rsm {

constexpr uint32_t kOrder = 255;     // the multiplicative group
constexpr uint32_t kExpSize = 512;   // exp[i] = alpha^(i mod 255), i < 512: the sum of two logs needs no reduction
constexpr uint32_t kLogSize = 256;   // log[0] = 0 (never a meaning, always an index inside the table)
constexpr uint32_t kMaxRoots = 64;
constexpr int kFailed = -1;

struct Code {
    uint32_t poly, fcr, prim, nroots, n;
};
HZ_HD uint32_t code_t(const Code &c) { return c.nroots / 2; }
HZ_HD uint32_t code_k(const Code &c) { return c.n - c.nroots; }

// ---- the field ----
// a * alpha (poly has bit 8 set: the xor clears the carry)
HZ_HD uint32_t mulx(uint32_t a, uint32_t poly) {
    a <<= 1;
    return (a & 0x100u) ? (a ^ poly) : a;
}
// a * b, shift and add: no table, no branch on data
HZ_HD uint32_t mul(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r ^= a & (0u - ((b >> i) & 1u));
        a = mulx(a, poly);
    }
    return r;
}
// exp: kExpSize bytes, log: kLogSize bytes -> true when alpha generates all 255 non-zero elements (poly is primitive)
inline bool build_tables(uint32_t poly, uint8_t *exp, uint8_t *log) {
    bool seen[256] = {false};
    uint32_t x = 1, distinct = 0;
    log[0] = 0;
    for (uint32_t i = 0; i < kOrder; i++) {
        if (!seen[x]) seen[x] = true, distinct++;
        exp[i] = (uint8_t)x;
        log[x] = (uint8_t)i;
        x = mulx(x, poly);
    }
    for (uint32_t i = kOrder; i < kExpSize; i++) exp[i] = exp[i - kOrder];
    return distinct == kOrder && x == 1;
}
// 1 / a (a = 0 gives 1: a defined value from inside the table)
HZ_HD uint32_t inv(uint32_t a, const uint8_t *exp, const uint8_t *log) { return exp[kOrder - log[a & 0xffu]]; }

// ---- the multiply by a constant of the syndrome step, in two forms ----
// the eight products x * 2^b, held in registers ...
HZ_HD void products(uint32_t x, uint32_t poly, uint32_t (&P)[8]) {
#pragma unroll
    for (int b = 0; b < 8; b++) P[b] = x, x = mulx(x, poly);
}
// ... selected by the bits of the running value
HZ_HD uint32_t mul_products(uint32_t s, const uint32_t (&P)[8]) {
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) r ^= P[b] & (0u - ((s >> b) & 1u));
    return r;
}
// or through the tables: lx = log x, x not zero
HZ_HD uint32_t mul_log(uint32_t s, uint32_t lx, const uint8_t *exp, const uint8_t *log) { return s ? exp[log[s & 0xffu] + lx] : 0u; }

// ---- the code ----
// log of root j, j < nroots, and log of the locator of position p, p < n (both below 255)
HZ_HD uint32_t root_log(const Code &c, uint32_t j) { return (c.prim * (c.fcr + j)) % kOrder; }
HZ_HD uint32_t locator_log(const Code &c, uint32_t p) { return (c.prim * (c.n - 1u - p)) % kOrder; }
HZ_HD uint32_t neg_log(uint32_t l) { return (kOrder - l) % kOrder; }

// ---- the decoder's steps ----
// Horner: one more received symbol into syndrome j
HZ_HD uint32_t syndrome_step(uint32_t s, uint32_t root, uint32_t v, uint32_t poly) { return mul(s, root, poly) ^ v; }
// Berlekamp-Massey, iteration r, coefficient c: its term of the discrepancy (sv = S_{r-c}, or 0 where c > r) ...
HZ_HD uint32_t bm_term(uint32_t lam, uint32_t sv, uint32_t poly) { return mul(lam, sv, poly); }
// ... and, where the discrepancy d is not zero, the new Lambda_c from B_{c-1} and the B_c of a length change
HZ_HD uint32_t bm_lambda(uint32_t lam, uint32_t d, uint32_t b_shifted, uint32_t poly) { return lam ^ mul(d, b_shifted, poly); }
HZ_HD uint32_t bm_b(uint32_t lam, uint32_t d_inv, uint32_t poly) { return mul(d_inv, lam, poly); }
// Omega_c = sum_{i <= c} Lambda_i S_{c-i}, c < L (lam: at least L entries, syn: at least L)
HZ_HD uint32_t omega_coeff(const uint8_t *lam, const uint8_t *syn, uint32_t c, uint32_t poly) {
    uint32_t o = 0;
    for (uint32_t i = 0; i <= c; i++) o ^= mul(lam[i], syn[c - i], poly);
    return o;
}
// a polynomial of degree deg at z
HZ_HD uint32_t poly_eval(const uint8_t *coef, uint32_t deg, uint32_t z, uint32_t poly) {
    uint32_t acc = coef[deg];
    for (uint32_t c = deg; c-- > 0;) acc = mul(acc, z, poly) ^ coef[c];
    return acc;
}
// Lambda'(z) = sum over odd i of Lambda_i z^(i-1), L >= 1
HZ_HD uint32_t lambda_prime(const uint8_t *lam, uint32_t L, uint32_t z, uint32_t poly) {
    const uint32_t w = mul(z, z, poly);
    uint32_t acc = 0;
    for (uint32_t i = (L & 1u) ? L : L - 1u;; i -= 2) {
        acc = mul(acc, w, poly) ^ lam[i];
        if (i == 1) break;
    }
    return acc;
}
// the error value at the position whose locator has the log xl, 1 <= L (omg: L entries, lam: L + 1)
HZ_HD uint32_t forney(const uint8_t *lam, const uint8_t *omg, uint32_t L, uint32_t xl, const Code &c, const uint8_t *exp, const uint8_t *log) {
    const uint32_t z = exp[neg_log(xl)];
    const uint32_t num = poly_eval(omg, L - 1u, z, c.poly), den = lambda_prime(lam, L, z, c.poly);
    const uint32_t shift = exp[(xl * ((kOrder + 1u - c.fcr) % kOrder)) % kOrder];  // X^(1 - fcr)
    return mul(mul(num, inv(den, exp, log), c.poly), shift, c.poly);
}

// ---- one word, one element after the other ----
// v: n symbols, `step` bytes apart, corrected in place -> the positions changed, or kFailed (v untouched)
inline int decode_word(const Code &c, const uint8_t *exp, const uint8_t *log, uint8_t *v, uint32_t step) {
    const uint32_t t = code_t(c);
    uint8_t syn[kMaxRoots] = {0};
    uint32_t any = 0;
    for (uint32_t j = 0; j < c.nroots; j++) {
        const uint32_t root = exp[root_log(c, j)];
        uint32_t s = 0;
        for (uint32_t p = 0; p < c.n; p++) s = syndrome_step(s, root, v[(size_t)p * step], c.poly);
        syn[j] = (uint8_t)s, any |= s;
    }
    if (!any) return 0;
    uint8_t lam[kMaxRoots + 2] = {1}, B[kMaxRoots + 2] = {1}, next[kMaxRoots + 2];
    uint32_t L = 0;
    for (uint32_t r = 0; r < c.nroots; r++) {
        uint32_t d = 0;
        for (uint32_t i = 0; i <= r && i <= kMaxRoots; i++) d ^= bm_term(lam[i], syn[r - i], c.poly);
        for (uint32_t i = kMaxRoots + 1; i > 0; i--) B[i] = B[i - 1];  // B <- z B
        B[0] = 0;
        if (d) {
            for (uint32_t i = 0; i <= kMaxRoots + 1; i++) next[i] = (uint8_t)bm_lambda(lam[i], d, B[i], c.poly);
            if (2 * L <= r) {
                const uint32_t di = inv(d, exp, log);
                for (uint32_t i = 0; i <= kMaxRoots + 1; i++) B[i] = (uint8_t)bm_b(lam[i], di, c.poly);
                L = r + 1 - L;
            }
            for (uint32_t i = 0; i <= kMaxRoots + 1; i++) lam[i] = next[i];
        }
        if (L > t) return kFailed;
    }
    if (L == 0) return kFailed;  // (syndromes that are not zero give L >= 1; here for the index below alone)
    uint8_t omg[kMaxRoots];
    for (uint32_t i = 0; i < L; i++) omg[i] = (uint8_t)omega_coeff(lam, syn, i, c.poly);
    uint32_t roots = 0, where[kMaxRoots];
    for (uint32_t p = 0; p < c.n; p++) {
        if (poly_eval(lam, L, exp[neg_log(locator_log(c, p))], c.poly) == 0) {
            if (roots < L) where[roots] = p;
            roots++;
        }
    }
    if (roots != L) return kFailed;
    for (uint32_t i = 0; i < L; i++) v[(size_t)where[i] * step] ^= (uint8_t)forney(lam, omg, L, locator_log(c, where[i]), c, exp, log);
    return (int)L;
}

}  // namespace rsm
}  // namespace hz
