/* examples/pbs_prime.c with the MULTI-BIT blind rotation (include/cntt_prime_multibit.h), no counterpart in the reference: prime64 plan,
 * p = 2^64 - 2^32 + 1 (W = 64), n = 1024, k = 1, L = 16, grouping g = 2 (8 groups of 4 GGSW ciphertexts), base_log = 8, levels = 4.  The
 * program generates a binary LWE key, a binary GLWE key and the bundled bootstrapping key in the layout the header fixes: key (r, t) is
 * the GGSW ciphertext of [t == the secret bits of group r] (bit i of t belongs to mask word r g + i), every row a GLWE encryption with
 * noise below 2^10, stored as n^-1 fwd(key).  It encrypts each of 4 messages (2 bits under one padding bit), bootstraps them through the
 * look-up table of f in one cntt_prime64_multibit_bootstrap_batch call, decrypts with the flattened GLWE key and exits non-zero on a
 * wrong message.  The library generates neither keys nor noise: this file is the recipe.  Host buffers throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_multibit.h"

#define P 18446744069414584321ull
#define N 1024u
#define K 1u
#define L 16u
#define G 2u
#define BASE_LOG 8u
#define LEVELS 4u
#define BATCH 4u
#define DELTA ((P - 1) / 8) /* one message step; m DELTA = round(m p / 8) for m < 4 */

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t next_mod_p(void) { /* uniform below p by rejection */
    uint64_t x;
    do x = next_u64();
    while (x >= P);
    return x;
}
static uint64_t add_p(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a || s >= P ? s - P : s;
}
static uint64_t sub_p(uint64_t a, uint64_t b) { return a >= b ? a - b : a - b + P; }

static unsigned f(unsigned m) { return (3u * m + 2u) & 3u; } /* the function the bootstrap evaluates */

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), npat = (size_t)1 << G, ngroups = L / G;
    const size_t nggsw = ngroups * npat, nkey = nggsw * slice; /* key polynomials: key[r][t][j][o] */
    const size_t nprod = nggsw * rows * K;
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc(nprod * N * 8), *skey = malloc(nprod * N * 8), *prod = malloc(nprod * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(BATCH * (L + 1) * 8), *lwe_out = calloc(BATCH * (K * N + 1), 8);
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row (q, l) of GGSW ciphertext (r, t): a fresh GLWE encryption of 0 -- mask A uniform, body sum_c A_c S_c + e, |e| < 2^10 -- with
     * 2^(64 - BASE_LOG l) mod p added to coefficient 0 of polynomial q when t is the pattern of the group's secret bits.  All products
     * A_c S_c in one batched call. */
    for (size_t r = 0; r < nggsw * rows; ++r)
        for (size_t c = 0; c < K; ++c) {
            for (size_t x = 0; x < N; ++x) mask[(r * K + c) * N + x] = next_mod_p();
            memcpy(skey + (r * K + c) * N, S + c * N, N * 8);
        }
    memcpy(prod, mask, nprod * N * 8);
    rc = cntt_prime64_fwd_batch(plan, skey, nprod, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(S)", rc);
    rc = cntt_prime64_mul_ntt_batch(plan, prod, skey, nprod, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("mul_ntt_batch", rc);
    for (size_t gi = 0; gi < ngroups; ++gi) {
        size_t pattern = 0;
        for (size_t i = 0; i < G; ++i) pattern |= (size_t)s[gi * G + i] << i; /* bit i of t: mask word gi g + i */
        for (size_t t = 0; t < npat; ++t)
            for (size_t q = 0; q <= K; ++q)
                for (size_t l = 1; l <= LEVELS; ++l) {
                    const size_t w = gi * npat + t, j = q * LEVELS + (l - 1), r = w * rows + j;
                    uint64_t *row = key + (w * slice + j * (K + 1)) * N; /* key[r][t][j][0 .. K] */
                    for (size_t c = 0; c < K; ++c) {
                        memcpy(row + c * N, mask + (r * K + c) * N, N * 8);
                        for (size_t x = 0; x < N; ++x) row[K * N + x] = add_p(row[K * N + x], prod[(r * K + c) * N + x]);
                    }
                    for (size_t x = 0; x < N; ++x) row[K * N + x] = sub_p(add_p(row[K * N + x], next_u64() >> 53), (uint64_t)1 << 10);
                    if (t == pattern) row[q * N] = add_p(row[q * N], (uint64_t)1 << (64 - BASE_LOG * l));
                }
    }
    /* the key the blind rotation reads: n^-1 fwd(key) */
    rc = cntt_prime64_fwd_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(key)", rc);
    rc = cntt_prime64_normalize_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(key)", rc);

    /* The table: a trivial GLWE (zero mask) whose body is X^(-n/8) v0, v0[j] = f(j / (n/4)) DELTA: boxes of n/4 coefficients, shifted
     * by half a box so that the rounding of the modulus switch stays inside the box of its message. */
    for (size_t j = 0; j < N; ++j) {
        const size_t t = j + N / 8;
        const uint64_t v = (uint64_t)f((unsigned)((t % N) / (N / 4))) * DELTA;
        lut[K * N + j] = t < N ? v : sub_p(0, v);
    }

    /* message m under the padding bit: m DELTA, plus noise below 2^40 */
    for (size_t b = 0; b < BATCH; ++b) {
        uint64_t body = add_p((uint64_t)b * DELTA, next_u64() >> 24);
        body = sub_p(body, (uint64_t)1 << 39);
        for (size_t i = 0; i < L; ++i) {
            lwe_in[b * (L + 1) + i] = next_mod_p();
            if (s[i]) body = add_p(body, lwe_in[b * (L + 1) + i]);
        }
        lwe_in[b * (L + 1) + L] = body;
    }

    rc = cntt_prime64_multibit_bootstrap_batch(plan, lwe_out, lwe_in, lut, 0, key, L, K, BASE_LOG, LEVELS, G, BATCH, NULL, 0, CNTT_MEM_HOST,
                                               NULL);
    if (rc != CNTT_OK) return die("multibit_bootstrap_batch", rc);

    /* phase = body - <mask, flattened GLWE key> mod p; the message is round(phase / DELTA) mod 8 */
    for (size_t b = 0; b < BATCH; ++b) {
        const uint64_t *ct = lwe_out + b * (K * N + 1);
        uint64_t phase = ct[K * N];
        for (size_t i = 0; i < K * N; ++i)
            if (S[i]) phase = sub_p(phase, ct[i]);
        const unsigned got = phase >= P - DELTA / 2 ? 0u : (unsigned)((phase + DELTA / 2) / DELTA) & 7u;
        printf("message %u: f = %u, bootstrap decrypts to %u%s\n", (unsigned)b, f((unsigned)b), got, got == f((unsigned)b) ? "" : "  WRONG");
        wrong += got != f((unsigned)b);
    }
    cntt_prime64_plan_free(plan);
    free(s), free(S), free(key), free(mask), free(skey), free(prod), free(lut), free(lwe_in), free(lwe_out);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
