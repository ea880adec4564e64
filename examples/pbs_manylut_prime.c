/* examples/pbs_prime.c with several look-up tables per bootstrap (include/cntt_prime_manylut.h), no counterpart in the reference: prime64
 * plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 1024, k = 1, L = 16, base_log = 8, levels = 4, log_lut_count = 2.  The
 * program generates a binary LWE key, a binary GLWE key and a NOISY bootstrapping key (|e| < 2^4 in every row) in the layout
 * cntt_prime_pbs.h fixes, encrypts each of the 8 messages of a 3-bit space under one padding bit (m -> m (p-1)/16, noise below 2^40),
 * and evaluates 2^2 = 4 different functions of every message in ONE cntt_prime64_bootstrap_manylut_batch call: the modulus switch keeps
 * multiples of 4, function h lives at the coefficients 4 c + h of the table and comes out at the extraction index h.  Every one of the
 * 32 outputs is decrypted with the flattened GLWE key; the program exits non-zero on a wrong one.  A message has a box of n / 4 / 8 = 32
 * steps of the coarse switch, shifted by half a box; the switch drifts by at most (L + 1) / 2 = 8.5 of them.  The library generates
 * neither keys nor noise: this file is the recipe.  Host buffers throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_manylut.h"

#define P 18446744069414584321ull
#define N 1024u
#define K 1u
#define L 16u
#define BASE_LOG 8u
#define LEVELS 4u
#define LOG_LUTS 2u
#define LUTS (1u << LOG_LUTS)
#define BATCH 8u
#define DELTA ((P - 1) / 16) /* one message step; m DELTA = round(m p / 16) for m < 8 */

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

static unsigned f(unsigned h, unsigned m) { return (m * (2u * h + 1u) + h) & 7u; } /* function h of the one bootstrap */

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* key polynomials: key[i][j][o] */
    const size_t nprod = (size_t)L * rows * K;
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc(nprod * N * 8), *skey = malloc(nprod * N * 8), *prod = malloc(nprod * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(BATCH * (L + 1) * 8), *lwe_out = calloc(BATCH * LUTS * (K * N + 1), 8);
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row (q, l) of iteration i: a fresh GLWE encryption of 0 -- mask A uniform, body sum_c A_c S_c + e, |e| < 2^4 -- with
     * s_i 2^(64 - BASE_LOG l) mod p added to coefficient 0 of polynomial q.  All products A_c S_c in one batched call:
     * cntt_prime64_mul_ntt_batch multiplies by the polynomial whose forward transform it is given. */
    for (size_t r = 0; r < (size_t)L * rows; ++r)
        for (size_t c = 0; c < K; ++c) {
            for (size_t x = 0; x < N; ++x) mask[(r * K + c) * N + x] = next_mod_p();
            memcpy(skey + (r * K + c) * N, S + c * N, N * 8);
        }
    memcpy(prod, mask, nprod * N * 8);
    rc = cntt_prime64_fwd_batch(plan, skey, nprod, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(S)", rc);
    rc = cntt_prime64_mul_ntt_batch(plan, prod, skey, nprod, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("mul_ntt_batch", rc);
    for (size_t i = 0; i < L; ++i)
        for (size_t q = 0; q <= K; ++q)
            for (size_t l = 1; l <= LEVELS; ++l) {
                const size_t j = q * LEVELS + (l - 1), r = i * rows + j;
                uint64_t *row = key + (i * slice + j * (K + 1)) * N; /* key[j][0 .. K] */
                for (size_t x = 0; x < N; ++x) row[K * N + x] = sub_p(next_u64() & 15, 8); /* the noise: -8 .. 7 */
                for (size_t c = 0; c < K; ++c) {
                    memcpy(row + c * N, mask + (r * K + c) * N, N * 8);
                    for (size_t x = 0; x < N; ++x) row[K * N + x] = add_p(row[K * N + x], prod[(r * K + c) * N + x]);
                }
                if (s[i]) row[q * N] = add_p(row[q * N], (uint64_t)1 << (64 - BASE_LOG * l)); /* 2^(W - BASE_LOG l) < p as it stands */
            }
    /* the key the blind rotation reads: n^-1 fwd(key), because the fused chain returns the unnormalised inverse transform */
    rc = cntt_prime64_fwd_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(key)", rc);
    rc = cntt_prime64_normalize_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(key)", rc);

    /* The table: a trivial GLWE (zero mask) whose body holds function h at the coefficients 4 c + h: per function n / 4 = 256 coarse
     * steps, boxes of 32 steps per message, shifted by half a box so that the rounding of the modulus switch stays inside the box. */
    for (size_t j = 0; j < N; ++j) {
        const size_t c = j >> LOG_LUTS, np = N >> LOG_LUTS, t = c + np / 16;
        const uint64_t v = (uint64_t)f((unsigned)(j & (LUTS - 1)), (unsigned)((t % np) / (np / 8))) * DELTA;
        lut[K * N + j] = t < np ? v : sub_p(0, v);
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

    rc = cntt_prime64_bootstrap_manylut_batch(plan, lwe_out, lwe_in, lut, 0, key, L, K, BASE_LOG, LEVELS, LOG_LUTS, LUTS, BATCH, NULL, 0,
                                              CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("bootstrap_manylut_batch", rc);

    /* output (b, h) at lwe_out[(b LUTS + h) (k n + 1)]: phase = body - <mask, flattened GLWE key> mod p; the message is
     * round(phase / DELTA) mod 16 */
    for (size_t b = 0; b < BATCH; ++b) {
        printf("message %u:", (unsigned)b);
        for (unsigned h = 0; h < LUTS; ++h) {
            const uint64_t *ct = lwe_out + (b * LUTS + h) * (K * N + 1);
            uint64_t phase = ct[K * N];
            for (size_t i = 0; i < K * N; ++i)
                if (S[i]) phase = sub_p(phase, ct[i]);
            const unsigned got = phase >= P - DELTA / 2 ? 0u : (unsigned)((phase + DELTA / 2) / DELTA) & 15u;
            printf(" f%u = %u -> %u%s", h, f(h, (unsigned)b), got, got == f(h, (unsigned)b) ? "" : "  WRONG");
            wrong += got != f(h, (unsigned)b);
        }
        printf("\n");
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
