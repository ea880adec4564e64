/* examples/pbs.c with the MULTI-BIT blind rotation (include/cntt_multibit.h), no counterpart in the reference: native64 Plan32 (ciphertext
 * modulus 2^64), n = 1024, k = 1, L = 12, base_log = 8, levels = 4, once with grouping g = 2 (6 groups of 4 GGSW ciphertexts) and once
 * with g = 3 (4 groups of 8).  The program generates a binary LWE key, a binary GLWE key and, per grouping, the bundled bootstrapping
 * key in the layout the header fixes: key (r, t) is the GGSW ciphertext of [t == the secret bits of group r] (bit i of t belongs to mask
 * word r g + i), every row a GLWE encryption with noise below 2^10, stored as the residue planes cntt_native_fwd_batch writes.  It
 * encrypts each of 4 messages (2 bits under one padding bit), bootstraps them through the look-up table of f in one
 * cntt_native_multibit_bootstrap_batch call, decrypts with the flattened GLWE key and exits non-zero on a wrong message.  The library
 * generates neither keys nor noise: this file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_multibit.h"

#define N 1024u
#define K 1u
#define L 12u
#define BASE_LOG 8u
#define LEVELS 4u
#define BATCH 4u
#define NPRIMES 5

static uint64_t rng_state = 0xA4093822299F31D0ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static unsigned f(unsigned m) { return (3u * m + 2u) & 3u; } /* the function the bootstrap evaluates */

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

/* one bootstrap of the four messages with grouping g; returns the number of wrong messages, or -1 after an error */
static int run(const cntt_native_t *plan, unsigned g, const uint64_t *s, const uint64_t *S, const uint64_t *lut, const uint64_t *lwe_in) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), npat = (size_t)1 << g, ngroups = L / g;
    const size_t nggsw = ngroups * npat, nkey = nggsw * slice; /* key polynomials: key[r][t][j][o] */
    const size_t nprod = nggsw * rows * K;
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc(nprod * N * 8), *skey = malloc(nprod * N * 8), *prod = malloc(nprod * N * 8);
    uint64_t *lwe_out = calloc(BATCH * (K * N + 1), 8);
    uint32_t *planes[NPRIMES];
    const void *bsk[NPRIMES];
    void *res[NPRIMES];
    int rc, wrong = 0;

    /* Row (q, l) of GGSW ciphertext (r, t): a fresh GLWE encryption of 0 -- mask A uniform, body sum_c A_c S_c + e, |e| < 2^10 -- with
     * 2^(64 - BASE_LOG l) added to coefficient 0 of polynomial q when t is the pattern of the group's secret bits, i.e. when
     * prod_{i in t} s_i prod_{i not in t} (1 - s_i) = 1.  All products A_c S_c in one batched call. */
    for (size_t r = 0; r < nggsw * rows; ++r)
        for (size_t c = 0; c < K; ++c) {
            for (size_t x = 0; x < N; ++x) mask[(r * K + c) * N + x] = next_u64();
            memcpy(skey + (r * K + c) * N, S + c * N, N * 8);
        }
    rc = cntt_native_negacyclic_polymul_batch(plan, prod, mask, skey, nprod, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("negacyclic_polymul_batch", rc), -1;
    for (size_t gi = 0; gi < ngroups; ++gi) {
        size_t pattern = 0;
        for (size_t i = 0; i < g; ++i) pattern |= (size_t)s[gi * g + i] << i; /* bit i of t: mask word gi g + i */
        for (size_t t = 0; t < npat; ++t)
            for (size_t q = 0; q <= K; ++q)
                for (size_t l = 1; l <= LEVELS; ++l) {
                    const size_t w = gi * npat + t, j = q * LEVELS + (l - 1), r = w * rows + j;
                    uint64_t *row = key + (w * slice + j * (K + 1)) * N; /* key[r][t][j][0 .. K] */
                    for (size_t c = 0; c < K; ++c) {
                        memcpy(row + c * N, mask + (r * K + c) * N, N * 8);
                        for (size_t x = 0; x < N; ++x) row[K * N + x] += prod[(r * K + c) * N + x];
                    }
                    for (size_t x = 0; x < N; ++x) row[K * N + x] += (next_u64() >> 53) - ((uint64_t)1 << 10);
                    if (t == pattern) row[q * N] += (uint64_t)1 << (64 - BASE_LOG * l);
                }
    }
    /* the key the blind rotation reads: the residue planes of fwd(key), not normalised */
    for (int i = 0; i < NPRIMES; ++i) {
        planes[i] = malloc(nkey * N * 4);
        res[i] = planes[i];
        bsk[i] = planes[i];
    }
    rc = cntt_native_fwd_batch(plan, key, res, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(key)", rc), -1;

    rc = cntt_native_multibit_bootstrap_batch(plan, lwe_out, lwe_in, lut, 0, bsk, L, K, BASE_LOG, LEVELS, g, BATCH, NULL, 0, CNTT_MEM_HOST,
                                              NULL);
    if (rc != CNTT_OK) return die("multibit_bootstrap_batch", rc), -1;

    /* phase = body - <mask, flattened GLWE key>; the message is its top 3 bits, rounded */
    for (size_t b = 0; b < BATCH; ++b) {
        const uint64_t *ct = lwe_out + b * (K * N + 1);
        uint64_t phase = ct[K * N];
        for (size_t i = 0; i < K * N; ++i) phase -= ct[i] * S[i];
        const unsigned got = (unsigned)(((phase >> 60) + 1) >> 1) & 7u;
        printf("g = %u, message %u: f = %u, bootstrap decrypts to %u%s\n", g, (unsigned)b, f((unsigned)b), got,
               got == f((unsigned)b) ? "" : "  WRONG");
        wrong += got != f((unsigned)b);
    }
    for (int i = 0; i < NPRIMES; ++i) free(planes[i]);
    free(key), free(mask), free(skey), free(prod), free(lwe_out);
    return wrong;
}

int main(void) {
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(BATCH * (L + 1) * 8);
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES) return die("nprimes", -1);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* The table: a trivial GLWE (zero mask) whose body is X^(-n/8) v0, v0[j] = f(j / (n/4)) 2^61: boxes of n/4 coefficients, shifted
     * by half a box so that the rounding of the modulus switch stays inside the box of its message. */
    for (size_t j = 0; j < N; ++j) {
        const size_t t = j + N / 8;
        const uint64_t v = (uint64_t)f((unsigned)((t % N) / (N / 4))) << 61;
        lut[K * N + j] = t < N ? v : (uint64_t)0 - v;
    }

    /* message m under the padding bit: m 2^61, plus noise below 2^40 */
    for (size_t b = 0; b < BATCH; ++b) {
        uint64_t body = ((uint64_t)b << 61) + (next_u64() >> 24) - ((uint64_t)1 << 39);
        for (size_t i = 0; i < L; ++i) {
            lwe_in[b * (L + 1) + i] = next_u64();
            body += lwe_in[b * (L + 1) + i] * s[i];
        }
        lwe_in[b * (L + 1) + L] = body;
    }

    for (unsigned g = 2; g <= 3; ++g) {
        const int w = run(plan, g, s, S, lut, lwe_in);
        if (w < 0) return 1;
        wrong += w;
    }
    cntt_native_plan_free(plan);
    free(s), free(S), free(lut), free(lwe_in);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
