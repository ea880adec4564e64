/* A TFHE programmable bootstrap on the C ABI (include/cntt_ext.h -> cntt_pbs.h), no counterpart in the reference: native64 Plan32,
 * n = 1024, k = 1, L = 16, base_log = 8, levels = 4.  The program generates a binary LWE key, a binary GLWE key and a NOISELESS
 * bootstrapping key in the layout cntt_pbs.h fixes, encrypts each of 4 messages (2 bits under one padding bit), bootstraps them
 * through the look-up table of f in one cntt_native_bootstrap_batch call, decrypts with the flattened GLWE key and exits non-zero on a
 * wrong message.  The library generates neither keys nor noise: this file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_ext.h"

#define N 1024u
#define K 1u
#define L 16u
#define BASE_LOG 8u
#define LEVELS 4u
#define BATCH 4u
#define NPRIMES 5

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* key polynomials: key[i][j][o] */
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc((size_t)L * rows * K * N * 8), *skey = malloc((size_t)L * rows * K * N * 8);
    uint64_t *prod = malloc((size_t)L * rows * K * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(BATCH * (L + 1) * 8), *lwe_out = calloc(BATCH * (K * N + 1), 8);
    uint32_t *planes[NPRIMES];
    const void *bsk[NPRIMES];
    void *res[NPRIMES];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES) return die("nprimes", -1);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row (p, l) of iteration i: a fresh GLWE encryption of 0 -- mask A uniform, body sum_q A_q S_q, no noise -- with
     * s_i 2^(64 - BASE_LOG l) added to coefficient 0 of polynomial p.  All products A_q S_q in one batched call. */
    for (size_t r = 0; r < (size_t)L * rows; ++r)
        for (size_t q = 0; q < K; ++q) {
            for (size_t c = 0; c < N; ++c) mask[(r * K + q) * N + c] = next_u64();
            memcpy(skey + (r * K + q) * N, S + q * N, N * 8);
        }
    rc = cntt_native_negacyclic_polymul_batch(plan, prod, mask, skey, (size_t)L * rows * K, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("negacyclic_polymul_batch", rc);
    for (size_t i = 0; i < L; ++i)
        for (size_t p = 0; p <= K; ++p)
            for (size_t l = 1; l <= LEVELS; ++l) {
                const size_t j = p * LEVELS + (l - 1), r = i * rows + j;
                uint64_t *row = key + (i * slice + j * (K + 1)) * N; /* key[j][0 .. K] */
                for (size_t q = 0; q < K; ++q) {
                    memcpy(row + q * N, mask + (r * K + q) * N, N * 8);
                    for (size_t c = 0; c < N; ++c) row[K * N + c] += prod[(r * K + q) * N + c];
                }
                row[p * N] += s[i] << (64 - BASE_LOG * l);
            }
    for (int i = 0; i < NPRIMES; ++i) {
        planes[i] = malloc(nkey * N * 4);
        res[i] = planes[i];
        bsk[i] = planes[i];
    }
    rc = cntt_native_fwd_batch(plan, key, res, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch", rc);

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

    rc = cntt_native_bootstrap_batch(plan, lwe_out, lwe_in, lut, 0, bsk, L, K, BASE_LOG, LEVELS, BATCH, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("bootstrap_batch", rc);

    /* phase = body - <mask, flattened GLWE key>; the message is its top 3 bits, rounded */
    for (size_t b = 0; b < BATCH; ++b) {
        const uint64_t *ct = lwe_out + b * (K * N + 1);
        uint64_t phase = ct[K * N];
        for (size_t i = 0; i < K * N; ++i) phase -= ct[i] * S[i];
        const unsigned got = (unsigned)(((phase >> 60) + 1) >> 1) & 7u;
        printf("message %u: f = %u, bootstrap decrypts to %u%s\n", (unsigned)b, f((unsigned)b), got, got == f((unsigned)b) ? "" : "  WRONG");
        wrong += got != f((unsigned)b);
    }
    cntt_native_plan_free(plan);
    for (int i = 0; i < NPRIMES; ++i) free(planes[i]);
    free(s), free(S), free(key), free(mask), free(skey), free(prod), free(lut), free(lwe_in), free(lwe_out);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
