/* Two chained table look-ups on the C ABI (include/cntt_ext.h -> cntt_keyswitch.h), no counterpart in the reference: native64 Plan32,
 * n = 1024, k = 1, L = 16; bootstrapping key base_log = 8, levels = 4 (noiseless, as in pbs.c); keyswitch key base_log = 5, levels = 5
 * with noise below 2^20.  The program generates a binary LWE key s, a binary GLWE key S, the bootstrapping key in the layout
 * cntt_pbs.h fixes and the keyswitch key from the flattened GLWE key to s in the layout cntt_keyswitch.h fixes (row (i, l) = an LWE
 * encryption under s of S[i] 2^(64 - 5 l), body last, rows packed), encrypts each of 4 messages (2 bits under one padding bit) under
 * the flattened GLWE key, runs cntt_native_keyswitch_bootstrap_batch TWICE -- the table of f, then the table of g on the first
 * call's output -- decrypts with the flattened GLWE key and exits non-zero unless every message reads g(f(m)).  The library
 * generates neither keys nor noise: this file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
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
#define KS_BASE_LOG 5u
#define KS_LEVELS 5u
#define BATCH 4u
#define NPRIMES 5

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static unsigned f(unsigned m) { return (3u * m + 2u) & 3u; } /* the function the first call evaluates */
static unsigned g(unsigned m) { return (m * m + 1u) & 3u; }  /* ... and the second */

/* The table of fn: a trivial GLWE (zero mask) whose body is X^(-n/8) v0, v0[j] = fn(j / (n/4)) 2^61: boxes of n/4 coefficients,
 * shifted by half a box so that the rounding of the modulus switch stays inside the box of its message. */
static void fill_table(uint64_t *lut, unsigned (*fn)(unsigned)) {
    memset(lut, 0, (K + 1) * N * 8);
    for (size_t j = 0; j < N; ++j) {
        const size_t t = j + N / 8;
        const uint64_t v = (uint64_t)fn((unsigned)((t % N) / (N / 4))) << 61;
        lut[K * N + j] = t < N ? v : (uint64_t)0 - v;
    }
}

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* key polynomials: key[i][j][o] */
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc((size_t)L * rows * K * N * 8), *skey = malloc((size_t)L * rows * K * N * 8);
    uint64_t *prod = malloc((size_t)L * rows * K * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *ct0 = malloc(BATCH * (K * N + 1) * 8), *ct1 = calloc(BATCH * (K * N + 1), 8);
    uint64_t *ct2 = calloc(BATCH * (K * N + 1), 8), *ksk = malloc((size_t)K * N * KS_LEVELS * (L + 1) * 8);
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

    /* The keyswitch key: row i * KS_LEVELS + (l - 1) = (a, <a, s> + S[i] 2^(64 - KS_BASE_LOG l) + e), |e| < 2^20, rows packed */
    for (size_t i = 0; i < K * N; ++i)
        for (size_t l = 1; l <= KS_LEVELS; ++l) {
            uint64_t *row = ksk + (i * KS_LEVELS + (l - 1)) * (L + 1);
            uint64_t body = (S[i] << (64 - KS_BASE_LOG * l)) + (next_u64() >> 44) - ((uint64_t)1 << 19);
            for (size_t c = 0; c < L; ++c) {
                row[c] = next_u64();
                body += row[c] * s[c];
            }
            row[L] = body;
        }

    /* message m under the padding bit, encrypted under the flattened GLWE key: m 2^61, plus noise below 2^40 */
    for (size_t b = 0; b < BATCH; ++b) {
        uint64_t *ct = ct0 + b * (K * N + 1);
        uint64_t body = ((uint64_t)b << 61) + (next_u64() >> 24) - ((uint64_t)1 << 39);
        for (size_t i = 0; i < K * N; ++i) {
            ct[i] = next_u64();
            body += ct[i] * S[i];
        }
        ct[K * N] = body;
    }

    /* f, then g on its output: the call takes and returns ciphertexts of dimension k n, so it chains with itself */
    fill_table(lut, f);
    rc = cntt_native_keyswitch_bootstrap_batch(plan, ct1, ct0, ksk, L + 1, KS_BASE_LOG, KS_LEVELS, lut, 0, bsk, L, K, BASE_LOG, LEVELS, BATCH,
                                               NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("keyswitch_bootstrap_batch (f)", rc);
    fill_table(lut, g);
    rc = cntt_native_keyswitch_bootstrap_batch(plan, ct2, ct1, ksk, L + 1, KS_BASE_LOG, KS_LEVELS, lut, 0, bsk, L, K, BASE_LOG, LEVELS, BATCH,
                                               NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("keyswitch_bootstrap_batch (g)", rc);

    /* phase = body - <mask, flattened GLWE key>; the message is its top 3 bits, rounded */
    for (size_t b = 0; b < BATCH; ++b) {
        const uint64_t *ct = ct2 + b * (K * N + 1);
        uint64_t phase = ct[K * N];
        for (size_t i = 0; i < K * N; ++i) phase -= ct[i] * S[i];
        const unsigned got = (unsigned)(((phase >> 60) + 1) >> 1) & 7u, want = g(f((unsigned)b));
        printf("message %u: g(f(m)) = %u, two chained calls decrypt to %u%s\n", (unsigned)b, want, got, got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_native_plan_free(plan);
    for (int i = 0; i < NPRIMES; ++i) free(planes[i]);
    free(s), free(S), free(key), free(mask), free(skey), free(prod), free(lut), free(ct0), free(ct1), free(ct2), free(ksk);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
