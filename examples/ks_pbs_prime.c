/* examples/ks_pbs.c restated for a PRIME ciphertext modulus on the C ABI (include/cntt_prime_keyswitch.h), no counterpart in the
 * reference: prime64 plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 1024, k = 1, L = 16; bootstrapping key base_log = 8,
 * levels = 4 (noiseless, as in pbs_prime.c); keyswitch key base_log = 5, levels = 5 with noise below 2^20.  The program generates a
 * binary LWE key s, a binary GLWE key S, the bootstrapping key in the layout cntt_prime_pbs.h fixes and the keyswitch key from the
 * flattened GLWE key to s in the layout cntt_prime_keyswitch.h fixes (row (i, l) = an LWE encryption under s of S[i] 2^(64 - 5 l) mod p,
 * body last, rows packed), encrypts each of 4 messages (2 bits under one padding bit, m -> m (p-1)/8) under the flattened GLWE key, runs
 * cntt_prime64_keyswitch_bootstrap_batch TWICE -- the table of f, then the table of g on the first call's output -- decrypts with the
 * flattened GLWE key and exits non-zero unless every message reads g(f(m)).  The library generates neither keys nor noise: this file is
 * the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_keyswitch.h"

#define P 18446744069414584321ull
#define N 1024u
#define K 1u
#define L 16u
#define BASE_LOG 8u
#define LEVELS 4u
#define KS_BASE_LOG 5u
#define KS_LEVELS 5u
#define BATCH 4u
#define DELTA ((P - 1) / 8) /* one message step; m DELTA = round(m p / 8) for m < 4 */

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

static unsigned f(unsigned m) { return (3u * m + 2u) & 3u; } /* the function the first call evaluates */
static unsigned g(unsigned m) { return (m * m + 1u) & 3u; }  /* ... and the second */

/* The table of fn: a trivial GLWE (zero mask) whose body is X^(-n/8) v0, v0[j] = fn(j / (n/4)) DELTA: boxes of n/4 coefficients, shifted
 * by half a box so that the rounding of the modulus switch stays inside the box of its message. */
static void fill_table(uint64_t *lut, unsigned (*fn)(unsigned)) {
    memset(lut, 0, (K + 1) * N * 8);
    for (size_t j = 0; j < N; ++j) {
        const size_t t = j + N / 8;
        const uint64_t v = (uint64_t)fn((unsigned)((t % N) / (N / 4))) * DELTA;
        lut[K * N + j] = t < N ? v : sub_p(0, v);
    }
}

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* key polynomials: key[i][j][o] */
    const size_t nprod = (size_t)L * rows * K;
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc(nprod * N * 8), *skey = malloc(nprod * N * 8), *prod = malloc(nprod * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *ct0 = malloc(BATCH * (K * N + 1) * 8), *ct1 = calloc(BATCH * (K * N + 1), 8);
    uint64_t *ct2 = calloc(BATCH * (K * N + 1), 8), *ksk = malloc((size_t)K * N * KS_LEVELS * (L + 1) * 8);
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row (q, l) of iteration i: a fresh GLWE encryption of 0 -- mask A uniform, body sum_c A_c S_c, no noise -- with
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

    /* The keyswitch key: row i * KS_LEVELS + (l - 1) = (a, <a, s> + S[i] 2^(64 - KS_BASE_LOG l) + e mod p), |e| < 2^20, rows packed */
    for (size_t i = 0; i < K * N; ++i)
        for (size_t l = 1; l <= KS_LEVELS; ++l) {
            uint64_t *row = ksk + (i * KS_LEVELS + (l - 1)) * (L + 1);
            uint64_t body = sub_p(add_p(S[i] << (64 - KS_BASE_LOG * l), next_u64() >> 44), (uint64_t)1 << 19);
            for (size_t c = 0; c < L; ++c) {
                row[c] = next_mod_p();
                if (s[c]) body = add_p(body, row[c]);
            }
            row[L] = body;
        }

    /* message m under the padding bit, encrypted under the flattened GLWE key: m DELTA, plus noise below 2^40 */
    for (size_t b = 0; b < BATCH; ++b) {
        uint64_t *ct = ct0 + b * (K * N + 1);
        uint64_t body = sub_p(add_p((uint64_t)b * DELTA, next_u64() >> 24), (uint64_t)1 << 39);
        for (size_t i = 0; i < K * N; ++i) {
            ct[i] = next_mod_p();
            if (S[i]) body = add_p(body, ct[i]);
        }
        ct[K * N] = body;
    }

    /* f, then g on its output: the call takes and returns ciphertexts of dimension k n, so it chains with itself */
    fill_table(lut, f);
    rc = cntt_prime64_keyswitch_bootstrap_batch(plan, ct1, ct0, ksk, L + 1, KS_BASE_LOG, KS_LEVELS, lut, 0, key, L, K, BASE_LOG, LEVELS, BATCH,
                                                NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("keyswitch_bootstrap_batch (f)", rc);
    fill_table(lut, g);
    rc = cntt_prime64_keyswitch_bootstrap_batch(plan, ct2, ct1, ksk, L + 1, KS_BASE_LOG, KS_LEVELS, lut, 0, key, L, K, BASE_LOG, LEVELS, BATCH,
                                                NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("keyswitch_bootstrap_batch (g)", rc);

    /* phase = body - <mask, flattened GLWE key> mod p; the message is round(phase / DELTA) mod 8 */
    for (size_t b = 0; b < BATCH; ++b) {
        const uint64_t *ct = ct2 + b * (K * N + 1);
        uint64_t phase = ct[K * N];
        for (size_t i = 0; i < K * N; ++i)
            if (S[i]) phase = sub_p(phase, ct[i]);
        const unsigned got = phase >= P - DELTA / 2 ? 0u : (unsigned)((phase + DELTA / 2) / DELTA) & 7u, want = g(f((unsigned)b));
        printf("message %u: g(f(m)) = %u, two chained calls decrypt to %u%s\n", (unsigned)b, want, got, got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_prime64_plan_free(plan);
    free(s), free(S), free(key), free(mask), free(skey), free(prod), free(lut), free(ct0), free(ct1), free(ct2), free(ksk);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
