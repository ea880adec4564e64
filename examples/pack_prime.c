/* examples/pack.c restated for a PRIME ciphertext modulus on the C ABI (include/cntt_prime_pack.h), behind the bootstrap of
 * examples/pbs_prime.c; no counterpart in the reference: prime64 plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 1024,
 * k = 1, L = 16; bootstrap base_log = 8, levels = 4; packing key base_log = 8, levels = 3 with noise below 2^20.  The program generates
 * a binary LWE key, a binary GLWE key, a NOISELESS bootstrapping key and a NOISY packing key from the flattened GLWE key back to the
 * GLWE key -- row (i, l) = a GLWE encryption of the constant polynomial Sflat[i] 2^(64 - 8 l), mask polynomial first, body last; both
 * keys in the layout the headers fix, n^-1 fwd(key): cntt_prime64_fwd_batch, then cntt_prime64_normalize_batch -- encrypts 8 messages
 * (2 bits under one padding bit, m -> m (p-1)/8), bootstraps them through the look-up table of f in one cntt_prime64_bootstrap_batch
 * call, packs the 8 outputs with cntt_prime64_pack_keyswitch_batch, decrypts the GLWE ciphertext on the host and exits non-zero unless
 * coefficient t reads f(m_t) and every coefficient past the eighth reads 0.  The library generates neither keys nor noise: this file
 * is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_pack.h"

#define P 18446744069414584321ull
#define N 1024u
#define K 1u
#define L 16u
#define BASE_LOG 8u
#define LEVELS 4u
#define PK_BASE_LOG 8u
#define PK_LEVELS 3u
#define COUNT 8u
#define DELTA ((P - 1) / 8) /* one message step; m DELTA = round(m p / 8) for m < 4 */

static uint64_t rng_state = 0x452821E638D01377ull;
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

/* prod[r][c] = mask[r][c] (*) S[c] for `count` rows of K polynomials, in one batched call (skey is scratch of the same size) */
static int products(const cntt_plan64_t *plan, uint64_t *prod, const uint64_t *mask, uint64_t *skey, const uint64_t *S, size_t count) {
    for (size_t r = 0; r < count; ++r)
        for (size_t c = 0; c < K; ++c) memcpy(skey + (r * K + c) * N, S + c * N, N * 8);
    memcpy(prod, mask, count * K * N * 8);
    int rc = cntt_prime64_fwd_batch(plan, skey, count * K, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return rc;
    return cntt_prime64_mul_ntt_batch(plan, prod, skey, count * K, CNTT_MEM_HOST, NULL);
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* bootstrapping key polynomials: key[i][j][o] */
    const size_t big = (size_t)K * N, prows = big * PK_LEVELS, npk = prows * (K + 1);       /* packing key polynomials: K[r][q] at r (K + 1) + q */
    const size_t nmask = (prows > (size_t)L * rows ? prows : (size_t)L * rows) * K;
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *pk = calloc(npk * N, 8);
    uint64_t *mask = malloc(nmask * N * 8), *skey = malloc(nmask * N * 8), *prod = malloc(nmask * N * 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(COUNT * (L + 1) * 8), *lwe_out = calloc(COUNT * (big + 1), 8);
    uint64_t *glwe = calloc((K + 1) * N, 8), *phase = malloc(N * 8);
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* The bootstrapping key of examples/pbs_prime.c: row (q, l) of iteration i is a noiseless GLWE encryption of 0 with
     * s_i 2^(64 - BASE_LOG l) mod p added to coefficient 0 of polynomial q. */
    for (size_t x = 0; x < (size_t)L * rows * K * N; ++x) mask[x] = next_mod_p();
    rc = products(plan, prod, mask, skey, S, (size_t)L * rows);
    if (rc != CNTT_OK) return die("products(bsk)", rc);
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
    rc = cntt_prime64_fwd_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(bsk)", rc);
    rc = cntt_prime64_normalize_batch(plan, key, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(bsk)", rc);

    /* The packing key.  Row r = i PK_LEVELS + (l - 1), i < k n: mask polynomials A_c uniform, body = sum_c A_c S_c + e +
     * Sflat[i] 2^(64 - PK_BASE_LOG l) at coefficient 0, |e| < 2^20 per coefficient; Sflat = the GLWE key, polynomial after polynomial,
     * which is the key the bootstrap's outputs are under. */
    for (size_t x = 0; x < prows * K * N; ++x) mask[x] = next_mod_p();
    rc = products(plan, prod, mask, skey, S, prows);
    if (rc != CNTT_OK) return die("products(pksk)", rc);
    for (size_t i = 0; i < big; ++i)
        for (size_t l = 1; l <= PK_LEVELS; ++l) {
            const size_t r = i * PK_LEVELS + (l - 1);
            uint64_t *row = pk + r * (K + 1) * N; /* K[r][0 .. K] */
            for (size_t x = 0; x < N; ++x) row[K * N + x] = sub_p(next_u64() >> 43, (uint64_t)1 << 20);
            for (size_t c = 0; c < K; ++c) {
                memcpy(row + c * N, mask + (r * K + c) * N, N * 8);
                for (size_t x = 0; x < N; ++x) row[K * N + x] = add_p(row[K * N + x], prod[(r * K + c) * N + x]);
            }
            if (S[i]) row[K * N] = add_p(row[K * N], (uint64_t)1 << (64 - PK_BASE_LOG * l));
        }
    /* the key the call reads: n^-1 fwd(key), as for the bootstrapping key */
    rc = cntt_prime64_fwd_batch(plan, pk, npk, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(pksk)", rc);
    rc = cntt_prime64_normalize_batch(plan, pk, npk, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(pksk)", rc);

    /* the table of examples/pbs_prime.c */
    for (size_t j = 0; j < N; ++j) {
        const size_t t = j + N / 8;
        const uint64_t v = (uint64_t)f((unsigned)((t % N) / (N / 4))) * DELTA;
        lut[K * N + j] = t < N ? v : sub_p(0, v);
    }

    /* message m = t mod 4 under the padding bit: m DELTA, plus noise below 2^40 */
    for (size_t b = 0; b < COUNT; ++b) {
        uint64_t body = add_p((uint64_t)(b & 3) * DELTA, next_u64() >> 24);
        body = sub_p(body, (uint64_t)1 << 39);
        for (size_t i = 0; i < L; ++i) {
            lwe_in[b * (L + 1) + i] = next_mod_p();
            if (s[i]) body = add_p(body, lwe_in[b * (L + 1) + i]);
        }
        lwe_in[b * (L + 1) + L] = body;
    }

    rc = cntt_prime64_bootstrap_batch(plan, lwe_out, lwe_in, lut, 0, key, L, K, BASE_LOG, LEVELS, COUNT, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("bootstrap_batch", rc);
    /* the COUNT outputs, dimension k n under Sflat, are one batch element of the packing keyswitch */
    rc = cntt_prime64_pack_keyswitch_batch(plan, glwe, lwe_out, pk, big, COUNT, K, PK_BASE_LOG, PK_LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("pack_keyswitch_batch", rc);

    /* phase = body - sum_c mask_c S_c in Z_p[X]/(X^n + 1) (S is binary); coefficient t is round(phase / DELTA) mod 8 */
    memcpy(phase, glwe + K * N, N * 8);
    for (size_t c = 0; c < K; ++c)
        for (size_t b = 0; b < N; ++b) {
            if (!S[c * N + b]) continue;
            for (size_t a = 0; a < N; ++a) {
                if (a + b < N) phase[a + b] = sub_p(phase[a + b], glwe[c * N + a]);
                else phase[a + b - N] = add_p(phase[a + b - N], glwe[c * N + a]);
            }
        }
    for (size_t t = 0; t < N; ++t) {
        const unsigned got = phase[t] >= P - DELTA / 2 ? 0u : (unsigned)((phase[t] + DELTA / 2) / DELTA) & 7u;
        const unsigned want = t < COUNT ? f((unsigned)(t & 3)) : 0u;
        if (t < COUNT)
            printf("message %u: f = %u, coefficient %u of the packed GLWE decrypts to %u%s\n", (unsigned)t, want, (unsigned)t, got,
                   got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_prime64_plan_free(plan);
    free(s), free(S), free(key), free(pk), free(mask), free(skey), free(prod), free(lut), free(lwe_in), free(lwe_out), free(glwe), free(phase);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
