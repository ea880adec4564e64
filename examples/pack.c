/* LWE ciphertexts packed into one GLWE ciphertext on the C ABI (include/cntt_ext.h -> cntt_pack.h), no counterpart in the reference:
 * native64 Plan32, n = 256, k = 1, binary keys; LWE dimension 32; packing key base_log = 4, levels = 6 with noise below 2^20.  The
 * program generates a binary LWE key s and a binary GLWE key S, the packing keyswitch key in the layout cntt_pack.h fixes (row (i, l)
 * = a GLWE encryption under S of the constant polynomial s[i] 2^(64 - 4 l), mask polynomial first, body last; all rows through ONE
 * cntt_native_fwd_batch), encrypts 8 messages (3 bits under the top of the word, noise below 2^40) as LWE ciphertexts under s, packs
 * them with cntt_native_pack_keyswitch_batch, decrypts the GLWE ciphertext on the host and exits non-zero unless coefficient t reads
 * message t and every coefficient past the last message reads 0.  The library generates neither keys nor noise: this file is the
 * recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_ext.h"

#define N 256u
#define K 1u
#define LIN 32u
#define BASE_LOG 4u
#define LEVELS 6u
#define COUNT 8u
#define NPRIMES 5

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

int main(void) {
    const size_t rows = (size_t)LIN * LEVELS, nkey = rows * (K + 1); /* key polynomials: K[r][p] at r (K + 1) + p */
    uint64_t *s = malloc(LIN * 8), *S = malloc(K * N * 8);
    uint64_t *key = calloc(nkey * N, 8), *mask = malloc(rows * K * N * 8), *skey = malloc(rows * K * N * 8), *prod = malloc(rows * K * N * 8);
    uint64_t *lwe = malloc(COUNT * (LIN + 1) * 8), *glwe = calloc((K + 1) * N, 8), *phase = malloc(N * 8);
    uint32_t *planes[NPRIMES];
    const void *pksk[NPRIMES];
    void *res[NPRIMES];
    unsigned msg[COUNT];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES) return die("nprimes", -1);

    for (size_t i = 0; i < LIN; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row r = i LEVELS + (l - 1): mask polynomials A_q uniform, body = sum_q A_q S_q + e + s[i] 2^(64 - BASE_LOG l) at coefficient 0,
     * |e| < 2^20 per coefficient.  All products A_q S_q in one batched call. */
    for (size_t r = 0; r < rows; ++r)
        for (size_t q = 0; q < K; ++q) {
            for (size_t c = 0; c < N; ++c) mask[(r * K + q) * N + c] = next_u64();
            memcpy(skey + (r * K + q) * N, S + q * N, N * 8);
        }
    rc = cntt_native_negacyclic_polymul_batch(plan, prod, mask, skey, rows * K, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("negacyclic_polymul_batch", rc);
    for (size_t i = 0; i < LIN; ++i)
        for (size_t l = 1; l <= LEVELS; ++l) {
            const size_t r = i * LEVELS + (l - 1);
            uint64_t *row = key + r * (K + 1) * N; /* K[r][0 .. K] */
            for (size_t c = 0; c < N; ++c) row[K * N + c] = (next_u64() >> 43) - ((uint64_t)1 << 20);
            for (size_t q = 0; q < K; ++q) {
                memcpy(row + q * N, mask + (r * K + q) * N, N * 8);
                for (size_t c = 0; c < N; ++c) row[K * N + c] += prod[(r * K + q) * N + c];
            }
            row[K * N] += s[i] << (64 - BASE_LOG * l);
        }
    for (int i = 0; i < NPRIMES; ++i) {
        planes[i] = malloc(nkey * N * 4);
        res[i] = planes[i];
        pksk[i] = planes[i];
    }
    rc = cntt_native_fwd_batch(plan, key, res, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch", rc);

    /* message m at the top three bits, encrypted under s: m 2^61, plus noise below 2^40 */
    for (size_t t = 0; t < COUNT; ++t) {
        uint64_t *ct = lwe + t * (LIN + 1);
        msg[t] = (unsigned)(next_u64() & 7);
        uint64_t body = ((uint64_t)msg[t] << 61) + (next_u64() >> 24) - ((uint64_t)1 << 39);
        for (size_t i = 0; i < LIN; ++i) {
            ct[i] = next_u64();
            body += ct[i] * s[i];
        }
        ct[LIN] = body;
    }

    rc = cntt_native_pack_keyswitch_batch(plan, glwe, lwe, pksk, LIN, COUNT, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("pack_keyswitch_batch", rc);

    /* phase = body - sum_q mask_q S_q in Z/2^64[X]/(X^n + 1); message t is the top 3 bits of coefficient t, rounded */
    memcpy(phase, glwe + K * N, N * 8);
    for (size_t q = 0; q < K; ++q)
        for (size_t a = 0; a < N; ++a)
            for (size_t b = 0; b < N; ++b) {
                const uint64_t v = glwe[q * N + a] * S[q * N + b];
                if (a + b < N) phase[a + b] -= v;
                else phase[a + b - N] += v;
            }
    for (size_t t = 0; t < N; ++t) {
        const unsigned got = (unsigned)(((phase[t] >> 60) + 1) >> 1) & 7u, want = t < COUNT ? msg[t] : 0u;
        if (t < COUNT) printf("message %u: %u, coefficient %u of the packed GLWE decrypts to %u%s\n", (unsigned)t, want, (unsigned)t, got, got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_native_plan_free(plan);
    for (int i = 0; i < NPRIMES; ++i) free(planes[i]);
    free(s), free(S), free(key), free(mask), free(skey), free(prod), free(lwe), free(glwe), free(phase);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
