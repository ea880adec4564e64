/* examples/pbs.c with several look-up tables per bootstrap (include/cntt_manylut.h), no counterpart in the reference: native64 Plan32
 * (ciphertext modulus 2^64), n = 1024, k = 1, L = 16, base_log = 16, levels = 4, log_lut_count = 2.  The program generates a binary LWE
 * key, a binary GLWE key and a NOISY bootstrapping key (|e| <= 2^4 in every row) as the residue planes cntt_pbs.h fixes, encrypts each
 * of the 8 messages of a 3-bit space under one padding bit (m -> m 2^60, noise below 2^40), and evaluates 2^2 = 4 different functions of
 * every message in ONE cntt_native_bootstrap_manylut_batch call: the modulus switch keeps multiples of 4, function h lives at the
 * coefficients 4 c + h of the table and comes out at the extraction index h.  Every one of the 32 outputs is decrypted with the flattened
 * GLWE key; the program exits non-zero on a wrong one.  A message has a box of n / 4 / 8 = 32 steps of the coarse switch, shifted by half
 * a box; the switch drifts by at most (L + 1) / 2 = 8.5 of them.  The library generates neither keys nor noise: this file is the
 * recipe.  Host buffers throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_manylut.h"

#define N 1024u
#define K 1u
#define L 16u
#define BASE_LOG 16u
#define LEVELS 4u
#define LOG_LUTS 2u
#define LUTS (1u << LOG_LUTS)
#define BATCH 8u
#define DELTA_LOG 60u /* one message step is 2^60: 3 bits under one padding bit */
#define NPRIMES 5

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t small_noise(void) { return (next_u64() >> 59) - 16; } /* |e| <= 2^4 */

static unsigned f(unsigned h, unsigned m) { return (m * (2u * h + 1u) + h) & 7u; } /* function h of the one bootstrap */

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

/* acc += a (*) S in Z/2^64[X]/(X^n + 1) for the binary key S */
static void mul_binary_add(uint64_t *acc, const uint64_t *a, const uint64_t *S) {
    for (size_t b = 0; b < N; ++b) {
        if (!S[b]) continue;
        for (size_t i = 0; i < N; ++i) {
            uint64_t *dst = acc + (i + b) % N;
            *dst = i + b < N ? *dst + a[i] : *dst - a[i];
        }
    }
}

int main(void) {
    const size_t rows = (K + 1) * LEVELS, slice = rows * (K + 1), nkey = (size_t)L * slice; /* key polynomials: key[i][j][o] */
    uint64_t *s = malloc(L * 8), *S = malloc(K * N * 8), *key = calloc(nkey * N, 8);
    uint64_t *lut = calloc((K + 1) * N, 8), *lwe_in = malloc(BATCH * (L + 1) * 8), *lwe_out = calloc(BATCH * LUTS * (K * N + 1), 8);
    void *planes[NPRIMES];
    const void *bsk[NPRIMES];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES || cntt_native_residue_bytes(plan) != 4) return 1;
    if (!s || !S || !key || !lut || !lwe_in || !lwe_out) return 1;
    for (int j = 0; j < NPRIMES; ++j) {
        planes[j] = malloc(nkey * N * 4);
        if (!planes[j]) return 1;
        bsk[j] = planes[j];
    }

    for (size_t i = 0; i < L; ++i) s[i] = next_u64() & 1;
    for (size_t i = 0; i < K * N; ++i) S[i] = next_u64() & 1;

    /* Row (q, l) of iteration i: a fresh GLWE encryption of 0 -- mask A uniform, body A (*) S + e, |e| <= 2^4 -- with
     * s_i 2^(64 - BASE_LOG l) added to coefficient 0 of polynomial q; the key the blind rotation reads is cntt_native_fwd_batch of it. */
    for (size_t i = 0; i < L; ++i)
        for (size_t q = 0; q <= K; ++q)
            for (size_t l = 1; l <= LEVELS; ++l) {
                uint64_t *row = key + (i * slice + (q * LEVELS + (l - 1)) * (K + 1)) * N;
                for (size_t x = 0; x < N; ++x) {
                    row[x] = next_u64();
                    row[K * N + x] = small_noise();
                }
                mul_binary_add(row + K * N, row, S);
                if (s[i]) row[q * N] += (uint64_t)1 << (64 - BASE_LOG * l);
            }
    rc = cntt_native_fwd_batch(plan, key, planes, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(key)", rc);

    /* The table: a trivial GLWE (zero mask) whose body holds function h at the coefficients 4 c + h: per function n / 4 = 256 coarse
     * steps, boxes of 32 steps per message, shifted by half a box so that the rounding of the modulus switch stays inside the box. */
    for (size_t j = 0; j < N; ++j) {
        const size_t c = j >> LOG_LUTS, np = N >> LOG_LUTS, t = c + np / 16;
        const uint64_t v = (uint64_t)f((unsigned)(j & (LUTS - 1)), (unsigned)((t % np) / (np / 8))) << DELTA_LOG;
        lut[K * N + j] = t < np ? v : 0 - v;
    }

    /* message m under the padding bit: m 2^60, plus noise below 2^40 */
    for (size_t b = 0; b < BATCH; ++b) {
        uint64_t body = ((uint64_t)b << DELTA_LOG) + (next_u64() >> 24) - ((uint64_t)1 << 39);
        for (size_t i = 0; i < L; ++i) {
            lwe_in[b * (L + 1) + i] = next_u64();
            if (s[i]) body += lwe_in[b * (L + 1) + i];
        }
        lwe_in[b * (L + 1) + L] = body;
    }

    rc = cntt_native_bootstrap_manylut_batch(plan, lwe_out, lwe_in, lut, 0, bsk, L, K, BASE_LOG, LEVELS, LOG_LUTS, LUTS, BATCH, NULL, 0,
                                             CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("bootstrap_manylut_batch", rc);

    /* output (b, h) at lwe_out[(b LUTS + h) (k n + 1)]: phase = body - <mask, flattened GLWE key> mod 2^64; the message is
     * round(phase / 2^60) mod 16 */
    for (size_t b = 0; b < BATCH; ++b) {
        printf("message %u:", (unsigned)b);
        for (unsigned h = 0; h < LUTS; ++h) {
            const uint64_t *ct = lwe_out + (b * LUTS + h) * (K * N + 1);
            uint64_t phase = ct[K * N];
            for (size_t i = 0; i < K * N; ++i)
                if (S[i]) phase -= ct[i];
            const unsigned got = (unsigned)(((phase >> (DELTA_LOG - 1)) + 1) >> 1) & 15u;
            printf(" f%u = %u -> %u%s", h, f(h, (unsigned)b), got, got == f(h, (unsigned)b) ? "" : "  WRONG");
            wrong += got != f(h, (unsigned)b);
        }
        printf("\n");
    }
    cntt_native_plan_free(plan);
    for (int j = 0; j < NPRIMES; ++j) free(planes[j]);
    free(s), free(S), free(key), free(lut), free(lwe_in), free(lwe_out);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("Success!\n");
    return 0;
}
