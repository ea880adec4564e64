/* An encrypted table lookup with the ciphertext modulus 2^64 whose address bits arrive as LWE ciphertexts, on the C ABI
 * (include/cntt_cbs.h, include/cntt_cmux.h, include/cntt_pbs.h); no counterpart in the reference, the native twin of cbs_lookup_prime.c
 * and lookup_native.c with the selectors made by the circuit bootstrap instead of from the secret key: native64 Plan32 (five 30-bit
 * residue primes), n = 64, k = 1, lwe_dim = 8.  The table has 4 * 64 = 256 entries of 3 bits, entry a at coefficient a mod 64 of
 * polynomial a / 64, as plaintexts m 2^61.  Per address the program
 *   encrypts the 8 address bits as LWE ciphertexts bit 2^63 + e, |e| < 2^40, under a binary LWE key,
 *   cntt_native_circuit_bootstrap_batch  turns them into 8 GGSW selectors (PBS gadget (16, 4), keyswitch gadget (22, 2), selector
 *                                        gadget (8, 3)), as the residue planes the next two calls read,
 *   cntt_native_cmux_tree_batch          over the top 2 bits: the GLWE ciphertext of table polynomial a / 64,
 *   cntt_native_blind_rotate_batch       over the low 6 bits with rot_t[i] = 2n - 2^i (body row 0) and lut_per_element = 1,
 *   cntt_native_sample_extract_batch     at index 0: the LWE ciphertext of entry a under the flattened key,
 * decrypts on the host and exits non-zero unless every looked-up entry decodes.  Every key row carries a noise |e| <= 2^4.  The library
 * generates neither keys nor noise: this file is the recipe, the bootstrapping key as cntt_pbs.h and the k + 1 functional keys as
 * cntt_cbs.h state them -- PLAIN words, not residue planes.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_cbs.h"

#define N 64u
#define LOGN 6u
#define K 1u
#define L 8u
#define PBS_BASE_LOG 16u
#define PBS_LEVELS 4u
#define KS_BASE_LOG 22u
#define KS_LEVELS 2u
#define CBS_BASE_LOG 8u
#define CBS_LEVELS 3u
#define M 4u     /* table polynomials */
#define DEPTH 2u /* log2 M */
#define BITS (LOGN + DEPTH)
#define DELTA_LOG 61u /* one message step is 2^61 */
#define SEL_POLYS ((K + 1) * CBS_LEVELS * (K + 1))
#define LIN (K * N)
#define R ((LIN + 1) * KS_LEVELS)
#define NPRIMES 5

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t next_u64(void) {
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static uint64_t small_noise(void) { return (next_u64() >> 59) - 16; } /* |e| <= 2^4 */

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

/* a GLWE encryption of zero under S into row (K + 1 polynomials): uniform mask, body = mask (*) S + e */
static void glwe_zero(uint64_t *row, const uint64_t *S) {
    for (size_t x = 0; x < N; ++x) {
        row[x] = next_u64();
        row[K * N + x] = small_noise();
    }
    mul_binary_add(row + K * N, row, S);
}

/* GGSW(bit) for the PBS gadget, coefficient domain: row j = q PBS_LEVELS + (l - 1) at polynomial j (K + 1) */
static void ggsw(uint64_t *sel, const uint64_t *S, unsigned bit) {
    for (size_t q = 0; q <= K; ++q)
        for (size_t l = 1; l <= PBS_LEVELS; ++l) {
            uint64_t *row = sel + (q * PBS_LEVELS + (l - 1)) * (K + 1) * N;
            glwe_zero(row, S);
            if (bit) row[q * N] += (uint64_t)1 << (64 - PBS_BASE_LOG * l);
        }
}

int main(void) {
    static const unsigned addresses[] = {0, 1, 63, 64, 127, 170, 192, 255};
    const size_t naddr = sizeof addresses / sizeof addresses[0], sel_words = (size_t)SEL_POLYS * N;
    const size_t bsk_polys = (size_t)L * (K + 1) * PBS_LEVELS * (K + 1), fk_polys = (size_t)(K + 1) * R * (K + 1);
    uint64_t *S = malloc(N * 8), *bsk = calloc(bsk_polys * N, 8), *fk = calloc(fk_polys * N, 8);
    uint64_t *table = malloc((size_t)M * N * 8), *glwe = malloc((K + 1) * N * 8), *acc = malloc((K + 1) * N * 8), *lwe = malloc((K * N + 1) * 8);
    uint64_t s_lwe[L], bits_lwe[BITS * (L + 1)];
    unsigned *entries = malloc((size_t)M * N * sizeof(unsigned));
    uint32_t rot_t[LOGN + 1];
    uint32_t *bskp[NPRIMES], *sels[NPRIMES];
    void *bskv[NPRIMES], *selv[NPRIMES];
    const void *bskc[NPRIMES], *low[NPRIMES], *top[NPRIMES];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES || cntt_native_residue_bytes(plan) != 4) return 1;
    if (!S || !bsk || !fk || !table || !glwe || !acc || !lwe || !entries) return 1;
    for (int j = 0; j < NPRIMES; ++j) {
        bskp[j] = malloc(bsk_polys * N * 4);
        sels[j] = malloc(BITS * sel_words * 4);
        if (!bskp[j] || !sels[j]) return 1;
        bskv[j] = bskp[j], bskc[j] = bskp[j], selv[j] = sels[j];
        low[j] = sels[j];                               /* selectors 0 .. LOGN - 1: the rotation */
        top[j] = sels[j] + LOGN * sel_words;            /* selectors LOGN .. BITS - 1: the tree, LSB first */
    }

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;
    for (size_t i = 0; i < L; ++i) s_lwe[i] = next_u64() & 1;
    for (size_t a = 0; a < (size_t)M * N; ++a) {
        entries[a] = (unsigned)(next_u64() & 7);
        table[a] = (uint64_t)entries[a] << DELTA_LOG; /* plaintexts: the table is not encrypted */
    }
    /* the bootstrapping key: GGSW(s_lwe[i]) per mask word, as the residue planes of fwd_batch */
    for (size_t i = 0; i < L; ++i) ggsw(bsk + i * (K + 1) * PBS_LEVELS * (K + 1) * N, S, (unsigned)s_lwe[i]);
    rc = cntt_native_fwd_batch(plan, bsk, bskv, bsk_polys, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(bsk)", rc);
    /* the functional keys F_0 .. F_K, plain words: row (i, j) of F_q encrypts s_in[i] M_q 2^(64 - KS_BASE_LOG j) for i < Lin and
     * -M_q 2^(64 - KS_BASE_LOG j) for i = Lin; s_in[i] = S[i] (k = 1), M_q = -S for q < K and 1 for q = K */
    for (size_t q = 0; q <= K; ++q)
        for (size_t i = 0; i <= LIN; ++i)
            for (size_t j = 1; j <= KS_LEVELS; ++j) {
                uint64_t *row = fk + ((q * R + i * KS_LEVELS + (j - 1)) * (K + 1)) * N;
                const uint64_t g = (uint64_t)1 << (64 - KS_BASE_LOG * j);
                const uint64_t f = i < LIN ? S[i] * g : (uint64_t)0 - g;
                glwe_zero(row, S);
                if (q == K) row[K * N] += f;
                else
                    for (size_t x = 0; x < N; ++x) row[K * N + x] -= f * S[x];
            }
    /* the fixed rotation rows: iteration i multiplies by X^(2n - 2^i) = X^(-2^i) where its selector encrypts 1; the body row is 0 */
    for (size_t i = 0; i < LOGN; ++i) rot_t[i] = 2 * N - (1u << i);
    rot_t[LOGN] = 0;

    for (size_t t = 0; t < naddr; ++t) {
        const unsigned a = addresses[t];
        /* the address bits as LWE ciphertexts: bit 2^63 + e */
        for (size_t i = 0; i < BITS; ++i) {
            uint64_t *ct = bits_lwe + i * (L + 1);
            ct[L] = ((uint64_t)((a >> i) & 1) << 63) + (next_u64() >> 23) - ((uint64_t)1 << 40);
            for (size_t x = 0; x < L; ++x) {
                ct[x] = next_u64();
                if (s_lwe[x]) ct[L] += ct[x];
            }
        }
        rc = cntt_native_circuit_bootstrap_batch(plan, selv, bits_lwe, bskc, fk, L, K, PBS_BASE_LOG, PBS_LEVELS, KS_BASE_LOG, KS_LEVELS,
                                                 CBS_BASE_LOG, CBS_LEVELS, BITS, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("circuit_bootstrap_batch", rc);
        rc = cntt_native_cmux_tree_batch(plan, glwe, table, top, M, K, CBS_BASE_LOG, CBS_LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("cmux_tree_batch", rc);
        rc = cntt_native_blind_rotate_batch(plan, acc, glwe, 1, rot_t, low, LOGN, K, CBS_BASE_LOG, CBS_LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("blind_rotate_batch", rc);
        rc = cntt_native_sample_extract_batch(plan, lwe, acc, K, 0, 1, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("sample_extract_batch", rc);
        /* phase = body - <mask, s> under the flattened key s[j] = S[j] */
        uint64_t phase = lwe[K * N];
        for (size_t x = 0; x < N; ++x)
            if (S[x]) phase -= lwe[x];
        const unsigned got = (unsigned)(((phase >> (DELTA_LOG - 1)) + 1) >> 1) & 7u;
        printf("address %3u: entry %u, looked up %u%s\n", a, entries[a], got, got == entries[a] ? "" : "  WRONG");
        wrong += got != entries[a];
    }
    cntt_native_plan_free(plan);
    for (int j = 0; j < NPRIMES; ++j) free(bskp[j]), free(sels[j]);
    free(S), free(bsk), free(fk), free(table), free(glwe), free(acc), free(lwe), free(entries);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("every looked-up entry decoded (%u addresses of a table of %u entries)\nSuccess!\n", (unsigned)naddr, M * N);
    return 0;
}
