/* An encrypted table lookup with the ciphertext modulus 2^64 on the C ABI (include/cntt_cmux.h, include/cntt_pbs.h); no counterpart in
 * the reference, the native twin of lookup_prime.c: native64 Plan32 (five 30-bit residue primes), n = 256, k = 1, base_log = 16,
 * levels = 4.  The table has 16 * 256 = 4096 entries of 3 bits, entry a at coefficient a mod 256 of polynomial a / 256, as plaintexts
 * m 2^61.  The 12 address bits come as NOISY GGSW ciphertexts under a binary GLWE key S: row (q, l) of a selector is a GLWE encryption
 * of zero (mask A uniform, body A (*) S + e, |e| < 2^10) with bit * 2^(64 - 16 l) added to polynomial q, stored as the residue planes
 * cntt_native_fwd_batch writes.  Per address the program runs
 *   cntt_native_cmux_tree_batch      over the top 4 bits: the GLWE ciphertext of table polynomial a / 256,
 *   cntt_native_blind_rotate_batch   over the low 8 bits with rot_t[i] = 2n - 2^i (body row 0) and lut_per_element = 1: bit i
 *                                    multiplies by X^(-2^i), so entry a arrives at coefficient 0,
 *   cntt_native_sample_extract_batch at index 0: the LWE ciphertext of entry a under the flattened key,
 * decrypts on the host and exits non-zero unless every looked-up entry decodes.  The library generates neither keys nor noise: this
 * file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_cmux.h"

#define N 256u
#define LOGN 8u
#define K 1u
#define BASE_LOG 16u
#define LEVELS 4u
#define M 16u    /* table polynomials */
#define DEPTH 4u /* log2 M */
#define BITS (LOGN + DEPTH)
#define DELTA_LOG 61u /* one message step is 2^61 */
#define SEL_POLYS ((K + 1) * LEVELS * (K + 1))
#define NPRIMES 5

static uint64_t rng_state = 0x243F6A8885A308D3ull;
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

/* GGSW(bit), coefficient domain, SEL_POLYS polynomials: row j = q LEVELS + (l - 1) at polynomial j (K + 1) */
static void ggsw(uint64_t *sel, const uint64_t *S, unsigned bit) {
    for (size_t q = 0; q <= K; ++q)
        for (size_t l = 1; l <= LEVELS; ++l) {
            uint64_t *row = sel + (q * LEVELS + (l - 1)) * (K + 1) * N;
            for (size_t x = 0; x < N; ++x) {
                row[x] = next_u64();
                row[K * N + x] = (next_u64() >> 53) - ((uint64_t)1 << 10); /* |e| <= 2^10 */
            }
            mul_binary_add(row + K * N, row, S);
            if (bit) row[q * N] += (uint64_t)1 << (64 - BASE_LOG * l);
        }
}

int main(void) {
    static const unsigned addresses[] = {0, 1, 255, 256, 2047, 2748, 3840, 4095};
    const size_t naddr = sizeof addresses / sizeof addresses[0], sel_words = (size_t)SEL_POLYS * N;
    uint64_t *S = malloc(N * 8), *G = calloc(2 * BITS * sel_words, 8);
    uint64_t *table = malloc((size_t)M * N * 8), *glwe = malloc((K + 1) * N * 8), *acc = malloc((K + 1) * N * 8), *lwe = malloc((K * N + 1) * 8);
    unsigned *entries = malloc((size_t)M * N * sizeof(unsigned));
    uint32_t rot_t[LOGN + 1];
    uint32_t *Gp[NPRIMES], *sels[NPRIMES];              /* residue planes: both values of every bit / the address at hand */
    void *Gv[NPRIMES];
    const void *low[NPRIMES], *top[NPRIMES];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (cntt_native_nprimes(plan) != NPRIMES || cntt_native_residue_bytes(plan) != 4) return 1;
    if (!S || !G || !table || !glwe || !acc || !lwe || !entries) return 1;
    for (int j = 0; j < NPRIMES; ++j) {
        Gp[j] = malloc(2 * BITS * sel_words * 4);
        sels[j] = malloc(BITS * sel_words * 4);
        if (!Gp[j] || !sels[j]) return 1;
        Gv[j] = Gp[j];
        low[j] = sels[j];                               /* selectors 0 .. LOGN - 1: the rotation */
        top[j] = sels[j] + LOGN * sel_words;            /* selectors LOGN .. BITS - 1: the tree, LSB first */
    }

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;
    for (size_t a = 0; a < (size_t)M * N; ++a) {
        entries[a] = (unsigned)(next_u64() & 7);
        table[a] = (uint64_t)entries[a] << DELTA_LOG; /* plaintexts: the table is not encrypted */
    }
    /* GGSW(0) and GGSW(1) of every address bit, then the form the calls read: the residue planes of fwd_batch */
    for (size_t i = 0; i < BITS; ++i)
        for (unsigned bit = 0; bit < 2; ++bit) ggsw(G + (2 * i + bit) * sel_words, S, bit);
    rc = cntt_native_fwd_batch(plan, G, Gv, 2 * BITS * SEL_POLYS, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(ggsw)", rc);
    /* the fixed rotation rows: iteration i multiplies by X^(2n - 2^i) = X^(-2^i) where its selector encrypts 1; the body row is 0 */
    for (size_t i = 0; i < LOGN; ++i) rot_t[i] = 2 * N - (1u << i);
    rot_t[LOGN] = 0;

    for (size_t t = 0; t < naddr; ++t) {
        const unsigned a = addresses[t];
        /* address bit i selects GGSW(bit), plane by plane */
        for (int j = 0; j < NPRIMES; ++j)
            for (size_t i = 0; i < BITS; ++i) memcpy(sels[j] + i * sel_words, Gp[j] + (2 * i + ((a >> i) & 1)) * sel_words, sel_words * 4);
        rc = cntt_native_cmux_tree_batch(plan, glwe, table, top, M, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("cmux_tree_batch", rc);
        rc = cntt_native_blind_rotate_batch(plan, acc, glwe, 1, rot_t, low, LOGN, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("blind_rotate_batch", rc);
        rc = cntt_native_sample_extract_batch(plan, lwe, acc, K, 0, 1, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("sample_extract_batch", rc);
        /* phase = body - <mask, s> under the flattened key s[j] = S[j] */
        uint64_t phase = lwe[K * N];
        for (size_t x = 0; x < N; ++x)
            if (S[x]) phase -= lwe[x];
        const unsigned got = (unsigned)(((phase >> (DELTA_LOG - 1)) + 1) >> 1) & 7u;
        printf("address %4u: entry %u, looked up %u%s\n", a, entries[a], got, got == entries[a] ? "" : "  WRONG");
        wrong += got != entries[a];
    }
    cntt_native_plan_free(plan);
    for (int j = 0; j < NPRIMES; ++j) free(Gp[j]), free(sels[j]);
    free(S), free(G), free(table), free(glwe), free(acc), free(lwe), free(entries);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("every looked-up entry decoded (%u addresses of a table of %u entries)\nSuccess!\n", (unsigned)naddr, M * N);
    return 0;
}
