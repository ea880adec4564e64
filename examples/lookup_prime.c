/* An encrypted table lookup with a PRIME ciphertext modulus on the C ABI (include/cntt_prime_cmux.h, include/cntt_prime_pbs.h); no
 * counterpart in the reference: prime64 plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 256, k = 1, base_log = 16,
 * levels = 4.  The table has 16 * 256 = 4096 entries of 3 bits, entry a at coefficient a mod 256 of polynomial a / 256, as plaintexts
 * m (p-1)/8.  The 12 address bits come as NOISY GGSW ciphertexts under a binary GLWE key S: row (q, l) of a selector is a GLWE encryption
 * of zero (mask A uniform, body A (*) S + e, |e| < 2^10) with bit * 2^(64 - 16 l) added to polynomial q, stored as n^-1 fwd(row):
 * cntt_prime64_fwd_batch, then cntt_prime64_normalize_batch.  Per address the program runs
 *   cntt_prime64_cmux_tree_batch      over the top 4 bits: the GLWE ciphertext of table polynomial a / 256,
 *   cntt_prime64_blind_rotate_batch   over the low 8 bits with rot_t[i] = 2n - 2^i (body row 0) and lut_per_element = 1: bit i
 *                                     multiplies by X^(-2^i), so entry a arrives at coefficient 0,
 *   cntt_prime64_sample_extract_batch at index 0: the LWE ciphertext of entry a under the flattened key,
 * decrypts on the host and exits non-zero unless every looked-up entry decodes.  The library generates neither keys nor noise: this
 * file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_cmux.h"

#define P 18446744069414584321ull
#define N 256u
#define LOGN 8u
#define K 1u
#define BASE_LOG 16u
#define LEVELS 4u
#define M 16u    /* table polynomials */
#define DEPTH 4u /* log2 M */
#define BITS (LOGN + DEPTH)
#define DELTA ((P - 1) / 8) /* one message step */
#define SEL_POLYS ((K + 1) * LEVELS * (K + 1))

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

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

/* acc += a (*) S in Z_p[X]/(X^n + 1) for the binary key S */
static void mul_binary_add(uint64_t *acc, const uint64_t *a, const uint64_t *S) {
    for (size_t b = 0; b < N; ++b) {
        if (!S[b]) continue;
        for (size_t i = 0; i < N; ++i) {
            uint64_t *dst = acc + (i + b) % N;
            *dst = i + b < N ? add_p(*dst, a[i]) : sub_p(*dst, a[i]);
        }
    }
}

/* GGSW(bit), coefficient domain, SEL_POLYS polynomials: row j = q LEVELS + (l - 1) at polynomial j (K + 1) */
static void ggsw(uint64_t *sel, const uint64_t *S, unsigned bit) {
    for (size_t q = 0; q <= K; ++q)
        for (size_t l = 1; l <= LEVELS; ++l) {
            uint64_t *row = sel + (q * LEVELS + (l - 1)) * (K + 1) * N;
            for (size_t x = 0; x < N; ++x) {
                row[x] = next_mod_p();
                row[K * N + x] = sub_p(next_u64() >> 53, (uint64_t)1 << 10); /* |e| < 2^10 */
            }
            mul_binary_add(row + K * N, row, S);
            if (bit) row[q * N] = add_p(row[q * N], (uint64_t)1 << (64 - BASE_LOG * l));
        }
}

int main(void) {
    static const unsigned addresses[] = {0, 1, 255, 256, 2047, 2748, 3840, 4095};
    const size_t naddr = sizeof addresses / sizeof addresses[0], sel_words = (size_t)SEL_POLYS * N;
    uint64_t *S = malloc(N * 8), *G = calloc(2 * BITS * sel_words, 8), *sels = malloc(BITS * sel_words * 8);
    uint64_t *table = malloc((size_t)M * N * 8), *glwe = malloc((K + 1) * N * 8), *acc = malloc((K + 1) * N * 8), *lwe = malloc((K * N + 1) * 8);
    unsigned *entries = malloc((size_t)M * N * sizeof(unsigned));
    uint32_t rot_t[LOGN + 1];
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (!S || !G || !sels || !table || !glwe || !acc || !lwe || !entries) return 1;

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;
    for (size_t a = 0; a < (size_t)M * N; ++a) {
        entries[a] = (unsigned)(next_u64() & 7);
        table[a] = (uint64_t)entries[a] * DELTA; /* plaintexts: the table is not encrypted */
    }
    /* GGSW(0) and GGSW(1) of every address bit, then the form the calls read: n^-1 fwd */
    for (size_t i = 0; i < BITS; ++i)
        for (unsigned bit = 0; bit < 2; ++bit) ggsw(G + (2 * i + bit) * sel_words, S, bit);
    rc = cntt_prime64_fwd_batch(plan, G, 2 * BITS * SEL_POLYS, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(ggsw)", rc);
    rc = cntt_prime64_normalize_batch(plan, G, 2 * BITS * SEL_POLYS, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(ggsw)", rc);
    /* the fixed rotation rows: iteration i multiplies by X^(2n - 2^i) = X^(-2^i) where its selector encrypts 1; the body row is 0 */
    for (size_t i = 0; i < LOGN; ++i) rot_t[i] = 2 * N - (1u << i);
    rot_t[LOGN] = 0;

    for (size_t t = 0; t < naddr; ++t) {
        const unsigned a = addresses[t];
        /* address bit i selects GGSW(bit): the low LOGN selectors for the rotation, then the DEPTH selectors of the tree, LSB first */
        for (size_t i = 0; i < BITS; ++i) memcpy(sels + i * sel_words, G + (2 * i + ((a >> i) & 1)) * sel_words, sel_words * 8);
        rc = cntt_prime64_cmux_tree_batch(plan, glwe, table, sels + LOGN * sel_words, M, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("cmux_tree_batch", rc);
        rc = cntt_prime64_blind_rotate_batch(plan, acc, glwe, 1, rot_t, sels, LOGN, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("blind_rotate_batch", rc);
        rc = cntt_prime64_sample_extract_batch(plan, lwe, acc, K, 0, 1, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("sample_extract_batch", rc);
        /* phase = body - <mask, s> under the flattened key s[j] = S[j] */
        uint64_t phase = lwe[K * N];
        for (size_t x = 0; x < N; ++x)
            if (S[x]) phase = sub_p(phase, lwe[x]);
        const unsigned got = phase >= P - DELTA / 2 ? 0u : (unsigned)((phase + DELTA / 2) / DELTA) & 7u;
        printf("address %4u: entry %u, looked up %u%s\n", a, entries[a], got, got == entries[a] ? "" : "  WRONG");
        wrong += got != entries[a];
    }
    cntt_prime64_plan_free(plan);
    free(S), free(G), free(sels), free(table), free(glwe), free(acc), free(lwe), free(entries);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("every looked-up entry decoded (%u addresses of a table of %u entries)\nSuccess!\n", (unsigned)naddr, M * N);
    return 0;
}
