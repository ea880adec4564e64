/* examples/lookup_prime.c with the selectors produced by the library: an encrypted table lookup whose address bits arrive as LWE
 * ciphertexts and are circuit-bootstrapped into GGSW selectors on the device (include/cntt_prime_cbs.h); no counterpart in the
 * reference.  prime64 plan, p = 2^64 - 2^32 + 1 (W = 64), n = 64, k = 1.  The table has 4 * 64 = 256 entries of 3 bits, entry a at
 * coefficient a mod 64 of polynomial a / 64, as plaintexts m (p-1)/8.  The 8 address bits are LWE encryptions of dimension 8 under a
 * binary key, phase bit (p+1)/2 + e.  Keys, all under the binary GLWE key S and with a noise |e| <= 16 per row:
 *   bsk_ntt     8 GGSWs of the LWE key bits, gadget (16, 4)                                   (cntt_prime_pbs.h)
 *   fpksk_ntt   k + 1 = 2 functional packing keys of (n + 1) * 2 rows, gadget (22, 2): row (i, j) of key q encrypts
 *               s_in[i] M_q 2^(64 - 22 j) for i < n and -M_q 2^(64 - 22 j) for i = n, M_0 = -S, M_1 = 1   (cntt_prime_cbs.h)
 * both stored as n^-1 fwd(row): cntt_prime64_fwd_batch, then cntt_prime64_normalize_batch.  Per address the program runs
 *   cntt_prime64_circuit_bootstrap_batch   the 8 bits -> 8 selectors of gadget (8, 3), bit i is selector i,
 *   cntt_prime64_cmux_tree_batch           over the top 2 bits: the GLWE ciphertext of table polynomial a / 64,
 *   cntt_prime64_blind_rotate_batch        over the low 6 bits with rot_t[i] = 2n - 2^i (body row 0) and lut_per_element = 1,
 *   cntt_prime64_sample_extract_batch      at index 0: the LWE ciphertext of entry a under the flattened key,
 * decrypts on the host and exits non-zero unless every looked-up entry decodes.  The library generates neither keys nor noise: this
 * file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_cbs.h"

#define P 18446744069414584321ull
#define N 64u
#define LOGN 6u
#define K 1u
#define L 8u /* dimension of the LWE ciphertexts of the address bits */
#define PBS_BASE_LOG 16u
#define PBS_LEVELS 4u
#define KS_BASE_LOG 22u
#define KS_LEVELS 2u
#define CBS_BASE_LOG 8u
#define CBS_LEVELS 3u
#define M 4u     /* table polynomials */
#define DEPTH 2u /* log2 M */
#define BITS (LOGN + DEPTH)
#define DELTA ((P - 1) / 8) /* one message step */
#define SEL_POLYS ((K + 1) * CBS_LEVELS * (K + 1))
#define BSK_POLYS (L * (K + 1) * PBS_LEVELS * (K + 1))
#define KS_ROWS ((K * N + 1) * KS_LEVELS)
#define FK_POLYS ((K + 1) * KS_ROWS * (K + 1))

static uint64_t rng_state = 0x13198A2E03707344ull;
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
static uint64_t noise(void) { return sub_p(next_u64() >> 59, 16); } /* in [-16, 15] */

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

/* one GLWE encryption of zero under S: K + 1 polynomials, mask uniform, body = mask (*) S + e */
static void glwe_zero(uint64_t *row, const uint64_t *S) {
    for (size_t x = 0; x < N; ++x) {
        row[x] = next_mod_p();
        row[K * N + x] = noise();
    }
    mul_binary_add(row + K * N, row, S);
}

/* GGSW(bit) with the PBS gadget, coefficient domain: row j = q levels + (l - 1) at polynomial j (K + 1) */
static void ggsw(uint64_t *sel, const uint64_t *S, unsigned bit) {
    for (size_t q = 0; q <= K; ++q)
        for (size_t l = 1; l <= PBS_LEVELS; ++l) {
            uint64_t *row = sel + (q * PBS_LEVELS + (l - 1)) * (K + 1) * N;
            glwe_zero(row, S);
            if (bit) row[q * N] = add_p(row[q * N], (uint64_t)1 << (64 - PBS_BASE_LOG * l));
        }
}

/* the k + 1 functional packing keys of cntt_prime_cbs.h, coefficient domain; s_in[i] = S[i] (k = 1) */
static void functional_keys(uint64_t *fk, const uint64_t *S) {
    for (size_t q = 0; q <= K; ++q)
        for (size_t i = 0; i <= K * N; ++i)
            for (size_t j = 1; j <= KS_LEVELS; ++j) {
                uint64_t *row = fk + ((q * KS_ROWS + i * KS_LEVELS + (j - 1)) * (K + 1)) * N, *body = row + K * N;
                const uint64_t g = (uint64_t)1 << (64 - KS_BASE_LOG * j);
                const int f = i < K * N ? (int)S[i] : -1; /* the factor s_in[i], or -1 for the body word */
                glwe_zero(row, S);
                if (f == 0) continue;
                if (q == K) /* M_k = 1: the constant f g */
                    body[0] = f > 0 ? add_p(body[0], g) : sub_p(body[0], g);
                else /* M_q = -S_q: the polynomial -f g S */
                    for (size_t x = 0; x < N; ++x)
                        if (S[x]) body[x] = f > 0 ? sub_p(body[x], g) : add_p(body[x], g);
            }
}

int main(void) {
    static const unsigned addresses[] = {0, 1, 63, 64, 127, 170, 192, 255};
    const size_t naddr = sizeof addresses / sizeof addresses[0], sel_words = (size_t)SEL_POLYS * N;
    uint64_t *S = malloc(N * 8), *bsk = malloc((size_t)BSK_POLYS * N * 8), *fk = malloc((size_t)FK_POLYS * N * 8);
    uint64_t *sels = malloc(BITS * sel_words * 8), *bits_in = malloc((size_t)BITS * (L + 1) * 8);
    uint64_t *table = malloc((size_t)M * N * 8), *glwe = malloc((K + 1) * N * 8), *acc = malloc((K + 1) * N * 8), *lwe = malloc((K * N + 1) * 8);
    uint64_t s_lwe[L];
    unsigned entries[M * N];
    uint32_t rot_t[LOGN + 1];
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (!S || !bsk || !fk || !sels || !bits_in || !table || !glwe || !acc || !lwe) return 1;

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;
    for (size_t i = 0; i < L; ++i) s_lwe[i] = next_u64() & 1;
    for (size_t a = 0; a < (size_t)M * N; ++a) {
        entries[a] = (unsigned)(next_u64() & 7);
        table[a] = (uint64_t)entries[a] * DELTA; /* plaintexts: the table is not encrypted */
    }
    /* the two keys, then the form the calls read: n^-1 fwd */
    for (size_t i = 0; i < L; ++i) ggsw(bsk + i * (K + 1) * PBS_LEVELS * (K + 1) * N, S, (unsigned)s_lwe[i]);
    functional_keys(fk, S);
    rc = cntt_prime64_fwd_batch(plan, bsk, BSK_POLYS, CNTT_MEM_HOST, NULL);
    if (rc == CNTT_OK) rc = cntt_prime64_normalize_batch(plan, bsk, BSK_POLYS, CNTT_MEM_HOST, NULL);
    if (rc == CNTT_OK) rc = cntt_prime64_fwd_batch(plan, fk, FK_POLYS, CNTT_MEM_HOST, NULL);
    if (rc == CNTT_OK) rc = cntt_prime64_normalize_batch(plan, fk, FK_POLYS, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch / normalize_batch of the keys", rc);
    /* the fixed rotation rows: iteration i multiplies by X^(2n - 2^i) = X^(-2^i) where its selector encrypts 1; the body row is 0 */
    for (size_t i = 0; i < LOGN; ++i) rot_t[i] = 2 * N - (1u << i);
    rot_t[LOGN] = 0;

    for (size_t t = 0; t < naddr; ++t) {
        const unsigned a = addresses[t];
        /* the address bits as LWE ciphertexts: phase bit (p + 1) / 2 + e, LSB first */
        for (size_t i = 0; i < BITS; ++i) {
            uint64_t *ct = bits_in + i * (L + 1), body = add_p(noise(), ((a >> i) & 1) ? (P + 1) / 2 : 0);
            for (size_t x = 0; x < L; ++x) {
                ct[x] = next_mod_p();
                if (s_lwe[x]) body = add_p(body, ct[x]);
            }
            ct[L] = body;
        }
        rc = cntt_prime64_circuit_bootstrap_batch(plan, sels, bits_in, bsk, fk, L, K, PBS_BASE_LOG, PBS_LEVELS, KS_BASE_LOG, KS_LEVELS, CBS_BASE_LOG,
                                                  CBS_LEVELS, BITS, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("circuit_bootstrap_batch", rc);
        /* the low LOGN selectors rotate, the DEPTH selectors after them drive the tree */
        rc = cntt_prime64_cmux_tree_batch(plan, glwe, table, sels + LOGN * sel_words, M, K, CBS_BASE_LOG, CBS_LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("cmux_tree_batch", rc);
        rc = cntt_prime64_blind_rotate_batch(plan, acc, glwe, 1, rot_t, sels, LOGN, K, CBS_BASE_LOG, CBS_LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("blind_rotate_batch", rc);
        rc = cntt_prime64_sample_extract_batch(plan, lwe, acc, K, 0, 1, CNTT_MEM_HOST, NULL);
        if (rc != CNTT_OK) return die("sample_extract_batch", rc);
        /* phase = body - <mask, s> under the flattened key s[j] = S[j] */
        uint64_t phase = lwe[K * N];
        for (size_t x = 0; x < N; ++x)
            if (S[x]) phase = sub_p(phase, lwe[x]);
        const unsigned got = phase >= P - DELTA / 2 ? 0u : (unsigned)((phase + DELTA / 2) / DELTA) & 7u;
        printf("address %3u: entry %u, looked up %u%s\n", a, entries[a], got, got == entries[a] ? "" : "  WRONG");
        wrong += got != entries[a];
    }
    cntt_prime64_plan_free(plan);
    free(S), free(bsk), free(fk), free(sels), free(bits_in), free(table), free(glwe), free(acc), free(lwe);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("every looked-up entry decoded (%u addresses of a table of %u entries)\nSuccess!\n", (unsigned)naddr, M * N);
    return 0;
}
