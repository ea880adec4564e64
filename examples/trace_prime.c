/* The homomorphic trace with a PRIME ciphertext modulus on the C ABI (include/cntt_prime_automorphism.h); no counterpart in the
 * reference: prime64 plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 256, k = 1, base_log = 8, levels = 6.  The
 * program generates a binary GLWE key S and the log2 n = 8 NOISY automorphism keys of the exponents t_r = n / 2^r + 1 -- row (r, l) of
 * a key is a GLWE encryption of sigma_t(S_r) 2^(64 - 8 l), mask polynomial first, body last, noise below 2^10; all keys back to back
 * in the layout the header fixes, n^-1 fwd(key): cntt_prime64_fwd_batch, then cntt_prime64_normalize_batch -- encrypts a GLWE
 * ciphertext that carries a 3-bit message in EVERY coefficient (m_i (p-1)/8, noise below 2^30), scales every word by n^-1 mod p (the
 * trace multiplies what survives by n; the scaling goes in front so that the keyswitch noise is not scaled with it), runs the full
 * trace in one cntt_prime64_glwe_trace_batch call, decrypts on the host and exits non-zero unless coefficient 0 reads its message and
 * every other coefficient reads 0.  The library generates neither keys nor noise: this file is the recipe.  Host buffers
 * (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_automorphism.h"

#define P 18446744069414584321ull
#define N 256u
#define LOGN 8u
#define K 1u
#define BASE_LOG 8u
#define LEVELS 6u
#define DELTA ((P - 1) / 8) /* one message step */

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
__extension__ typedef unsigned __int128 u128;
static uint64_t mul_p(uint64_t a, uint64_t b) { return (uint64_t)((u128)a * b % P); }
static uint64_t pow_p(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, a = mul_p(a, a))
        if (e & 1) r = mul_p(r, a);
    return r;
}

static int die(const char *what, int rc) {
    fprintf(stderr, "%s: status %d: %s\n", what, rc, cntt_last_error());
    return 1;
}

/* acc -= a (*) S in Z_p[X]/(X^n + 1) for the binary key S (sign = 0), or acc += a (*) S (sign = 1) */
static void mul_binary_acc(uint64_t *acc, const uint64_t *a, const uint64_t *S, int sign) {
    for (size_t b = 0; b < N; ++b) {
        if (!S[b]) continue;
        for (size_t i = 0; i < N; ++i) {
            const int plus = (i + b < N) == (sign != 0);
            uint64_t *dst = acc + (i + b) % N;
            *dst = plus ? add_p(*dst, a[i]) : sub_p(*dst, a[i]);
        }
    }
}

int main(void) {
    const size_t key_polys = (size_t)K * LEVELS * (K + 1), nkey = LOGN * key_polys;
    uint64_t *S = malloc(N * 8), *rot = malloc(N * 8), *ak = calloc(nkey * N, 8);
    uint64_t *ct = calloc((K + 1) * N, 8), *out = calloc((K + 1) * N, 8), *phase = malloc(N * 8);
    unsigned msgs[N];
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (!S || !rot || !ak || !ct || !out || !phase) return 1;

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;

    /* The automorphism keys.  Key r belongs to t = n / 2^r + 1.  sigma_t(S)[j] = +-S[j t^-1 mod 2n mod n] (the header's gather form; here
     * by the scatter that defines it: X^i -> (-1)^floor(i t / n) X^(i t mod n)).  Row l: mask A uniform, body = A (*) S + e +
     * sigma_t(S) 2^(64 - BASE_LOG l), |e| < 2^10 per coefficient. */
    for (size_t r = 0; r < LOGN; ++r) {
        const size_t t = (N >> r) + 1;
        memset(rot, 0, N * 8);
        for (size_t i = 0; i < N; ++i) {
            const size_t e = i * t % (2 * N);
            rot[e % N] = e >= N ? sub_p(0, S[i]) : S[i];
        }
        for (size_t l = 1; l <= LEVELS; ++l) {
            uint64_t *row = ak + (r * key_polys + (l - 1) * (K + 1)) * N; /* AK[l - 1][0 .. K] */
            for (size_t x = 0; x < N; ++x) {
                row[x] = next_mod_p();
                row[K * N + x] = sub_p(next_u64() >> 53, (uint64_t)1 << 10);
            }
            mul_binary_acc(row + K * N, row, S, 1);
            for (size_t x = 0; x < N; ++x) row[K * N + x] = add_p(row[K * N + x], mul_p(rot[x], (uint64_t)1 << (64 - BASE_LOG * l)));
        }
    }
    /* the keys the call reads: n^-1 fwd(key) */
    rc = cntt_prime64_fwd_batch(plan, ak, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(ak)", rc);
    rc = cntt_prime64_normalize_batch(plan, ak, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(ak)", rc);

    /* a message in every coefficient: body = A (*) S + m_i DELTA + e, |e| < 2^30 */
    for (size_t x = 0; x < N; ++x) {
        msgs[x] = (unsigned)(next_u64() & 7);
        ct[x] = next_mod_p();
        ct[K * N + x] = sub_p(add_p((uint64_t)msgs[x] * DELTA, next_u64() >> 33), (uint64_t)1 << 30);
    }
    if (msgs[0] == 0) msgs[0] = 5, ct[K * N] = add_p(ct[K * N], 5 * DELTA);
    mul_binary_acc(ct + K * N, ct, S, 1);

    /* n^-1 mod p in front of the trace, which multiplies the surviving coefficient by n */
    const uint64_t n_inv = pow_p(N, P - 2);
    for (size_t x = 0; x < (K + 1) * N; ++x) ct[x] = mul_p(ct[x], n_inv);

    rc = cntt_prime64_glwe_trace_batch(plan, out, ct, ak, LOGN, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("glwe_trace_batch", rc);

    /* phase = body - mask (*) S; coefficient i is round(phase / DELTA) mod 8 */
    memcpy(phase, out + K * N, N * 8);
    mul_binary_acc(phase, out, S, 0);
    for (size_t i = 0; i < N; ++i) {
        const unsigned got = phase[i] >= P - DELTA / 2 ? 0u : (unsigned)((phase[i] + DELTA / 2) / DELTA) & 7u;
        const unsigned want = i == 0 ? msgs[0] : 0u;
        if (i < 4 || got != want)
            printf("coefficient %u: message %u, after the trace it decrypts to %u%s\n", (unsigned)i, msgs[i], got, got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_prime64_plan_free(plan);
    free(S), free(rot), free(ak), free(ct), free(out), free(phase);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("only the constant coefficient survived the trace of %u steps\nSuccess!\n", LOGN);
    return 0;
}
