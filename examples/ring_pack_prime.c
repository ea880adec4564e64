/* Ring packing of LWE ciphertexts with a PRIME ciphertext modulus on the C ABI (include/cntt_prime_ring_pack.h); no counterpart in the
 * reference: prime64 plan, p = 2^64 - 2^32 + 1 = 18446744069414584321 (W = 64), n = 256, k = 1, base_log = 16, levels = 4, M = 16.  The
 * program generates a binary GLWE key S and the log2 n = 8 NOISY trace keys of the exponents t_r = n / 2^r + 1 exactly as
 * examples/trace_prime.c does -- row (r, l) of a key is a GLWE encryption of sigma_t(S_r) 2^(64 - 16 l), mask polynomial first, body
 * last, noise below 2^10; all keys back to back, n^-1 fwd(key): cntt_prime64_fwd_batch, then cntt_prime64_normalize_batch -- and
 * encrypts M = 16 LWE ciphertexts under the FLATTENED key s[j] = S[j] (k n = 256 mask words, the body word last), each a 3-bit message
 * m_j (p-1)/8 with noise below 2^30.  Every input word is scaled by n^-1 mod p (the packing multiplies what survives by n; the scaling
 * goes in front so that the keyswitch noise is not scaled with it), ONE cntt_prime64_ring_pack_batch call packs them, the host decrypts
 * and the program exits non-zero unless message j reads at coefficient j n / M = 16 j -- the layout is strided -- and every other
 * coefficient reads 0.  The packing key is 8 * 4 * 2 = 64 polynomials; the packing keyswitch of examples/pack_prime.c would need
 * 256 * 4 * 2 = 2048 at the same digits.  The library generates neither keys nor noise: this file is the recipe.  Host buffers
 * (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_prime_ring_pack.h"

#define P 18446744069414584321ull
#define N 256u
#define LOGN 8u
#define K 1u
#define BASE_LOG 16u
#define LEVELS 4u
#define M 16u
#define DELTA ((P - 1) / 8) /* one message step */

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
    const size_t key_polys = (size_t)K * LEVELS * (K + 1), nkey = LOGN * key_polys, row = (size_t)K * N + 1;
    uint64_t *S = malloc(N * 8), *rot = malloc(N * 8), *ak = calloc(nkey * N, 8);
    uint64_t *lwe = calloc(M * row, 8), *out = calloc((K + 1) * N, 8), *phase = malloc(N * 8);
    unsigned msgs[M];
    cntt_plan64_t *plan = NULL;
    int rc = cntt_prime64_plan_new(N, P, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (!S || !rot || !ak || !lwe || !out || !phase) return 1;

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;

    /* The trace keys.  Key r belongs to t = n / 2^r + 1; sigma_t(S) by the scatter that defines it: X^i -> (-1)^floor(i t / n)
     * X^(i t mod n).  Row l: mask A uniform, body = A (*) S + e + sigma_t(S) 2^(64 - BASE_LOG l), |e| < 2^10 per coefficient. */
    for (size_t r = 0; r < LOGN; ++r) {
        const size_t t = (N >> r) + 1;
        memset(rot, 0, N * 8);
        for (size_t i = 0; i < N; ++i) {
            const size_t e = i * t % (2 * N);
            rot[e % N] = e >= N ? sub_p(0, S[i]) : S[i];
        }
        for (size_t l = 1; l <= LEVELS; ++l) {
            uint64_t *kr = ak + (r * key_polys + (l - 1) * (K + 1)) * N; /* AK[l - 1][0 .. K] */
            for (size_t x = 0; x < N; ++x) {
                kr[x] = next_mod_p();
                kr[K * N + x] = sub_p(next_u64() >> 53, (uint64_t)1 << 10);
            }
            mul_binary_acc(kr + K * N, kr, S, 1);
            for (size_t x = 0; x < N; ++x) kr[K * N + x] = add_p(kr[K * N + x], mul_p(rot[x], (uint64_t)1 << (64 - BASE_LOG * l)));
        }
    }
    /* the keys the call reads: n^-1 fwd(key) */
    rc = cntt_prime64_fwd_batch(plan, ak, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(ak)", rc);
    rc = cntt_prime64_normalize_batch(plan, ak, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("normalize_batch(ak)", rc);

    /* M LWE ciphertexts under the flattened key: body = <mask, S> + m_j DELTA + e, |e| < 2^30; then every word times n^-1 mod p, in
     * front of the packing, which multiplies the messages by n */
    const uint64_t n_inv = pow_p(N, P - 2);
    for (size_t j = 0; j < M; ++j) {
        uint64_t *ct = lwe + j * row;
        msgs[j] = (unsigned)(next_u64() & 7);
        if (j == 0 && msgs[0] == 0) msgs[0] = 5;
        uint64_t body = sub_p(add_p((uint64_t)msgs[j] * DELTA, next_u64() >> 33), (uint64_t)1 << 30);
        for (size_t x = 0; x < N; ++x) {
            ct[x] = next_mod_p();
            if (S[x]) body = add_p(body, ct[x]);
        }
        ct[K * N] = body;
        for (size_t x = 0; x < row; ++x) ct[x] = mul_p(ct[x], n_inv);
    }

    rc = cntt_prime64_ring_pack_batch(plan, out, lwe, ak, M, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("ring_pack_batch", rc);

    /* phase = body - mask (*) S; coefficient i is round(phase / DELTA) mod 8; message j sits at coefficient j n / M */
    memcpy(phase, out + K * N, N * 8);
    mul_binary_acc(phase, out, S, 0);
    for (size_t i = 0; i < N; ++i) {
        const unsigned got = phase[i] >= P - DELTA / 2 ? 0u : (unsigned)((phase[i] + DELTA / 2) / DELTA) & 7u;
        const unsigned want = i % (N / M) == 0 ? msgs[i / (N / M)] : 0u;
        if (i % (N / M) == 0)
            printf("message %2u = %u: coefficient %3u decrypts to %u%s\n", (unsigned)(i / (N / M)), want, (unsigned)i, got, got == want ? "" : "  WRONG");
        else if (got != want)
            printf("coefficient %u decrypts to %u, not 0  WRONG\n", (unsigned)i, got);
        wrong += got != want;
    }
    cntt_prime64_plan_free(plan);
    free(S), free(rot), free(ak), free(lwe), free(out), free(phase);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("every message decoded at its strided coefficient; the other %u coefficients are 0\nSuccess!\n", N - M);
    return 0;
}
