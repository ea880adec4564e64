/* Ring packing of LWE ciphertexts with the ciphertext modulus 2^64 on the C ABI (include/cntt_ring_pack.h); no counterpart in the
 * reference: native64 Plan32, n = 256, k = 1, M = 16, base_log = 8, levels = 6.  The counterpart of ring_pack_prime.c, and the one thing
 * that differs is the encoding: the packing multiplies every message by n = 2^8, which is not a unit mod 2^64, so a 3-bit message sits at
 * bit 64 - 8 - 3 = 53 -- eight bits of headroom BELOW the message -- and comes out at bit 61, the top of the word.  The program generates
 * a binary GLWE key S and the log2 n = 8 NOISY automorphism keys of the exponents t_r = n / 2^r + 1 exactly as trace_native.c does (noise
 * below 2^10; all keys back to back, then ONE cntt_native_fwd_batch into the five residue planes), encrypts M LWE ciphertexts under the
 * flattened key s[j] = S[j] (noise below 2^20), packs them in one cntt_native_ring_pack_batch call, decrypts on the host and exits non-zero
 * unless coefficient j n / M reads message j and every other coefficient reads 0.  The library generates neither keys nor noise: this
 * file is the recipe.  Host buffers (CNTT_MEM_HOST) throughout. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/cntt_ring_pack.h"

#define N 256u
#define LOGN 8u
#define K 1u
#define M 16u
#define BASE_LOG 8u
#define LEVELS 6u
#define NPRIMES 5
#define IN_SHIFT (64u - LOGN - 3u) /* where the message goes in */
#define OUT_SHIFT 61u               /* where it comes out: n = 2^LOGN times higher */

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

/* acc -= a (*) S in Z/2^64[X]/(X^n + 1) for the binary key S (sign = 0), or acc += a (*) S (sign = 1): unsigned arithmetic wraps */
static void mul_binary_acc(uint64_t *acc, const uint64_t *a, const uint64_t *S, int sign) {
    for (size_t b = 0; b < N; ++b) {
        if (!S[b]) continue;
        for (size_t i = 0; i < N; ++i) {
            const int plus = (i + b < N) == (sign != 0);
            uint64_t *dst = acc + (i + b) % N;
            *dst = plus ? *dst + a[i] : *dst - a[i];
        }
    }
}

int main(void) {
    const size_t key_polys = (size_t)K * LEVELS * (K + 1), nkey = LOGN * key_polys, row = K * N + 1;
    uint64_t *S = malloc(N * 8), *rot = malloc(N * 8), *ak = calloc(nkey * N, 8);
    uint64_t *lwe = calloc(M * row, 8), *out = calloc((K + 1) * N, 8), *phase = malloc(N * 8);
    uint32_t *plane[NPRIMES];
    const void *key[NPRIMES];
    unsigned msgs[M];
    cntt_native_t *plan = NULL;
    int rc = cntt_native_plan_new(CNTT_NATIVE64_PLAN32, N, &plan), wrong = 0;
    if (rc != CNTT_OK) return die("plan", rc);
    if (!S || !rot || !ak || !lwe || !out || !phase || cntt_native_nprimes(plan) != NPRIMES) return 1;
    for (int i = 0; i < NPRIMES; ++i) {
        if (!(plane[i] = malloc(nkey * N * 4))) return 1;
        key[i] = plane[i];
    }

    for (size_t i = 0; i < N; ++i) S[i] = next_u64() & 1;

    /* The automorphism keys.  Key r belongs to t = n / 2^r + 1.  sigma_t(S) by the scatter that defines it: X^i ->
     * (-1)^floor(i t / n) X^(i t mod n).  Row l: mask A uniform, body = A (*) S + e + sigma_t(S) 2^(64 - BASE_LOG l), |e| < 2^10. */
    for (size_t r = 0; r < LOGN; ++r) {
        const size_t t = (N >> r) + 1;
        memset(rot, 0, N * 8);
        for (size_t i = 0; i < N; ++i) {
            const size_t e = i * t % (2 * N);
            rot[e % N] = e >= N ? 0 - S[i] : S[i];
        }
        for (size_t l = 1; l <= LEVELS; ++l) {
            uint64_t *krow = ak + (r * key_polys + (l - 1) * (K + 1)) * N; /* AK[l - 1][0 .. K] */
            for (size_t x = 0; x < N; ++x) {
                krow[x] = next_u64();
                krow[K * N + x] = (next_u64() >> 53) - ((uint64_t)1 << 10);
            }
            mul_binary_acc(krow + K * N, krow, S, 1);
            for (size_t x = 0; x < N; ++x) krow[K * N + x] += rot[x] << (64 - BASE_LOG * l);
        }
    }
    /* the keys the call reads: the residue planes of one forward transform over all key polynomials */
    rc = cntt_native_fwd_batch(plan, ak, (void *const *)plane, nkey, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("fwd_batch(ak)", rc);

    /* M LWE ciphertexts under the flattened key, the message LOGN bits below the top: body = <a, s> + m_j 2^53 + e, |e| < 2^20 */
    for (size_t j = 0; j < M; ++j) {
        uint64_t *c = lwe + j * row, dot = 0;
        msgs[j] = (unsigned)(next_u64() & 7);
        for (size_t x = 0; x < N; ++x) {
            c[x] = next_u64();
            if (S[x]) dot += c[x];
        }
        c[K * N] = dot + ((uint64_t)msgs[j] << IN_SHIFT) + (next_u64() >> 43) - ((uint64_t)1 << 20);
    }

    rc = cntt_native_ring_pack_batch(plan, out, lwe, key, M, K, BASE_LOG, LEVELS, 1, NULL, 0, CNTT_MEM_HOST, NULL);
    if (rc != CNTT_OK) return die("ring_pack_batch", rc);

    /* phase = body - mask (*) S; coefficient i is round(phase / 2^61) mod 8; message j sits at coefficient j n / M */
    memcpy(phase, out + K * N, N * 8);
    mul_binary_acc(phase, out, S, 0);
    for (size_t i = 0; i < N; ++i) {
        const unsigned got = (unsigned)(((phase[i] >> (OUT_SHIFT - 1)) + 1) >> 1) & 7u;
        const unsigned want = i % (N / M) == 0 ? msgs[i / (N / M)] : 0u;
        if ((i % (N / M) == 0 && i < 4 * (N / M)) || got != want)
            printf("coefficient %u: expected %u, after the packing it decrypts to %u%s\n", (unsigned)i, want, got, got == want ? "" : "  WRONG");
        wrong += got != want;
    }
    cntt_native_plan_free(plan);
    for (int i = 0; i < NPRIMES; ++i) free(plane[i]);
    free(S), free(rot), free(ak), free(lwe), free(out), free(phase);
    if (wrong) {
        fprintf(stderr, "MISMATCH\n");
        return 2;
    }
    printf("%u messages packed at stride %u, read with %u bits of headroom below the message\nSuccess!\n", M, N / M, LOGN);
    return 0;
}
