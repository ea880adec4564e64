/* The LWE-to-GLWE packing keyswitch of the prime32 / prime64 plans on the device -- the way back from the LWE ciphertexts a bootstrap
 * or a keyswitch modulo a prime ends in to ONE GLWE ciphertext that encrypts sum_t m_t X^t, so that packed results and repacked table
 * inputs stay on the device.  It runs through the NTT mod p: the sum over the packed ciphertexts is an external product of digit
 * polynomials against an NTT-domain key -- one transform per digit polynomial, no residue split, no CRT.  No counterpart in the
 * reference; the convention below is this library's own, fixed to the last bit so that an integrator can generate matching keys.  No
 * key or noise generation: the caller brings the key.  Include this file on its own (it includes cntt_prime_keyswitch.h); it is not
 * part of cntt_ext.h.  Plain C11.
 *
 * Symbols: T = the plan's word (uint32_t / uint64_t), p = the modulus, W = the bit length of p, n = ntt_size, k = glwe_dim,
 * Lin = lwe_dim_in, m = lwe_count (1 <= m <= n: the LWE ciphertexts packed into one GLWE), B = 2^base_log.  An LWE ciphertext is its
 * mask words with the body last and a GLWE ciphertext its k mask polynomials with the body polynomial last, as in cntt_prime_pbs.h.
 * Batch element g packs the m ciphertexts in[g][0 .. m - 1]:
 *
 *   out[g][q] = [q == k] * sum_{t < m} in[g][t][Lin] X^t  -  sum_{i < Lin} sum_{l = 1 .. levels} D_{g,i,l} (*) K[i * levels + l - 1][q]
 *               mod p,  for q <= k
 *
 * D_{g,i,l} is the polynomial of digits with coefficient t equal to d_l(in[g][t][i]) for t < m and 0 for t >= m; d_1 .. d_levels are
 * exactly the digits of cntt_prime_pbs.h of the plain word (no rotation): taken from the balanced lift x', rounded to
 * 2^(W - base_log * levels), d_1 most significant; the levels below the top lie in [-B/2, B/2), the top digit d_1 is unmasked and
 * lies in [-B/2, B/2].  (*) is the negacyclic product in Z_p[X]/(X^n + 1).  The body words in[g][t][Lin] are not decomposed.  Every
 * output word is canonical (< p).
 *
 * Key layout.  pksk_ntt is ONE array of Lin * levels * (k + 1) NTT-domain polynomials, K[r][q] at index r * (k + 1) + q, holding
 * n^-1 * fwd(key polynomial): exactly what one cntt_prime*_fwd_batch followed by one cntt_prime*_normalize_batch over all key
 * polynomials in that order writes -- the convention of bsk_ntt in cntt_prime_pbs.h, because the fused chain returns the unnormalised
 * inverse transform.  Row r = i * levels + (l - 1) is a GLWE encryption under the OUTPUT key (k mask polynomials, body last) of the
 * constant polynomial s_in[i] * 2^(W - base_log * l) mod p.
 *
 * Phase.  With a noise-free key, s = W - base_log * levels and r_{t,i} the rounded number of cntt_prime_pbs.h of in[g][t][i]
 * (r_{t,i} * 2^s = sum_l d_l 2^(W - base_log * l) as integers, |r_{t,i} * 2^s - lift(in[g][t][i])| <= 2^(s-1), = 0 when s = 0), the phase
 * of the output under the output key is, per coefficient t,
 *   phase(out[g])[t] = in[g][t][Lin] - sum_i s_in[i] * r_{t,i} * 2^s  mod p   for t < m,      phase(out[g])[t] = 0   for t >= m
 * i.e. coefficient t carries the phase of LWE t under s_in, up to the rounding, and the coefficients t >= m are zero.
 *
 * The words are exactly those of a sequence of existing public calls.  The mask words are walked in chunks of
 *   C = max(1, CNTT_PRIME_PACK_TERMS / levels)
 * words, capped at Lin (there is no max_terms here: the accumulation is modular).  out starts as the body polynomial, mask
 * polynomials zero.  Then, per chunk [i0, i0 + c): form the polynomials P_i[t] = in[g][t][i], zero for t >= m;
 * cntt_prime*_gadget_decompose_batch(CNTT_SRC_PLAIN, npolys = c) gives the digit polynomials in the order (i, l); negate each digit
 * mod p, with 0 staying 0; cntt_prime*_external_product_batch(out, those terms, key slice from row i0 * levels, nterms = c * levels,
 * nout = k + 1, accumulate = 1) accumulates into out.
 *
 * Exactness.  The decomposition, the transpose and the body are exact integer arithmetic for every prime the plans accept.  The
 * external product is cntt_prime*_external_product_batch word for word, so the "Exactness" caveat of cntt_prime_pbs.h applies: for
 * primes of the reference's strict range (2^62 <= p < 2^63 on 64-bit words, 2^30 <= p < 2^31 on 32-bit words) it is the reference's
 * composition fwd / mul_accumulate / inv with its wrapping Barrett product.  The call therefore equals the public-call sequence above
 * for EVERY prime, and equals the big-integer formula at the top only outside that caveat.
 *
 * Valid: base_log >= 1, levels >= 1, base_log * levels <= W (the digits are full words: no cap of 31 as in the LWE keyswitch),
 * 1 <= m <= n, every size the external product accepts.  Lin == 0 writes the body polynomial only (pksk_ntt may then be NULL).
 * batch == 0 does nothing.  Input or key words >= p are not rejected and not reduced: the call completes without a fault and the
 * affected outputs are unspecified.
 *
 * Cost.  The direct route -- cntt_prime*_keyswitch_batch on the m ciphertexts with rows of (k + 1) n words, then rotate and sum -- costs
 * m * Lin * levels * (k + 1) * n multiply-accumulates; this one about Lin * levels * (n log n + (k + 1) n), whatever m is.  Measured
 * times of both routes, and where this one overtakes the direct route (at n = 1024 and batches of 1 and 16: only at 16384 rows on
 * 32-bit words; the call is launch-bound there): profiles/r14_prime_pack.txt (tools/prime_pack_bench.py takes the figures). */
#ifndef CNTT_PRIME_PACK_H
#define CNTT_PRIME_PACK_H

#include "cntt_prime_keyswitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Terms of one external product of the packing keyswitch at most (before the division by levels).  64 is the starting value, that of
 * CNTT_PACK_TERMS: no same-machine A/B against 32 / 128 has been recorded yet (profiles/r14_prime_pack.txt). */
#define CNTT_PRIME_PACK_TERMS 64

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* lwe_in: batch x m x (Lin + 1) words; glwe_out: batch x (k + 1) polynomials, only written; pksk_ntt as above.
 * Workspace (the negated digit polynomials of one chunk), with up(x) = x rounded up to a multiple of 256:
 *   cntt_prime64_pack_workspace_bytes = up(batch * C * levels * n * sizeof(T))          (C as above, capped at Lin)
 * The rules are those of cntt_prime_pbs.h: 16-byte aligned, living where the other buffers live; NULL on the device path is one
 * stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain (n <= 2048 on 64-bit words,
 * n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear chain of kernels and may be
 * captured into a hipGraph; elsewhere the composed external product keeps its own per-call scratch.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan,
 * base_log == 0, levels == 0, base_log * levels > W, lwe_count == 0 or lwe_count > n, a NULL argument, a NULL key with Lin > 0,
 * glwe_out overlapping lwe_in, pksk_ntt or the workspace, lwe_in overlapping the workspace (byte ranges), a non-NULL workspace that is
 * misaligned or too small, batch * max(C * levels, k + 1) >= 2^32 (what one launch of the external product holds), Lin * levels >= 2^32,
 * and sizes whose ciphertexts, key or output would pass 2^63 bytes (the byte counts are checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises. */
int cntt_prime64_pack_keyswitch_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *lwe_in, const uint64_t *pksk_ntt,
                                      size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels,
                                      size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* the formula above; 0 for a NULL plan or levels == 0 */
size_t cntt_prime64_pack_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim_in, unsigned levels, size_t batch);

/* ---- prime32: the same two calls on 32-bit words ---------------------------------------------------------------------------------- */
int cntt_prime32_pack_keyswitch_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *lwe_in, const uint32_t *pksk_ntt,
                                      size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels,
                                      size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_pack_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim_in, unsigned levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_PACK_H */
