/* Ring packing of LWE ciphertexts through automorphisms on the prime32 / prime64 plans: M = lwe_count LWE ciphertexts become ONE GLWE
 * ciphertext with the log2 n trace keys of cntt_prime_automorphism.h -- the PackLWEs algorithm of Chen, Dai, Kim and Song ("Efficient
 * homomorphic conversion between (ring) LWE ciphertexts", ACNS 2021) -- next to the packing keyswitch of cntt_prime_pack.h, whose key
 * grows with the LWE dimension.  No counterpart in the reference; the convention below is this library's own, fixed to the last bit.  No
 * key or noise generation: the caller brings the keys.  Include this file on its own (it includes cntt_prime_automorphism.h); it is not
 * part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_prime_automorphism.h: T = the plan's word, p = the modulus, W = the bit length of p, n = ntt_size,
 * k = glwe_dim, B = 2^base_log, sigma_t the automorphism X -> X^t, a GLWE ciphertext = its k mask polynomials with the body polynomial
 * last.  M = lwe_count is a power of two with 1 <= M <= n.  An LWE ciphertext here has k n mask words with the body word last and is
 * encrypted under the flattened GLWE key, s[q n + j] = S_q[j]: what cntt_prime*_sample_extract_batch writes at index 0.
 *
 * 1. glwe_embed_batch: the inverse of sample extraction at index 0.  For q < k:
 *      glwe[q][0] = lwe[q n],   glwe[q][i] = -lwe[q n + n - i] mod p for 1 <= i < n (0 stays 0),   glwe[k] = (lwe[k n], 0, ..., 0).
 *    Coefficient 0 of the phase of the result is the phase of the LWE ciphertext; the other n - 1 coefficients are junk that the packing
 *    removes.  cntt_prime*_sample_extract_batch(index = 0) of the result returns lwe word for word.
 *
 * 2. glwe_merge_batch: one node of the packing tree.  With E = glwe_even[b], O = glwe_odd[b], polynomial by polynomial and canonical
 *    mod p,   a = E + X^shift O,   d = E - X^shift O   (X^shift is CNTT_SRC_ROTATE of cntt_prime_pbs.h, 0 <= shift < 2n), and
 *      glwe_out[b] = a + AutoKS_t(d)
 *    with AutoKS_t the Galois keyswitch of cntt_prime_automorphism.h (call 3 there, add_input = 0) against ONE key of that header's
 *    layout.  The words are exactly those of this sequence: the prefill out[q] = a[q] for q < k and out[k] = a[k] + sigma_t(d[k]) mod p;
 *    the terms = the NEGATED CNTT_SRC_PLAIN digits of sigma_t(d[q]), q < k, in the order (q, l);
 *    cntt_prime*_external_product_batch(out, terms, ak_ntt, nterms = k levels, nout = k + 1, accumulate = 1).  One kernel reads E and O
 *    once and writes the prefill and the terms; a, d, the rotation and the permutation are never stored.
 *    Phase: with a noise-free key and base_log levels = W, phase(out) = phase(E) + X^shift phase(O) + sigma_t(phase(E) - X^shift phase(O)).
 *
 * 3. ring_pack_batch.  lwe_in is batch x M LWE ciphertexts, glwe_out batch GLWE ciphertexts, ak_ntt the FULL trace key array of
 *    cntt_prime_automorphism.h: log2 n keys, key r (of t_r = n / 2^r + 1) at polynomial r k levels (k + 1).  With l = log2 M:
 *      c_0[j] = the embedding (call 1) of lwe_in[g][j],  j < M;
 *      for s = 1 .. l, h = M / 2^s:  c_s[j] = merge(E = c_(s-1)[j], O = c_(s-1)[j + h], shift = n / 2^s, t = 2^s + 1)  for j < h
 *        -- t = 2^s + 1 is t_r with r = log2 n - s, so stage s uses key r = log2 n - s;
 *      glwe_out[g] = cntt_prime*_glwe_trace_batch(c_l[0], steps = log2 n - l), which uses the keys 0 .. steps - 1.
 *    The words are exactly those of call 1 on all M ciphertexts, call 2 once per stage on the batch h pairs of that stage, and the trace.
 *    Stage 1 reads the LWE rows directly through the rule of call 1 (the M embedded ciphertexts are never written); a whole packing is
 *    log2 n steps -- log2 M stages and log2 n - log2 M trace rounds -- each one kernel here plus the external product.
 *    LAYOUT AND FACTOR.  With noise-free keys and base_log levels = W, coefficient j (n / M) of the phase of glwe_out[g] is
 *    n * phase(lwe_in[g][j]) mod p and every other coefficient is 0: message j sits at coefficient j n / M, NOT at coefficient j (the
 *    layout is strided, unlike cntt_prime_pack.h), and the factor is n for every M.  Modulo a prime n is a unit: the caller removes the
 *    factor by scaling the INPUT LWE words, every word times n^-1 mod p, before the call, for the reason the trace of
 *    cntt_prime_automorphism.h gives -- the packing is linear in the phase, so the messages come out unscaled with the keyswitch noise
 *    on top, where scaling the output would multiply that noise by n^-1, which is not a small number.
 *
 * Exactness: that of cntt_prime_automorphism.h.  The embedding, the rotation, the sums, the permutation and the digits are exact
 * integer arithmetic for every prime the plans accept; the external product is cntt_prime*_external_product_batch word for word, so the
 * calls equal the public-call sequences above for EVERY prime and the big-integer formulas outside the strict-range caveat of
 * cntt_prime_pbs.h.
 *
 * Valid: t odd and below 2n; shift < 2n; lwe_count a power of two in 1 .. n; base_log >= 1, levels >= 1, base_log * levels <= W; every
 * size the external product accepts.  batch == 0 does nothing.  k == 0 is valid: no key is read and ak_ntt may be NULL.  Words >= p are
 * not rejected and not reduced: the call completes without a fault and the affected outputs are unspecified.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word, a written operand disjoint from every other one.  No call here
 * runs in place.  Workspace, with up(x) = x rounded up to a multiple of 256, H = max(M / 2, 1), Q = max(M / 4, 1):
 *   cntt_prime*_glwe_merge_workspace_bytes = up(batch * k * levels * n * sizeof(T))                   (the negated digit polynomials)
 *   cntt_prime*_ring_pack_workspace_bytes  = up(batch * H * k * levels * n * sizeof(T)) + up(batch * H * (k + 1) * n * sizeof(T))
 *                                            + up(batch * Q * (k + 1) * n * sizeof(T))
 *   (the digits of the widest stage and two ciphertext buffers: the stages and the trace steps alternate between them so that the last
 *   operation writes glwe_out).  The rules are those of cntt_prime_automorphism.h: 16-byte aligned, living where the other buffers live;
 *   NULL on the device path is one stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain
 *   (n <= 2048 on 64-bit words, n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear
 *   chain of kernels and may be captured into a hipGraph.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for everything
 * cntt_prime_automorphism.h refuses -- a NULL plan, t even or t >= 2n, base_log == 0, levels == 0, base_log * levels > W, a NULL argument
 * (ak_ntt only when k > 0), a misaligned pointer, a non-NULL workspace that is misaligned or too small -- and for lwe_count zero, not a
 * power of two or above n; shift >= 2n; batch * H * max(k * levels, k + 1) >= 2^32 (H = 1 in call 2: what the widest launch of the
 * external product holds); sizes whose ciphertexts, digits or keys would pass 2^63 bytes (checked before they are formed); a written
 * operand (glwe_out, the workspace) overlapping any other operand (byte ranges).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  The key is log2 n * k * levels * (k + 1) polynomials where pksk_ntt of cntt_prime_pack.h at Lin = k n has
 * k n * levels * (k + 1); the work is M - 1 Galois keyswitches in log2 M launches plus log2 n - log2 M for the trace.  Measured times
 * against cntt_prime*_pack_keyswitch_batch and against the public-call sequence: profiles/r20_prime_ring_pack.txt
 * (tools/prime_ring_pack_bench.py takes the figures). */
#ifndef CNTT_PRIME_RING_PACK_H
#define CNTT_PRIME_RING_PACK_H

#include "cntt_prime_automorphism.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* lwe_in: batch x (k * n + 1) words; glwe_out: batch x (k + 1) polynomials, only written */
int cntt_prime64_glwe_embed_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *lwe_in, size_t glwe_dim, size_t batch,
                                  cntt_mem_t where, void *stream);

/* glwe_even, glwe_odd, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ak_ntt: k * levels * (k + 1) polynomials, one key */
int cntt_prime64_glwe_merge_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *glwe_even, const uint64_t *glwe_odd,
                                  const uint64_t *ak_ntt, size_t shift, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,
                                  size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_prime64_glwe_merge_workspace_bytes(const cntt_plan64_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* lwe_in: batch x lwe_count x (k * n + 1) words; glwe_out: batch x (k + 1) polynomials; ak_ntt: log2 n * k * levels * (k + 1) polynomials */
int cntt_prime64_ring_pack_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *lwe_in, const uint64_t *ak_ntt,
                                 size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime64_ring_pack_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_count, size_t glwe_dim, unsigned levels, size_t batch);

/* ---- prime32: the same five calls on 32-bit words --------------------------------------------------------------------------------- */
int cntt_prime32_glwe_embed_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *lwe_in, size_t glwe_dim, size_t batch,
                                  cntt_mem_t where, void *stream);
int cntt_prime32_glwe_merge_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *glwe_even, const uint32_t *glwe_odd,
                                  const uint32_t *ak_ntt, size_t shift, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,
                                  size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_glwe_merge_workspace_bytes(const cntt_plan32_t *plan, size_t glwe_dim, unsigned levels, size_t batch);
int cntt_prime32_ring_pack_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *lwe_in, const uint32_t *ak_ntt,
                                 size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_ring_pack_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_count, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the two kernels of these calls launch for `polys` output polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest): one per polynomial up to 8 per CU of a 256-CU part, fewer where two staged polynomials limit what a CU holds.  For
 * tests and tools, like cntt_prime_automorphism_grid: pure arithmetic, no device call. */
unsigned cntt_prime_ring_pack_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_RING_PACK_H */
