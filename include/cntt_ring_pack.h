/* Ring packing of LWE ciphertexts through automorphisms on the native plans (ciphertext modulus 2^32 / 2^64 / 2^128): M = lwe_count LWE
 * ciphertexts become ONE GLWE ciphertext with the log2 n trace keys of the trace header -- the PackLWEs algorithm of Chen, Dai, Kim and
 * Song ("Efficient homomorphic conversion between (ring) LWE ciphertexts", ACNS 2021) -- next to the packing keyswitch of cntt_pack.h, whose
 * key grows with the LWE dimension.  The counterpart mod p is cntt_prime_ring_pack.h, which this file mirrors call for call.  No
 * counterpart in the reference; the convention below is this library's own, fixed to the last bit.  No key or noise generation: the caller
 * brings the keys.  Include this file on its own (it includes cntt_ext.h, which has every type it needs); it is not part of cntt.h or
 * cntt_ext.h.  Plain C11.  "The trace header" below is the header that declares cntt_native_glwe_automorphism_keyswitch_batch and
 * cntt_native_glwe_trace_batch, the native counterpart of cntt_prime_automorphism.h; include it next to this one for those calls.
 *
 * Symbols are those of the trace header: w = the word width of the plan's kind, wb = w / 8 = cntt_native_word_bytes, n = ntt_size,
 * k = glwe_dim, B = 2^base_log, sigma_t the automorphism X -> X^t, a GLWE ciphertext = its k mask polynomials with the body polynomial
 * last, every word little-endian.  All arithmetic is mod 2^w and wraps.  M = lwe_count is a power of two with 1 <= M <= n.  An LWE
 * ciphertext here has k n mask words with the body word last and is encrypted under the flattened GLWE key, s[q n + j] = S_q[j]: what
 * cntt_native_sample_extract_batch writes at index 0.
 *
 * 1. cntt_native_glwe_embed_batch: the inverse of sample extraction at index 0, every kind (the binary ones too: no key is read).
 *    For q < k:
 *      glwe[q][0] = lwe[q n],   glwe[q][i] = -lwe[q n + n - i] mod 2^w for 1 <= i < n,   glwe[k] = (lwe[k n], 0, ..., 0).
 *    Coefficient 0 of the phase of the result is the phase of the LWE ciphertext; the other n - 1 coefficients are junk that the packing
 *    removes.  cntt_native_sample_extract_batch(index = 0) of the result returns lwe word for word.
 *
 * 2. cntt_native_glwe_merge_batch: one node of the packing tree, the five non-binary kinds.  With E = glwe_even[b], O = glwe_odd[b],
 *    polynomial by polynomial,   a = E + X^shift O,   d = E - X^shift O   (X^shift is CNTT_SRC_ROTATE of cntt_gadget.h,
 *    0 <= shift < 2n), and
 *      glwe_out[b] = a + AutoKS_t(d)
 *    with AutoKS_t the Galois keyswitch of the trace header (call 3 there, add_input = 0) against ONE key of that header's residue-plane
 *    layout.  The words are exactly those of this sequence: the prefill out[q] = a[q] for q < k and out[k] = a[k] + sigma_t(d[k]);
 *    the terms = the NEGATED CNTT_SRC_PLAIN digits of sigma_t(d[q]), q < k, in the order (q, l);
 *    cntt_native_external_product_batch(out, terms, ak_ntt, nterms = k levels, nout = k + 1, accumulate = 1).  One kernel reads E and O
 *    once and writes the prefill and the terms; a, d, the rotation and the permutation are never stored.
 *    Phase: with a noise-free key and base_log levels = w, phase(out) = phase(E) + X^shift phase(O) + sigma_t(phase(E) - X^shift phase(O)).
 *
 * 3. cntt_native_ring_pack_batch, the five non-binary kinds.  lwe_in is batch x M LWE ciphertexts, glwe_out batch GLWE ciphertexts, ak_ntt
 *    the FULL trace key array of the trace header: log2 n keys, key r (of t_r = n / 2^r + 1) at residue polynomial r k levels (k + 1) of
 *    every plane.  With l = log2 M:
 *      c_0[j] = the embedding (call 1) of lwe_in[g][j],  j < M;
 *      for s = 1 .. l, h = M / 2^s:  c_s[j] = merge(E = c_(s-1)[j], O = c_(s-1)[j + h], shift = n / 2^s, t = 2^s + 1)  for j < h
 *        -- t = 2^s + 1 is t_r with r = log2 n - s, so stage s uses key r = log2 n - s;
 *      glwe_out[g] = cntt_native_glwe_trace_batch(c_l[0], steps = log2 n - l), which uses the keys 0 .. steps - 1.
 *    The words are exactly those of call 1 on all M ciphertexts, call 2 once per stage on the batch h pairs of that stage, and the trace.
 *    Stage 1 reads the LWE rows directly through the rule of call 1 (the M embedded ciphertexts are never written); a whole packing is
 *    log2 n steps -- log2 M stages and log2 n - log2 M trace rounds -- each one kernel here plus the external product.
 *    LAYOUT AND FACTOR.  With noise-free keys and base_log levels = w, coefficient j (n / M) of the phase of glwe_out[g] is
 *    n * phase(lwe_in[g][j]) mod 2^w and every other coefficient is 0: message j sits at coefficient j n / M, NOT at coefficient j (the
 *    layout is strided, unlike cntt_pack.h), and the factor is n for every M.
 *    WHAT DIFFERS FROM THE PRIME PLANS.  Modulo a prime n is a unit and the caller scales the input by n^-1.  n is NOT a unit mod 2^w: the
 *    top log2 n bits of every phase are gone for good.  The caller therefore encodes with log2 n bits of headroom BELOW the message -- a
 *    message of m bits sits at bit w - log2 n - m, not at bit w - m -- so that the factor moves it to the top of the word.  The noise of
 *    the input grows by the same factor n; of the log2 n steps in all (the stages first, then the trace rounds), the keyswitch noise of
 *    step i = 0 .. log2 n - 1 grows by 2^(log2 n - 1 - i), since every later step doubles what is already there.
 *    examples/ring_pack_native.c decodes that way.
 *
 * Exactness: that of the trace header.  The embedding, the rotation, the sums, the permutation and the digits are wrapping word
 * arithmetic; the external product is cntt_native_external_product_batch word for word, exact while
 * k * levels <= cntt_native_max_terms(plan).  Beyond it calls 2 and 3 return CNTT_EINVAL, the message giving both numbers.
 *
 * Valid: t odd and below 2n; shift < 2n; lwe_count a power of two in 1 .. n; base_log >= 1, levels >= 1, base_log * levels <= w; every
 * size the external product accepts.  batch == 0 does nothing.  k == 0 is valid: no key is read and ak_ntt may be NULL.
 *
 * Operands: the rules of cntt.h and the trace header -- every pointer aligned to its word (a plane to its residue), a written operand
 * disjoint from every other one.  No call here runs in place.  Workspace, with up(x) = x rounded up to a multiple of 256,
 * H = max(M / 2, 1), Q = max(M / 4, 1):
 *   cntt_native_glwe_merge_workspace_bytes = up(batch * k * levels * n * wb)                          (the negated digit polynomials)
 *   cntt_native_ring_pack_workspace_bytes  = up(batch * H * k * levels * n * wb) + up(batch * H * (k + 1) * n * wb)
 *                                            + up(batch * Q * (k + 1) * n * wb)
 *   (the digits of the widest stage and two ciphertext buffers: the stages and the trace steps alternate between them so that the last
 *   operation writes glwe_out).  The rules are those of the trace header: 16-byte aligned, living where the other buffers live; on the
 *   host path it is checked and then not used; NULL on the device path is one stream-ordered allocation for the whole call.  With a caller
 *   workspace the Plan32 kinds at 32 <= n <= 4096 (the fused external product) make no allocation anywhere in the call, which is then a
 *   linear chain of kernels and may be captured into a hipGraph; elsewhere the external product keeps allocating its own scratch.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; a binary kind
 * (calls 2 and 3); t even or t >= 2n; shift >= 2n; lwe_count zero, not a power of two or above n; base_log == 0, levels == 0,
 * base_log * levels > w; k * levels > cntt_native_max_terms(plan); batch * H * max(k * levels, k + 1) >= 2^32 (H = 1 in call 2: what the
 * widest launch of the external product holds); sizes whose ciphertexts, digits or keys would pass 2^63 bytes (checked before they are
 * formed); a NULL argument or a NULL plane (ak_ntt only when k > 0); a misaligned pointer; a non-NULL workspace that is misaligned or too
 * small; a written operand (glwe_out, the workspace) overlapping any other operand (byte ranges).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  The key is log2 n * k * levels * (k + 1) residue polynomials per plane where pksk_ntt of cntt_pack.h at Lin = k n has
 * k n * levels * (k + 1) (102 times more at n = 1024, 186 times at n = 2048); the work is M - 1 Galois keyswitches in log2 M launches plus
 * log2 n - log2 M for the trace.
 * Measured times against cntt_native_pack_keyswitch_batch and against the public-call sequence: profiles/r28_native_ring_pack.txt
 * (tools/native_ring_pack_bench.py takes the figures).
 * Measured at k = 1, n = 1024 / 2048, levels 2 / 4, batch 1 / 16, M = 1 / 32 / n on the 64- and 32-bit Plan32 kinds (one box, the n = 1024
 * rows taken twice: within 2 % run to run): call 3 is 15.5 to 148 times faster than cntt_native_pack_keyswitch_batch at Lin = k n,
 * lwe_count = M -- least at M = n, batch 16, most at n = 2048 with four levels and small M -- and 0.99 to 1.27 times faster than its own
 * public-call sequence (1.00 at M = 1, where the two are the same launches; 1.12 to 1.27 at M = n, batch 16).  Reading the LWE rows as
 * leaves against embedding first: within 0.01 ms of a 0.4 to 1.2 ms call at M = 2, at the noise.  Staging through LDS against the global
 * gather: 0.99 to 1.06, no loss at the default and 4 to 6 % gained at M = n, batch 16; the shared default stays.  128-bit words, the
 * Plan52 kinds and k > 1 were not measured. */
#ifndef CNTT_RING_PACK_H
#define CNTT_RING_PACK_H

#include "cntt_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lwe_in: batch x (k * n + 1) words; glwe_out: batch x (k + 1) polynomials, only written */
int cntt_native_glwe_embed_batch(const cntt_native_t *plan, void *glwe_out, const void *lwe_in, size_t glwe_dim, size_t batch, cntt_mem_t where,
                                 void *stream);

/* glwe_even, glwe_odd, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ak_ntt: planes of k * levels * (k + 1) residue
 * polynomials, one key */
int cntt_native_glwe_merge_batch(const cntt_native_t *plan, void *glwe_out, const void *glwe_even, const void *glwe_odd,
                                 const void *const *ak_ntt, size_t shift, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,
                                 size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_native_glwe_merge_workspace_bytes(const cntt_native_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* lwe_in: batch x lwe_count x (k * n + 1) words; glwe_out: batch x (k + 1) polynomials; ak_ntt: planes of log2 n * k * levels * (k + 1)
 * residue polynomials */
int cntt_native_ring_pack_batch(const cntt_native_t *plan, void *glwe_out, const void *lwe_in, const void *const *ak_ntt, size_t lwe_count,
                                size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                cntt_mem_t where, void *stream);
size_t cntt_native_ring_pack_workspace_bytes(const cntt_native_t *plan, size_t lwe_count, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the two kernels of these calls launch for `polys` output polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest): one per polynomial up to 8 per CU of a 256-CU part, fewer where two staged polynomials (up to 64 KiB together) limit
 * what a CU holds at 160 KiB of LDS.  The rule of cntt_native_automorphism_grid: an assumption about what fills the chip, not a measured
 * optimum.  For tests and tools: pure arithmetic, no device call. */
unsigned cntt_native_ring_pack_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_RING_PACK_H */
