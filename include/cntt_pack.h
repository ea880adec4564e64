/* Part of cntt_ext.h (which includes this file; include that one): the LWE-to-GLWE packing keyswitch of the native / native_binary
 * plans on the device -- the way back from the LWE ciphertexts a bootstrap or a keyswitch ends in to ONE GLWE ciphertext that
 * encrypts sum_t m_t X^t.  It runs through the NTT: the sum over the packed ciphertexts is an external product of digit polynomials
 * against an NTT-domain key.  No counterpart in the reference; the convention below is this library's own, fixed to the last bit so
 * that an integrator can generate matching keys.  No key or noise generation: the caller brings the key.  Plain C11.
 *
 * Symbols: w = word width of the plan's kind (32, 64, 128), n = ntt_size, k = glwe_dim, Lin = lwe_dim_in, m = lwe_count
 * (1 <= m <= n: the LWE ciphertexts packed into one GLWE), B = 2^base_log.  An LWE ciphertext is its mask words with the body last
 * and a GLWE ciphertext its k mask polynomials with the body polynomial last, as in cntt_pbs.h.  Batch element g packs the m
 * ciphertexts in[g][0 .. m - 1]:
 *
 *   out[g][p] = [p == k] * sum_{t < m} in[g][t][Lin] X^t  -  sum_{i < Lin} sum_{l = 1 .. levels} D_{g,i,l} (*) K[i * levels + l - 1][p]
 *               mod 2^w,  for p <= k
 *
 * D_{g,i,l} is the polynomial of small digits with coefficient t equal to d_l(in[g][t][i]) for t < m and 0 for t >= m; d_1 .. d_levels
 * are the signed digits of cntt_gadget.h of the plain word (no rotation): the closest multiple of 2^(w - base_log * levels), ties up,
 * wrapping at the top; digits in [-B/2, B/2), d_1 most significant, the carry out of level 1 dropped.  (*) is negacyclic_polymul in
 * Z/2^w[X]/(X^n + 1).  The body words in[g][t][Lin] are not decomposed.
 *
 * Key layout.  pksk_ntt is nprimes pointers; plane j holds Lin * levels * (k + 1) residue polynomials, K[r][p] at index
 * r * (k + 1) + p: exactly what ONE cntt_native_fwd_batch (cntt_native_fwd_binary_batch for the binary kinds: the key is the binary
 * operand) over all key polynomials in that order writes -- unnormalised, bit-reversed, the convention of bsk_ntt in cntt_pbs.h.
 * Row r = i * levels + (l - 1) is a GLWE encryption under the OUTPUT key (k mask polynomials, body last) of the constant polynomial
 * s_in[i] * 2^(w - base_log * l).  With a noise-free key, s = w - base_log * levels and r_{t,i} the rounded (base_log * levels)-bit
 * number of cntt_gadget.h of in[g][t][i], the phase of the output under the output key is
 *   phase(out[g]) = sum_{t < m} X^t (in[g][t][Lin] - sum_i s_in[i] * r_{t,i} * 2^s)   mod 2^w
 * i.e. coefficient t carries the phase of LWE t under s_in, up to the rounding, and the coefficients t >= m are zero.
 *
 * The words are exactly those of a sequence of existing calls.  The mask words are walked in chunks of
 *   C = max(1, min(cntt_native_max_terms(plan), CNTT_PACK_TERMS) / levels)
 * words, capped at Lin.  The accumulator out starts from the body polynomial (mask polynomials zero); then, per chunk [i0, i0 + c),
 * `terms` = the digit polynomials negated mod 2^w, terms[g][(i - i0) * levels + l - 1][t] = -d_l(in[g][t][i]), and
 * cntt_native_external_product_batch(out, terms, key slice from row i0 * levels, nterms = c * levels, nout = k + 1, accumulate = 1).
 *
 * Valid: base_log >= 1, levels >= 1, base_log * levels <= w (the digits of cntt_gadget.h), levels <= cntt_native_max_terms(plan),
 * 1 <= m <= n.  Every kind and every size the external product accepts.  Lin == 0 writes the body polynomial only (pksk_ntt and its
 * planes may then be NULL).  batch == 0 does nothing.
 *
 * Cost.  The direct route -- cntt_native_keyswitch_batch on the m ciphertexts with rows of (k + 1) n words, then rotate and sum --
 * costs m * Lin * levels * (k + 1) * n multiply-accumulates; this one about Lin * levels * (n log n + (k + 1) n), whatever m is.
 * The m at which it overtakes the direct route has NOT been measured (profiles/r11_native_pack.txt: no GPU could be reached;
 * tools/native_pack_bench.py takes the figures). */
#ifndef CNTT_PACK_H
#define CNTT_PACK_H

#include "cntt_keyswitch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Terms of one external product of the packing keyswitch at most (before the division by levels and the cap of
 * cntt_native_max_terms).  64 is the starting value: no same-machine A/B against 32 / 128 has been recorded yet
 * (profiles/r11_native_pack.txt). */
#define CNTT_PACK_TERMS 64

/* lwe_in: batch x m x (Lin + 1) words; glwe_out: batch x (k + 1) polynomials, only written; pksk_ntt as above.
 * Workspace (the negated digit polynomials of one chunk), with up(x) = x rounded up to a multiple of 256 and wb = w / 8:
 *   cntt_native_pack_workspace_bytes = up(batch * C * levels * n * wb)          (C as above, capped at Lin)
 * 16-byte aligned, living where the other buffers live; NULL on the device path is one stream-ordered allocation for the whole call.
 * With a caller workspace the Plan32 kinds at 32 <= n <= 4096 make no allocation anywhere in the call, which is then a linear chain of
 * kernels and may be captured into a hipGraph.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for base_log == 0, levels == 0,
 * base_log * levels > w, levels > cntt_native_max_terms(plan), lwe_count == 0 or lwe_count > n, a NULL argument, a NULL key plane
 * with Lin > 0, glwe_out overlapping lwe_in or the workspace, lwe_in overlapping the workspace (byte ranges), and a non-NULL
 * workspace that is misaligned or too small.  where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device
 * path, copies out and synchronises. */
int cntt_native_pack_keyswitch_batch(const cntt_native_t *plan, void *glwe_out, const void *lwe_in, const void *const *pksk_ntt,
                                     size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
                                     void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* the formula above; 0 for a NULL plan or levels == 0 */
size_t cntt_native_pack_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim_in, unsigned levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PACK_H */
