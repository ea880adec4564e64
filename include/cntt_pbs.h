/* Part of cntt_ext.h (which includes this file; include that one): the TFHE programmable bootstrap of the native / native_binary plans
 * on the device -- modulus switch of the LWE words, accumulator set-up, the blind rotation loop in place, sample extraction -- as
 * four calls, and one call that runs them all.  The loop runs the kernels of cntt_gadget.h (CNTT_SRC_CMUX decomposition) and of
 * cntt_native_external_product_batch (accumulate = 1) once per LWE mask word, into ONE accumulator and ONE digit scratch.  No
 * counterpart in the reference.  The keyswitch back to dimension L, alone and in one call with the bootstrap, is in cntt_keyswitch.h.
 * No key or noise generation: the caller brings the keys.  Plain C11.
 *
 * Symbols: w = word width of the plan's kind (32, 64, 128), n = ntt_size = 2^logn, k = glwe_dim, L = lwe_dim.
 *
 * Data layouts:
 *   - An LWE ciphertext is L + 1 words with the body last.
 *   - A GLWE ciphertext is k + 1 polynomials with the body last.
 *   - A batch puts its elements back to back.
 *
 * Workspace.  With wb = w / 8 and up(x) = x rounded up to a multiple of 256:
 *   digits = batch * (k + 1) * levels * n * wb        (the terms of one iteration)
 *   rot    = (L + 1) * batch * 4                      (rot_t)
 *   acc    = batch * (k + 1) * n * wb                 (the accumulator)
 *   cntt_native_pbs_workspace_bytes = up(digits) + up(rot) + up(acc)      -- what cntt_native_bootstrap_batch needs, in this order
 *   cntt_native_blind_rotate_batch needs `digits` bytes (so the figure above always suffices).
 * A workspace must be 16-byte aligned and lives where the other buffers live; on the host path (CNTT_MEM_HOST) it is checked and
 * then not used.  workspace == NULL on the device path: the call makes one stream-ordered allocation (hipMallocAsync) for its
 * whole run -- never one per iteration.  With a caller workspace the Plan32 kinds at 32 <= n <= 4096 make no allocation anywhere
 * in the call, which may then be captured into a hipGraph (a linear chain of kernels, no parallel branches).  Elsewhere (other
 * sizes, the Plan52 kinds, the testing switch "native_ext" = 0) cntt_native_external_product_batch keeps allocating its own
 * stream-ordered scratch in every iteration, as it does when called on its own.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are
 * refused before any device call.  batch == 0 does nothing.  where / stream as every other _batch call: CNTT_MEM_HOST copies in,
 * runs the device path, copies out and synchronises. */
#ifndef CNTT_PBS_H
#define CNTT_PBS_H

#include "cntt_gadget.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ms(x) = (((x >> (w - logn - 2)) + 1) >> 1) mod 2n: round(x * 2n / 2^w) with ties up; a result of 2n wraps to 0.
 *   rot_t[i * batch + b] = ms(lwe[b][i])                 for i < L
 *   rot_t[L * batch + b] = (2n - ms(lwe[b][L])) mod 2n   (the body, negated)
 * lwe: batch x (L + 1) words; rot_t: (L + 1) x batch uint32.  The output is transposed on purpose: row i is the contiguous `rot`
 * array that iteration i hands to the decomposition.  lwe_dim == 0 writes the body row only.
 * CNTT_EINVAL for a NULL argument and for rot_t overlapping lwe. */
int cntt_native_lwe_modswitch_batch(const cntt_native_t *plan, uint32_t *rot_t, const void *lwe, size_t lwe_dim, size_t batch,
                                    cntt_mem_t where, void *stream);

/* Set-up:  acc[b][p] = X^(rot_t[L * batch + b]) * lut[p]  for all k + 1 polynomials (CNTT_SRC_ROTATE of cntt_gadget.h).
 *   lut is k + 1 polynomials shared by the batch, or batch * (k + 1) polynomials when lut_per_element != 0.  A trivial GLWE has
 *   zero mask polynomials; the call does not assume that.
 * Then for i = 0 .. L - 1:  acc[b] += ExtProd(bsk_i, X^(rot_t[i * batch + b]) acc[b] - acc[b]).
 *   The result has exactly the words of cntt_native_gadget_decompose_batch(CNTT_SRC_CMUX, npolys = k + 1) followed by
 *   cntt_native_external_product_batch(nterms = (k + 1) * levels, nout = k + 1, accumulate = 1) into the same buffer.
 * bsk_ntt: nprimes planes of L * (k + 1) * levels * (k + 1) residue polynomials.  Iteration i's slice starts at polynomial
 *   i * (k + 1) * levels * (k + 1).  Within the slice key[j][o] sits at j * (k + 1) + o with j = p * levels + (l - 1), as in
 *   cntt_gadget.h: row (p, l) encrypts s_i times the gadget factor 2^(w - base_log * l) on polynomial p.  This is what one
 *   cntt_native_fwd_batch (cntt_native_fwd_binary_batch for the binary kinds) over all key polynomials writes.
 * acc: batch x (k + 1) polynomials, written only.  Every kind and every size the two calls above accept.
 * acc may not overlap lut, rot_t or the workspace.  The "native_gadget" switch is not consulted: its fused kernel needs two buffers.
 * CNTT_EINVAL for: base_log == 0, levels == 0, base_log * levels > w, rot_t == NULL (the decomposition's cases);
 *   (k + 1) * levels > cntt_native_max_terms(plan); a NULL argument; a NULL key plane (lwe_dim > 0); the overlaps above; a non-NULL
 *   workspace that is misaligned or whose workspace_bytes is too small; on the host path an exponent that is not below 2n. */
int cntt_native_blind_rotate_batch(const cntt_native_t *plan, void *acc, const void *lut, int lut_per_element, const uint32_t *rot_t,
                                   const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                   size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* The LWE ciphertext of dimension k * n under the flattened GLWE key that encrypts coefficient h = index of the GLWE plaintext:
 *   lwe_out[b][p * n + j] = glwe[b][p][h - j]  for j <= h,  else  -glwe[b][p][h - j + n] mod 2^w        (p < k, j < n)
 *   lwe_out[b][k * n]     = glwe[b][k][h]                                                              (the body)
 * glwe: batch x (k + 1) polynomials; lwe_out: batch x (k * n + 1) words.
 * CNTT_EINVAL for index >= n, a NULL argument and lwe_out overlapping glwe. */
int cntt_native_sample_extract_batch(const cntt_native_t *plan, void *lwe_out, const void *glwe, size_t glwe_dim, size_t index,
                                     size_t batch, cntt_mem_t where, void *stream);

/* cntt_native_lwe_modswitch_batch, cntt_native_blind_rotate_batch and cntt_native_sample_extract_batch with index = 0 in one call:
 * lwe_in is batch x (L + 1) words, lwe_out batch x (k * n + 1) words; rot_t and the accumulator live in the workspace.
 * CNTT_EINVAL for the cases of the three calls, and for lwe_out overlapping lwe_in, lut or the workspace. */
int cntt_native_bootstrap_batch(const cntt_native_t *plan, void *lwe_out, const void *lwe_in, const void *lut, int lut_per_element,
                                const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* up(digits) + up(rot) + up(acc) of the formula above; 0 for a NULL plan */
size_t cntt_native_pbs_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PBS_H */
