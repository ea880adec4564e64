/* The TFHE programmable bootstrap with a PRIME ciphertext modulus on the prime32 / prime64 plans: rotation, CMux difference and signed
 * gadget decomposition mod p, the modulus switch Z_p -> Z_2n, accumulator set-up, the blind rotation loop in place and sample
 * extraction -- the loop that the reference's caller (the NTT backend of tfhe-rs, classically with p = 2^64 - 2^32 + 1) writes around
 * the transforms.  One transform per polynomial: no residue split, no CRT.  The loop runs the decomposition below (CNTT_SRC_CMUX) and
 * cntt_prime*_external_product_batch (accumulate = 1) once per LWE mask word, into ONE accumulator and ONE digit scratch.  No
 * counterpart in the reference (concrete-ntt has no decomposer): the convention below is this library's own, fixed to the last bit so
 * that an integrator can generate matching keys.  Bit-compatibility with the non-native decomposer of tfhe-rs is NOT claimed.  No key
 * or noise generation: the caller brings the keys.  Include this file on its own (it is not part of cntt_ext.h).  Plain C11.
 *
 * Symbols: T = the plan's word (uint32_t / uint64_t), p = the modulus, n = ntt_size = 2^logn, W = the bit length of p
 * (2^(W-1) < p < 2^W), B = 2^base_log, k = glwe_dim, L = lwe_dim.  Valid: base_log >= 1, levels >= 1, base_log * levels <= W.
 * Every input word is canonical (< p).  Words >= p are not rejected and not reduced: the call completes without a fault and the
 * affected outputs are unspecified.
 *
 * Source polynomial g of an input polynomial f (n words) and an exponent a < 2n (one per batch element, rot[b], shared by the
 * element's npolys polynomials; rot lives where the polynomials live; a >= 2n is CNTT_EINVAL on the host path, the device path
 * takes a mod 2n): cntt_src_mode_t exactly as in cntt_gadget.h, with every negation and difference taken MOD p
 * (-x = p - x for x != 0, and 0 stays 0):
 *   CNTT_SRC_PLAIN   g = f                       (rot may be NULL and is not read)
 *   CNTT_SRC_ROTATE  g = X^a f  in Z_p[X]/(X^n + 1): for a < n, g[i] = f[i - a] if i >= a else -f[i - a + n]; for a >= n the
 *                    negation of the result for a - n
 *   CNTT_SRC_CMUX    g = X^a f - f  mod p
 *
 * Digits of a word x:
 *   balanced lift   x' = x if x <= (p - 1) / 2, else x - p                      (a signed integer, |x'| <= (p - 1) / 2)
 *   s = W - base_log * levels;   r = floor((x' + 2^(s-1)) / 2^s), floor towards minus infinity;  r = x' when s = 0
 *   from the low level up, for the levels `levels` ... 2:  d = state mod B taken in [0, B);  state = (state - d) / B;
 *                                                          if d >= B/2 then d -= B and state += 1
 *   the top digit d_1 is the remaining state, UNMASKED: it lies in [-B/2, B/2], both ends reachable.
 * Then sum_l d_l 2^(W - base_log * l) = r 2^s as integers and |r 2^s - x'| <= 2^(s-1) (= 0 when s = 0), so the reconstruction holds
 * mod p for every prime: nothing is lost at the top, as it would be if the 2^W wrap of the native convention were borrowed.
 * Digits are stored canonically mod p (d >= 0 -> d, d < 0 -> p + d), which is what cntt_prime*_external_product_batch expects of
 * `terms`.
 *
 * Term order: term j = q * levels + (l - 1) is level l of polynomial q, as in cntt_gadget.h: key row j belongs to the gadget factor
 * 2^(W - base_log * l) mod p of polynomial q.
 *
 * Modulus switch: ms(x) = floor((2 x 2n + p) / (2 p)) mod 2n = round(x 2n / p); p is odd, so there are no ties; a result of 2n wraps
 * to 0.  Exact (no floating point).  Needs logn <= 29.
 *
 * Data layouts (as cntt_pbs.h): an LWE ciphertext is L + 1 words with the body last; a GLWE ciphertext is k + 1 polynomials with the
 * body last; a batch puts its elements back to back.
 *
 * Bootstrapping key: bsk_ntt is ONE array of L * (k + 1) * levels * (k + 1) NTT-domain polynomials.  Iteration i's slice starts at
 * polynomial i * (k + 1) * levels * (k + 1); within the slice key[j][o] sits at j * (k + 1) + o with j = q * levels + (l - 1): row
 * (q, l) encrypts s_i times the gadget factor 2^(W - base_log * l) mod p on polynomial q.  cntt_prime*_external_product_batch returns
 * the UNNORMALISED inverse transform, which carries the factor n, so the key must hold n^-1 * fwd(key polynomial): what
 * cntt_prime*_fwd_batch followed by cntt_prime*_normalize_batch over all key polynomials writes.
 *
 * Workspace.  With wb = sizeof(T) and up(x) = x rounded up to a multiple of 256:
 *   digits = batch * (k + 1) * levels * n * wb        (the terms of one iteration)
 *   rot    = (L + 1) * batch * 4                      (rot_t)
 *   acc    = batch * (k + 1) * n * wb                 (the accumulator)
 *   cntt_prime*_pbs_workspace_bytes = up(digits) + up(rot) + up(acc)      -- what cntt_prime*_bootstrap_batch needs, in this order
 *   cntt_prime*_blind_rotate_batch needs `digits` bytes (so the figure above always suffices).
 * A workspace must be 16-byte aligned and lives where the other buffers live; on the host path (CNTT_MEM_HOST) it is checked and
 * then not used.  workspace == NULL on the device path: the call makes one stream-ordered allocation (hipMallocAsync) for its
 * whole run -- never one per iteration.  With a caller workspace the shapes that the fused mul_accumulate chain serves (the
 * transform lives in one wavefront group: n <= 2048 for 64-bit words, 4096 for 32-bit words; k + 1 <= 4) make no allocation anywhere
 * in the call, which may then be captured into a hipGraph (a linear chain of kernels, no parallel branches).  Elsewhere
 * cntt_prime*_external_product_batch keeps allocating its own stream-ordered scratch in every iteration, as it does when called on
 * its own.
 *
 * There is no bound on the number of terms (a prime plan's accumulation is modular; cntt_native_max_terms has no counterpart here).
 *
 * Exactness.  Every call here is exact integer arithmetic mod p, and the blind rotation has exactly the words of the public
 * per-iteration calls for every prime the plans accept.  For the primes of the reference's strict range (2^62 <= p < 2^63 on 64-bit
 * words, 2^30 <= p < 2^31 on 32-bit words) cntt_prime*_mul_accumulate reproduces the reference's wrapping Barrett reduction
 * (INTEGRATION.md section 6), which is not always the exact product mod p -- so for those primes the external product, and with it
 * the blind rotation, equals the reference's composition and NOT necessarily the big-integer negacyclic product; a caller who needs
 * exact products stays outside that range, as with the CPU crate.  Decomposition, modulus switch and extraction are exact there too.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are
 * refused before any device call.  batch == 0 does nothing.  where / stream as every other _batch call: CNTT_MEM_HOST copies in,
 * runs the device path, copies out and synchronises. */
#ifndef CNTT_PRIME_PBS_H
#define CNTT_PRIME_PBS_H

#include "cntt_gadget.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* terms[b][q * levels + l - 1] = level l of the digits of src_mode(polys[b][q], rot[b]);  batch x npolys polynomials in,
 * batch x npolys * levels out.  Every size.  CNTT_EINVAL (terms untouched) for base_log == 0, levels == 0, base_log * levels > W, an
 * unknown mode, rot == NULL with a mode that reads it, or terms overlapping polys (byte ranges).  batch == 0 or npolys == 0 does
 * nothing. */
int cntt_prime64_gadget_decompose_batch(const cntt_plan64_t *plan, uint64_t *terms, const uint64_t *polys, const uint32_t *rot,
                                        size_t npolys, unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t batch,
                                        cntt_mem_t where, void *stream);

/*   rot_t[i * batch + b] = ms(lwe[b][i])                 for i < L
 *   rot_t[L * batch + b] = (2n - ms(lwe[b][L])) mod 2n   (the body, negated)
 * lwe: batch x (L + 1) words; rot_t: (L + 1) x batch uint32.  The output is transposed on purpose: row i is the contiguous `rot`
 * array that iteration i hands to the decomposition.  lwe_dim == 0 writes the body row only.
 * CNTT_EINVAL for a NULL argument and for rot_t overlapping lwe. */
int cntt_prime64_lwe_modswitch_batch(const cntt_plan64_t *plan, uint32_t *rot_t, const uint64_t *lwe, size_t lwe_dim, size_t batch,
                                     cntt_mem_t where, void *stream);

/* Set-up:  acc[b][q] = X^(rot_t[L * batch + b]) * lut[q]  for all k + 1 polynomials (CNTT_SRC_ROTATE).
 *   lut is k + 1 polynomials shared by the batch, or batch * (k + 1) polynomials when lut_per_element != 0.  A trivial GLWE has
 *   zero mask polynomials; the call does not assume that.
 * Then for i = 0 .. L - 1:  acc[b] += ExtProd(bsk_i, X^(rot_t[i * batch + b]) acc[b] - acc[b]).
 *   The result has exactly the words of cntt_prime64_gadget_decompose_batch(CNTT_SRC_CMUX, npolys = k + 1) followed by
 *   cntt_prime64_external_product_batch(nterms = (k + 1) * levels, nout = k + 1, accumulate = 1) into the same buffer.
 * acc: batch x (k + 1) polynomials, written only.  acc may not overlap lut, rot_t or the workspace.
 * CNTT_EINVAL for: the decomposition's cases; rot_t == NULL; a NULL argument; bsk_ntt == NULL (lwe_dim > 0); the overlaps above; a
 *   non-NULL workspace that is misaligned or whose workspace_bytes is too small; on the host path an exponent that is not below 2n. */
int cntt_prime64_blind_rotate_batch(const cntt_plan64_t *plan, uint64_t *acc, const uint64_t *lut, int lut_per_element,
                                    const uint32_t *rot_t, const uint64_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                    unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                    void *stream);

/* The LWE ciphertext of dimension k * n under the flattened GLWE key that encrypts coefficient h = index of the GLWE plaintext:
 *   lwe_out[b][q * n + j] = glwe[b][q][h - j]  for j <= h,  else  -glwe[b][q][h - j + n] mod p        (q < k, j < n)
 *   lwe_out[b][k * n]     = glwe[b][k][h]                                                              (the body)
 * glwe: batch x (k + 1) polynomials; lwe_out: batch x (k * n + 1) words.
 * CNTT_EINVAL for index >= n, a NULL argument and lwe_out overlapping glwe. */
int cntt_prime64_sample_extract_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *glwe, size_t glwe_dim, size_t index,
                                      size_t batch, cntt_mem_t where, void *stream);

/* cntt_prime64_lwe_modswitch_batch, cntt_prime64_blind_rotate_batch and cntt_prime64_sample_extract_batch with index = 0 in one call:
 * lwe_in is batch x (L + 1) words, lwe_out batch x (k * n + 1) words; rot_t and the accumulator live in the workspace.
 * CNTT_EINVAL for the cases of the three calls, and for lwe_out overlapping lwe_in, lut or the workspace. */
int cntt_prime64_bootstrap_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                                 int lut_per_element, const uint64_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                 unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* up(digits) + up(rot) + up(acc) of the formula above; 0 for a NULL plan */
size_t cntt_prime64_pbs_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch);

/* ---- prime32: the same six calls on 32-bit words --------------------------------------------------------------------------------- */
int cntt_prime32_gadget_decompose_batch(const cntt_plan32_t *plan, uint32_t *terms, const uint32_t *polys, const uint32_t *rot,
                                        size_t npolys, unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t batch,
                                        cntt_mem_t where, void *stream);
int cntt_prime32_lwe_modswitch_batch(const cntt_plan32_t *plan, uint32_t *rot_t, const uint32_t *lwe, size_t lwe_dim, size_t batch,
                                     cntt_mem_t where, void *stream);
int cntt_prime32_blind_rotate_batch(const cntt_plan32_t *plan, uint32_t *acc, const uint32_t *lut, int lut_per_element,
                                    const uint32_t *rot_t, const uint32_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                    unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                    void *stream);
int cntt_prime32_sample_extract_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *glwe, size_t glwe_dim, size_t index,
                                      size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_bootstrap_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *lwe_in, const uint32_t *lut,
                                 int lut_per_element, const uint32_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                 unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_pbs_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_PBS_H */
