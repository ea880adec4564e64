/* Part of cntt_ext.h (which includes this file; include that one): the LWE keyswitch of the native / native_binary plans on the
 * device, and the keyswitch followed by the programmable bootstrap of cntt_pbs.h in one call -- the step that takes the output of
 * one bootstrap (dimension k * n, under the flattened GLWE key) back to the dimension the next one takes, so that table look-ups
 * chain without leaving the device.  No counterpart in the reference; the convention below is this library's own, fixed to the
 * last bit so that an integrator can generate matching keys.  No key or noise generation: the caller brings the keys.  Plain C11.
 *
 * Symbols: w = word width of the plan's kind (32, 64, 128) -- the only thing the keyswitch itself takes from the plan; ntt_size plays
 * no part in it.  Lin = lwe_dim_in, Lout = lwe_dim_out, B = 2^base_log.  An LWE ciphertext is its mask words with the body last, as
 * in cntt_pbs.h; a batch puts its elements back to back.
 *
 *   out[b][c] = (c == Lout ? in[b][Lin] : 0) - sum_{i < Lin} sum_{l = 1 .. levels} d_l(in[b][i]) * ksk[(i * levels + l - 1) * row_stride + c]
 *               mod 2^w,  for c <= Lout
 *
 * d_1 .. d_levels are the signed digits of cntt_gadget.h of the plain word in[b][i] (no rotation): the closest multiple of
 * 2^(w - base_log * levels), ties up, wrapping at the top; digits in [-B/2, B/2), d_1 most significant, the carry out of level 1
 * dropped.  The body word in[b][Lin] is not decomposed.
 *
 * Key layout.  ksk is Lin * levels rows of w-bit words.  Row i * levels + (l - 1) is an LWE encryption under the OUTPUT key of
 * s_in[i] * 2^(w - base_log * l), Lout mask words with the body last, and starts at word (i * levels + l - 1) * row_stride.
 * row_stride >= Lout + 1 is counted in words: row_stride == Lout + 1 is the packed form, a larger one lets the caller pad every row
 * (to 16 bytes, say); padding words are never read.  The buffer holds (Lin * levels - 1) * row_stride + Lout + 1 words or more.
 * With a noise-free key, s = w - base_log * levels and r_i the rounded (base_log * levels)-bit number of cntt_gadget.h, the phase of
 * the output under the output key is  in[b][Lin] - sum_i s_in[i] * r_i * 2^s  mod 2^w.
 *
 * Valid: 1 <= base_log <= 31 (the kernel keeps a digit in one signed 32-bit register), levels >= 1, base_log * levels <= w.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are refused
 * before any device call.  batch == 0 does nothing.  where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the
 * device path, copies out and synchronises. */
#ifndef CNTT_KEYSWITCH_H
#define CNTT_KEYSWITCH_H

#include "cntt_pbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lwe_in: batch x (Lin + 1) words; lwe_out: batch x (Lout + 1) words; ksk as above.  Every kind (the Plan52 kinds too: only w counts).
 * Lin == 0 copies the body and zeroes the mask (ksk may then be NULL); Lout == 0 is valid (the body only).
 * CNTT_EINVAL for base_log == 0, levels == 0, base_log * levels > w, base_log > 31, row_stride < Lout + 1, a NULL argument, and
 * lwe_out overlapping lwe_in or ksk (byte ranges). */
int cntt_native_keyswitch_batch(const cntt_native_t *plan, void *lwe_out, const void *lwe_in, const void *ksk, size_t lwe_dim_in,
                                size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels, size_t batch, cntt_mem_t where,
                                void *stream);

/* cntt_native_keyswitch_batch from dimension k * n to L = lwe_dim (digits ks_base_log, ks_levels; ksk has k * n * ks_levels rows of
 * row_stride >= L + 1 words), then cntt_native_bootstrap_batch on its output with the remaining arguments: exactly the words of the
 * two calls made one after the other.  lwe_in and lwe_out are both batch x (k * n + 1) words, so the call chains with itself; the
 * batch x (L + 1) ciphertexts in between live in the workspace.
 * Workspace, with up(x) = x rounded up to a multiple of 256 and wb = w / 8:
 *   cntt_native_ks_pbs_workspace_bytes = cntt_native_pbs_workspace_bytes(plan, L, k, levels, batch) + up(batch * (L + 1) * wb)
 *   -- the bootstrap's part first, the keyswitched ciphertexts behind it.
 * The rules are those of cntt_pbs.h: 16-byte aligned, living where the other buffers live; NULL on the device path is one
 * stream-ordered allocation for the whole call.  With a caller workspace the Plan32 kinds at 32 <= n <= 4096 make no allocation
 * anywhere in the call, which may then be captured into a hipGraph (a linear chain of kernels: the keyswitch is one more).
 * CNTT_EINVAL for the cases of the two calls (the keyswitch's digit arguments are named ks_base_log and ks_levels), for a non-NULL
 * workspace that is misaligned or too small, for lwe_out overlapping lwe_in, ksk, lut or the workspace, and for lwe_in, ksk or lut
 * overlapping the workspace. */
int cntt_native_keyswitch_bootstrap_batch(const cntt_native_t *plan, void *lwe_out, const void *lwe_in, const void *ksk, size_t row_stride,
                                          unsigned ks_base_log, unsigned ks_levels, const void *lut, int lut_per_element,
                                          const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                          size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);

/* the formula above; levels_bsk = the bootstrap's `levels`; 0 for a NULL plan */
size_t cntt_native_ks_pbs_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_KEYSWITCH_H */
