/* The LWE keyswitch of the prime32 / prime64 plans on the device, and the keyswitch followed by the programmable bootstrap of
 * cntt_prime_pbs.h in one call -- the step that takes the output of one bootstrap (dimension k * n, under the flattened GLWE key) back
 * to the dimension the next one takes, so that table look-ups chain modulo a prime without leaving the device.  No counterpart in the
 * reference; the convention below is this library's own, fixed to the last bit so that an integrator can generate matching keys.  No
 * key or noise generation: the caller brings the keys.  Include this file on its own (it includes cntt_prime_pbs.h).  Plain C11.
 *
 * Symbols: T = the plan's word (uint32_t / uint64_t), p = the modulus -- the only thing the keyswitch itself takes from the plan;
 * ntt_size plays no part in it --, W = the bit length of p, Lin = lwe_dim_in, Lout = lwe_dim_out, B = 2^base_log.  An LWE ciphertext
 * is its mask words with the body last, as in cntt_prime_pbs.h; a batch puts its elements back to back.
 *
 *   out[b][c] = (c == Lout ? in[b][Lin] : 0) - sum_{i < Lin} sum_{l = 1 .. levels} d_l(in[b][i]) * ksk[(i * levels + l - 1) * row_stride + c]
 *               mod p,  for c <= Lout
 *
 * d_1 .. d_levels are the digits of cntt_prime_pbs.h of the plain word in[b][i] (no rotation): taken from the balanced lift x',
 * rounded to 2^(W - base_log * levels), d_1 most significant; the levels below the top lie in [-B/2, B/2), the top digit d_1 is
 * unmasked and lies in [-B/2, B/2].  The body word in[b][Lin] is not decomposed.  Every output word is canonical (< p).
 *
 * Key layout.  ksk is Lin * levels rows of words of type T.  Row i * levels + (l - 1) is an LWE encryption under the OUTPUT key of
 * s_in[i] * 2^(W - base_log * l) mod p, Lout mask words with the body last, and starts at word (i * levels + l - 1) * row_stride.
 * row_stride >= Lout + 1 is counted in words: row_stride == Lout + 1 is the packed form, a larger one lets the caller pad every row
 * (to 16 bytes, say); padding words are never read.  The buffer holds (Lin * levels - 1) * row_stride + Lout + 1 words or more.
 *
 * Phase.  With a noise-free key, s = W - base_log * levels and r_i the rounded number of cntt_prime_pbs.h
 * (r_i * 2^s = sum_l d_l 2^(W - base_log * l) as integers, |r_i * 2^s - lift(in[b][i])| <= 2^(s-1), = 0 when s = 0):
 *   out_body - <out_mask, s_out> = in_body - sum_i s_in[i] * r_i * 2^s  mod p.
 *
 * Exactness.  The call is exact integer arithmetic mod p for EVERY prime the plans accept, the reference's strict range
 * (2^62 <= p < 2^63 on 64-bit words, 2^30 <= p < 2^31 on 32-bit words) included: it does not go through the reference's wrapping
 * Barrett product, so the caveat of cntt_prime_pbs.h ("Exactness") does not apply to the keyswitch.  It does apply to the bootstrap
 * half of the combined call, which is cntt_prime*_bootstrap_batch word for word.
 *
 * Valid: 1 <= base_log <= 31 (the kernel keeps a digit, offset by B/2, in one 32-bit register), levels >= 1,
 * base_log * levels <= W, Lin * levels < 2^32.  Input or key words >= p are not rejected and not reduced: the call completes without
 * a fault and the affected outputs are unspecified.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are refused
 * before any device call.  batch == 0 does nothing.  where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the
 * device path, copies out and synchronises. */
#ifndef CNTT_PRIME_KEYSWITCH_H
#define CNTT_PRIME_KEYSWITCH_H

#include "cntt_prime_pbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* lwe_in: batch x (Lin + 1) words; lwe_out: batch x (Lout + 1) words; ksk as above.
 * Lin == 0 copies the body and zeroes the mask (ksk may then be NULL); Lout == 0 is valid (the body only).
 * CNTT_EINVAL for a NULL plan or argument, base_log == 0, levels == 0, base_log * levels > W, base_log > 31, Lin * levels >= 2^32,
 * row_stride < Lout + 1, and lwe_out overlapping lwe_in or ksk (byte ranges). */
int cntt_prime64_keyswitch_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *ksk,
                                 size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,
                                 size_t batch, cntt_mem_t where, void *stream);

/* cntt_prime64_keyswitch_batch from dimension k * n to L = lwe_dim (digits ks_base_log, ks_levels; ksk has k * n * ks_levels rows of
 * row_stride >= L + 1 words), then cntt_prime64_bootstrap_batch on its output with the remaining arguments: exactly the words of the
 * two calls made one after the other.  lwe_in and lwe_out are both batch x (k * n + 1) words, so the call chains with itself; the
 * batch x (L + 1) ciphertexts in between live in the workspace.
 * Workspace, with up(x) = x rounded up to a multiple of 256:
 *   cntt_prime64_ks_pbs_workspace_bytes = cntt_prime64_pbs_workspace_bytes(plan, L, k, levels, batch) + up(batch * (L + 1) * sizeof(T))
 *   -- the bootstrap's part first, the keyswitched ciphertexts behind it.
 * The rules are those of cntt_prime_pbs.h: 16-byte aligned, living where the other buffers live; NULL on the device path is one
 * stream-ordered allocation for the whole call.  With a caller workspace the shapes on which cntt_prime64_bootstrap_batch makes no
 * allocation make none anywhere in this call either, which may then be captured into a hipGraph (a linear chain of kernels: the
 * keyswitch is one more).
 * CNTT_EINVAL for the cases of the two calls (the keyswitch's digit arguments are named ks_base_log and ks_levels), for a non-NULL
 * workspace that is misaligned or too small, for lwe_out overlapping lwe_in, ksk, lut or the workspace, and for lwe_in, ksk or lut
 * overlapping the workspace. */
int cntt_prime64_keyswitch_bootstrap_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *ksk,
                                           size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const uint64_t *lut,
                                           int lut_per_element, const uint64_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                           unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                           cntt_mem_t where, void *stream);

/* the formula above; levels_bsk = the bootstrap's `levels`; 0 for a NULL plan */
size_t cntt_prime64_ks_pbs_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk, size_t batch);

/* ---- prime32: the same three calls on 32-bit words -------------------------------------------------------------------------------- */
int cntt_prime32_keyswitch_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *lwe_in, const uint32_t *ksk,
                                 size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,
                                 size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_keyswitch_bootstrap_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *lwe_in, const uint32_t *ksk,
                                           size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const uint32_t *lut,
                                           int lut_per_element, const uint32_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                           unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                           cntt_mem_t where, void *stream);
size_t cntt_prime32_ks_pbs_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_KEYSWITCH_H */
