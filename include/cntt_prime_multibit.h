/* The MULTI-BIT programmable bootstrap with a prime ciphertext modulus on the prime32 / prime64 plans: the LWE mask is taken in groups of
 * g = `grouping` words (1 ... 4), and one group is absorbed by ONE external product against a key bundled from 2^g GGSW ciphertexts,
 * where the classic loop of cntt_prime_pbs.h runs g CMux iterations one after the other.  L / g rounds of
 * (k + 1) * levels + (k + 1) transforms each instead of L; the extra work is pointwise.  No counterpart in the reference; the
 * convention below is this library's own, fixed to the last bit so that an integrator can generate matching keys.  Bit-compatibility
 * with the multi-bit key layout of tfhe-rs is NOT claimed.  No key or noise generation.  Include this file on its own (it is not part
 * of cntt.h or cntt_ext.h).  Plain C11.
 *
 * Symbols, digits, term order, modulus switch and data layouts: cntt_prime_pbs.h, plus g = grouping, G = L / g groups,
 * J = (k + 1) * levels.
 *
 * One group step.  For group r and batch element b let a_i = rot_t[(r g + i) * batch + b] for i < g, and for a pattern t in [0, 2^g)
 *     e_t = sum over the set bits i of t of a_i   mod 2n            (bit i of t, least significant first, belongs to mask word r g + i)
 * Then
 *     acc[b] <- sum_t X^(e_t) * ExtProd(BSK[r][t], acc[b])
 * with ExtProd the external product of the CNTT_SRC_PLAIN digits of acc[b]: no rotation and no CMux difference, the rotation lives in
 * the bundle.  The bundle sum_t X^(e_t) BSK[r][t] is never formed: X^e is a pointwise factor in the NTT domain,
 *     fwd(X^e)[c] = psi^(e (2 bitrev_logn(c) + 1)),   psi = the plan's primitive 2n-th root (cntt_plan_info_t.root), psi^n = -1
 * so per output polynomial o the step is  inv( sum_t fwd(X^(e_t)) . sum_j fwd(d_j(acc[b])) . K[r][t][j][o] ).
 *
 * Key.  bsk_mb is ONE array of G * 2^g * J * (k + 1) NTT-domain polynomials.  Group r, pattern t starts at polynomial
 * (r * 2^g + t) * J * (k + 1); inside, the layout is that of one iteration's slice of bsk_ntt (cntt_prime_pbs.h): key[j][o] at
 * j * (k + 1) + o, j = q * levels + (l - 1), holding n^-1 * fwd(key polynomial) (cntt_prime*_fwd_batch, then
 * cntt_prime*_normalize_batch).  Key (r, t) is the GGSW ciphertext of
 *     prod_{i in t} s_{r g + i} * prod_{i not in t} (1 - s_{r g + i})
 * i.e. row (q, l) encrypts that bit times the gadget factor 2^(W - base_log * l) mod p on polynomial q.  Exactly one pattern of a group
 * is 1, so with noiseless keys the step multiplies the accumulator by X^(sum_i a_i s_{r g + i}) up to the decomposition's rounding.
 * grouping = 1 is valid: two GGSW ciphertexts per mask word, of 1 - s and of s.
 *
 * Exactness.  Every call here is exact integer arithmetic mod p for EVERY prime the plans accept: the pointwise products are Montgomery
 * products, which are exact for every odd modulus, and not the reference's wrapping Barrett product.  So for the primes of the
 * reference's strict range (2^62 <= p < 2^63, 2^30 <= p < 2^31), for which cntt_prime*_external_product_batch equals the reference and
 * not always the true product (cntt_prime_pbs.h, "Exactness"), cntt_prime*_multibit_accumulate_batch still equals the big-integer
 * value.  The transforms are exact for every prime.
 *
 * Workspace.  The formula of cntt_prime*_pbs_workspace_bytes: up(digits) + up(rot) + up(acc) for the bootstrap, `digits` bytes for the
 * blind rotation; 16-byte aligned.  With a caller workspace the calls make no allocation and no copy at any ntt_size (after the plan's
 * first multi-bit call on the device: "First call" below), so they can be captured into a hipGraph: a linear chain of kernels.  workspace == NULL: one
 * stream-ordered allocation for the whole call.
 *
 * First call.  The first multi-bit call of a plan on a device -- any of the three calls below, cntt_prime*_multibit_accumulate_batch
 * included -- builds the plan's table of n powers of psi there: a synchronous allocation and copy, as the first transform of a plan
 * builds its twiddle tables.  That call must NOT be made inside a stream capture (it would invalidate the capture): make one eager
 * call per plan and device first.  Plans that never make a multi-bit call never build the table.
 *
 * Sizes.  n >= 16 on 64-bit words.  The 32-bit plans start at n = 32 (cntt_prime32_plan_new), so the kernel's n = 16 path on 32-bit
 * words -- one 16-byte vector per four coefficients, four vectors per polynomial -- cannot be reached through this interface.
 *
 * Speed (profiles/r17_prime_multibit.txt, tools/prime_multibit_bench.py: one MI355X, one process; p = 4611686018427322369, k = 1,
 * L = 720, n = 1024 and 2048, (base_log, levels) = (22, 1) and (11, 2)).  At batch 1, 16 and 256 every grouping beats
 * cntt_prime64_bootstrap_batch, g = 3 by the most: 2.2 to 4.3 times.  At batch 4096 the multi-bit call is SLOWER in three of the four
 * shapes (g = 2: 0.89 to 0.98 of the classic call's speed; g = 4: 0.65 to 0.81) and 5 % faster in one (n = 2048, (22, 1), g = 2): there
 * the pointwise kernel is 70 to 90 % of a group step.  There is no dispatch between the two calls: they take different keys.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are refused
 * before any device call.  batch == 0 does nothing.  where / stream as every other _batch call. */
#ifndef CNTT_PRIME_MULTIBIT_H
#define CNTT_PRIME_MULTIBIT_H

#include "cntt_prime_pbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups of the accumulate kernel for `vectors` 16-byte vectors of output (256 threads each; the kernel walks further vectors in a
 * grid-stride loop).  For tests and tools. */
unsigned cntt_prime_multibit_grid(size_t vectors);

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* The pointwise step alone, in the NTT domain:
 *   out_ntt[b][o][c] = sum_{t < 2^g} fwd(X^(e_t(b)))[c] * ( sum_{j < nterms} terms_ntt[b][j][c] * key_group[t][j][o][c] )  mod p
 * canonical, with e_t(b) formed from rot_rows[i * batch + b], i < g, as above.  terms_ntt: batch x nterms polynomials; key_group:
 * 2^g x nterms x nout polynomials; rot_rows: g x batch uint32; out_ntt: batch x nout polynomials, written only; it may not overlap an
 * input.  nterms == 0 writes zeros; nout == 0 does nothing.  Not inside a stream capture when it is the plan's first multi-bit call on
 * the device ("First call" above).
 * CNTT_EINVAL for grouping outside 1 ... 4, a NULL argument, a misaligned operand, out_ntt overlapping an input, and on the host path an
 * exponent that is not below 2n (the device path takes it mod 2n). */
int cntt_prime64_multibit_accumulate_batch(const cntt_plan64_t *plan, uint64_t *out_ntt, const uint64_t *terms_ntt,
                                           const uint32_t *rot_rows, const uint64_t *key_group, size_t nterms, size_t nout,
                                           unsigned grouping, size_t batch, cntt_mem_t where, void *stream);

/* Set-up as cntt_prime64_blind_rotate_batch: acc[b][q] = X^(rot_t[L * batch + b]) * lut[q].  Then the G group steps, each with exactly
 * the words of cntt_prime64_gadget_decompose_batch(CNTT_SRC_PLAIN, npolys = k + 1), cntt_prime64_fwd_batch over the digits,
 * cntt_prime64_multibit_accumulate_batch(nterms = J, nout = k + 1) and cntt_prime64_inv_batch.  lwe_dim == 0 writes the rotated table only.
 * Not inside a stream capture when it is the plan's first multi-bit call on the device ("First call" above).
 * acc: batch x (k + 1) polynomials, written only; it may not overlap lut, rot_t, bsk_mb or the workspace.
 * CNTT_EINVAL for: the decomposition's cases; grouping outside 1 ... 4; lwe_dim not a multiple of grouping; a NULL argument (bsk_mb only
 *   when lwe_dim > 0); the overlaps above; a non-NULL workspace that is misaligned or too small; on the host path an exponent that is
 *   not below 2n. */
int cntt_prime64_multibit_blind_rotate_batch(const cntt_plan64_t *plan, uint64_t *acc, const uint64_t *lut, int lut_per_element,
                                             const uint32_t *rot_t, const uint64_t *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                             unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                             size_t workspace_bytes, cntt_mem_t where, void *stream);

/* cntt_prime64_lwe_modswitch_batch, cntt_prime64_multibit_blind_rotate_batch and cntt_prime64_sample_extract_batch with index = 0 in one
 * call: lwe_in is batch x (L + 1) words, lwe_out batch x (k * n + 1) words; rot_t and the accumulator live in the workspace.
 * Not inside a stream capture when it is the plan's first multi-bit call on the device ("First call" above).
 * CNTT_EINVAL for the cases of the three calls, and for lwe_out overlapping lwe_in, lut, bsk_mb or the workspace. */
int cntt_prime64_multibit_bootstrap_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                                          int lut_per_element, const uint64_t *bsk_mb, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                          unsigned levels, unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes,
                                          cntt_mem_t where, void *stream);

/* up(digits) + up(rot) + up(acc), today the figure of cntt_prime64_pbs_workspace_bytes; 0 for a NULL plan */
size_t cntt_prime64_multibit_pbs_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels,
                                                 unsigned grouping, size_t batch);

/* ---- prime32: the same four calls on 32-bit words -------------------------------------------------------------------------------- */
int cntt_prime32_multibit_accumulate_batch(const cntt_plan32_t *plan, uint32_t *out_ntt, const uint32_t *terms_ntt,
                                           const uint32_t *rot_rows, const uint32_t *key_group, size_t nterms, size_t nout,
                                           unsigned grouping, size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_multibit_blind_rotate_batch(const cntt_plan32_t *plan, uint32_t *acc, const uint32_t *lut, int lut_per_element,
                                             const uint32_t *rot_t, const uint32_t *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                             unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                             size_t workspace_bytes, cntt_mem_t where, void *stream);
int cntt_prime32_multibit_bootstrap_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *lwe_in, const uint32_t *lut,
                                          int lut_per_element, const uint32_t *bsk_mb, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                          unsigned levels, unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes,
                                          cntt_mem_t where, void *stream);
size_t cntt_prime32_multibit_pbs_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels,
                                                 unsigned grouping, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_MULTIBIT_H */
