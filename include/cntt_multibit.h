/* The MULTI-BIT programmable bootstrap on the native plans (ciphertext modulus 2^32 / 2^64 / 2^128): the LWE mask is taken in groups of
 * g = `grouping` words (1 ... 4), and one group is absorbed by ONE external product against a key bundled from 2^g GGSW ciphertexts,
 * where the classic loop of cntt_pbs.h runs g CMux iterations one after the other.  L / g rounds of (k + 1) * levels + (k + 1)
 * transforms per residue prime instead of L; the extra work is pointwise.  The counterpart mod p is cntt_prime_multibit.h.  No
 * counterpart in the reference; the convention below is this library's own, fixed to the last bit so that an integrator can generate
 * matching keys.  Bit-compatibility with the multi-bit key layout of tfhe-rs is NOT claimed.  No key or noise generation.  Include this
 * file on its own (it is not part of cntt.h or cntt_ext.h).  Plain C11.
 *
 * Symbols, digits, term order, modulus switch and data layouts: cntt_pbs.h and cntt_gadget.h, plus g = grouping, G = L / g groups,
 * J = (k + 1) * levels, w = the word width of the plan's kind, P_i the residue primes of the plan (cntt_native_nprimes of them).
 *
 * One group step.  For group r and batch element b let a_i = rot_t[(r g + i) * batch + b] for i < g, and for a pattern t in [0, 2^g)
 *     e_t = sum over the set bits i of t of a_i   mod 2n            (bit i of t, least significant first, belongs to mask word r g + i)
 * the rule of cntt_prime_multibit.h.  Then, per output polynomial o,
 *     acc[b][o] <- sum_{t < 2^g} X^(e_t) * sum_{j < J} d_j(acc[b]) (*) K[r][t][j][o]      mod 2^w
 * with d_j the CNTT_SRC_PLAIN digits of cntt_native_gadget_decompose_batch and (*) the negacyclic product: no rotation and no CMux
 * difference, the rotation lives in the bundle.  The bundle sum_t X^(e_t) K[r][t] is never formed: per residue prime X^e is a pointwise
 * factor in the NTT domain,
 *     fwd(X^e)[c] = psi_i^(e (2 bitrev_logn(c) + 1)),   psi_i = the primitive 2n-th root of sub-plan i (cntt_native_ntt32), psi_i^n = -1.
 *
 * Key.  bsk_mb is cntt_native_nprimes residue planes, each of G * 2^g * J * (k + 1) polynomials of 32-bit residues.  Group r, pattern t
 * starts at polynomial (r * 2^g + t) * J * (k + 1); inside, the layout is that of one iteration's slice of bsk_ntt (cntt_pbs.h):
 * key[j][o] at j * (k + 1) + o, j = q * levels + (l - 1).  The words are exactly what cntt_native_fwd_batch writes for the key
 * polynomials (cntt_native_fwd_binary_batch for the binary kinds): canonical, NOT normalised.  Key (r, t) is the GGSW ciphertext of
 *     prod_{i in t} s_{r g + i} * prod_{i not in t} (1 - s_{r g + i})
 * i.e. row (q, l) encrypts that bit times the gadget factor 2^(w - base_log * l) on polynomial q.  Exactly one pattern of a group is 1,
 * so with noiseless keys the step multiplies the accumulator by X^(sum_i a_i s_{r g + i}) up to the decomposition's rounding.
 * grouping = 1 is valid: two GGSW ciphertexts per mask word, of 1 - s and of s.
 *
 * Exactness.  A product with a monomial is a signed permutation of the coefficients, so the group step is an integer sum of 2^g * J
 * negacyclic products, and the calls are exact -- the words of the expression above, to the last bit -- while
 *     2^g * (k + 1) * levels <= cntt_native_max_terms(plan)
 * (cntt_ext.h).  Beyond that cntt_native_multibit_blind_rotate_batch and cntt_native_multibit_bootstrap_batch return CNTT_EINVAL before
 * any device call, the message giving both numbers.  native64 at n = 1024: cntt_native_max_terms = 1964, so every g <= 4 with J <= 122.
 * cntt_native_multibit_accumulate_batch is arithmetic mod P_i and exact for every nterms.
 *
 * Scope.  The six Plan32 kinds (native32 / 64 / 128 and the three binary kinds) at every n >= 32 their sub-plans transform.  The Plan52
 * kinds get CNTT_EINVAL naming the kind: their key residues are 50-bit words, and the kernel's sums are derived for primes below 2^30.
 *
 * Workspace.  With up(x) = x rounded up to 256 bytes, word = cntt_native_word_bytes, P = batch * (k + 1) * n polynomial words:
 *     digits  = P * levels * word            the CNTT_SRC_PLAIN digits
 *     terms   = nprimes * P * levels * 4     their residue planes, transformed in place
 *     outputs = nprimes * P * 4              the step's residue planes
 *     rot     = (L + 1) * batch * 4          rot_t
 *     acc     = P * word                     the accumulator
 * cntt_native_multibit_pbs_workspace_bytes = up(digits) + up(terms) + up(outputs) + up(rot) + up(acc), what the bootstrap needs; the
 * blind rotation uses the first three parts and accepts any workspace of up(digits) + up(terms) + up(outputs) bytes or more.  16-byte
 * aligned.  With a caller workspace the calls make no allocation and no copy at any ntt_size (after the plan's first multi-bit call on
 * the device: "First call" below), so they can be captured into a hipGraph: a linear chain of kernels.  workspace == NULL: one
 * stream-ordered allocation for the whole call.
 *
 * First call.  The first multi-bit call of a plan on a device -- any of the three calls below, cntt_native_multibit_accumulate_batch
 * included -- builds the plan's tables of n powers of psi_i per prime there: a synchronous allocation and copy, as the first transform
 * of a plan builds its twiddle tables.  That call must NOT be made inside a stream capture (it would invalidate the capture): make one
 * eager call per plan and device first.  Plans that never make a multi-bit call never build the tables.
 *
 * Speed (profiles/r18_native_multibit.txt, tools/native_multibit_bench.py: one MI355X, one process; native64 Plan32, k = 1, L = 720,
 * n = 1024 and 2048, (base_log, levels) = (22, 1) and (11, 2)).  A group step is 2 * nprimes + 4 launches (digits, split, nprimes
 * forward transforms, one pointwise launch for all planes, nprimes inverse transforms, CRT) against 2 per mask word of the classic
 * call's fused loop.  At batch 1 and 16 every g >= 2 beats cntt_native_bootstrap_batch, g = 4 by the most: 2.4 to 3.3 times.  At batch
 * 256 g = 3 is best, 1.3 to 1.8 times faster.  At batch 4096 the multi-bit call is SLOWER at every grouping: 1.34 to 1.79 times slower
 * at its best g (2 or 3).  g = 1 is slower than the classic call in most shapes.  There is no dispatch between the two calls: they
 * take different keys.
 *
 * Errors.  Every error below returns CNTT_EINVAL with the outputs untouched and cntt_last_error naming the argument; all are refused
 * before any device call.  batch == 0 does nothing.  where / stream as every other _batch call. */
#ifndef CNTT_MULTIBIT_H
#define CNTT_MULTIBIT_H

#include "cntt_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups PER RESIDUE PLANE of the accumulate kernel for `vectors` 16-byte vectors of one plane's output (256 threads each; the
 * kernel walks further vectors in a grid-stride loop; the planes are the grid's second dimension).  For tests and tools. */
unsigned cntt_native_multibit_grid(size_t vectors);

/* The pointwise step alone, in the NTT domain, on every residue plane i of the plan:
 *   out_ntt[i][b][o][c] = n^-1 * sum_{t < 2^g} fwd_i(X^(e_t(b)))[c] * ( sum_{j < nterms} terms_ntt[i][b][j][c] * key_group[i][t][j][o][c] )  mod P_i
 * canonical, with e_t(b) formed from rot_rows[i * batch + b], i < g, as above.  The factor n^-1 is the one that takes the place of a
 * normalisation pass: cntt_native_inv_batch on out_ntt gives the coefficient-domain words mod 2^w of
 *   sum_t X^(e_t) sum_j terms[b][j] (*) key[t][j][o]
 * when terms_ntt and key_group are what cntt_native_fwd_batch writes for `terms` and `key` (and the sum is within the exact range).
 * out_ntt, terms_ntt, key_group: cntt_native_nprimes planes of batch x nout, batch x nterms and 2^g x nterms x nout polynomials of
 * 32-bit canonical residues; rot_rows: g x batch uint32.  out_ntt is written only; no plane of it may overlap an input or another plane
 * of it.  nterms == 0 writes zeros; nout == 0 does nothing.  Not inside a stream capture when it is the plan's first multi-bit call on
 * the device ("First call" above).
 * CNTT_EINVAL for a Plan52 kind, grouping outside 1 ... 4, a NULL argument or residue plane, a misaligned operand, an out_ntt plane
 * overlapping another operand, and on the host path an exponent that is not below 2n (the device path takes it mod 2n). */
int cntt_native_multibit_accumulate_batch(const cntt_native_t *plan, void *const *out_ntt, const void *const *terms_ntt,
                                          const uint32_t *rot_rows, const void *const *key_group, size_t nterms, size_t nout,
                                          unsigned grouping, size_t batch, cntt_mem_t where, void *stream);

/* Set-up as cntt_native_blind_rotate_batch: acc[b][q] = X^(rot_t[L * batch + b]) * lut[q].  Then the G group steps, each with exactly the
 * words of cntt_native_gadget_decompose_batch(CNTT_SRC_PLAIN, npolys = k + 1), cntt_native_fwd_batch over the digits,
 * cntt_native_multibit_accumulate_batch(nterms = J, nout = k + 1) and cntt_native_inv_batch.  lwe_dim == 0 writes the rotated table only.
 * Not inside a stream capture when it is the plan's first multi-bit call on the device ("First call" above).
 * acc: batch x (k + 1) polynomials, written only; it may not overlap lut, rot_t, bsk_mb or the workspace.
 * CNTT_EINVAL for: a Plan52 kind; the decomposition's cases; grouping outside 1 ... 4; lwe_dim not a multiple of grouping;
 *   2^g * (k + 1) * levels above cntt_native_max_terms; a NULL argument or residue plane (bsk_mb only when lwe_dim > 0); the overlaps
 *   above; a misaligned operand; a non-NULL workspace that is misaligned or too small; on the host path an exponent that is not below 2n. */
int cntt_native_multibit_blind_rotate_batch(const cntt_native_t *plan, void *acc, const void *lut, int lut_per_element,
                                            const uint32_t *rot_t, const void *const *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                            unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                            size_t workspace_bytes, cntt_mem_t where, void *stream);

/* cntt_native_lwe_modswitch_batch, cntt_native_multibit_blind_rotate_batch and cntt_native_sample_extract_batch with index = 0 in one
 * call: lwe_in is batch x (L + 1) words, lwe_out batch x (k * n + 1) words; rot_t and the accumulator live in the workspace.
 * Not inside a stream capture when it is the plan's first multi-bit call on the device ("First call" above).
 * CNTT_EINVAL for the cases of the three calls, and for lwe_out overlapping lwe_in, lut, bsk_mb or the workspace. */
int cntt_native_multibit_bootstrap_batch(const cntt_native_t *plan, void *lwe_out, const void *lwe_in, const void *lut,
                                         int lut_per_element, const void *const *bsk_mb, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                         unsigned levels, unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes,
                                         cntt_mem_t where, void *stream);

/* up(digits) + up(terms) + up(outputs) + up(rot) + up(acc) as defined above (`grouping` does not enter it today); 0 for a NULL plan, for
 * a Plan52 kind, and for sizes whose workspace would not fit 2^62 bytes (the two calls above refuse those with CNTT_EINVAL) */
size_t cntt_native_multibit_pbs_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned levels,
                                                unsigned grouping, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_MULTIBIT_H */
