/* The many-LUT programmable bootstrap on the prime32 / prime64 plans, and the circuit bootstrap that runs ONE blind rotation per input
 * bit instead of one per selector level: the PBSmanyLUT of Chillotti, Ligier, Orfila and Tap (Asiacrypt 2021).  The modulus switch clears
 * the low log_lut_count bits of every exponent, so that the rotated table keeps 2^log_lut_count neighbouring coefficients intact, and
 * one rotation evaluates up to 2^log_lut_count functions of the encrypted message, extracted at the indices 0, 1, ...  No counterpart
 * in the reference; the convention below is this library's own, fixed to the last bit.  No key or noise generation: the caller brings
 * the keys.  Include this file on its own (it includes cntt_prime_cbs.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_prime_pbs.h and cntt_prime_cbs.h: T = the plan's word, p = the modulus, W = the bit length of p,
 * n = ntt_size = 2^logn, k = glwe_dim, L = lwe_dim, Lin = k * n, R = (Lin + 1) * Lk, Lc = cbs_levels.  New: t = log_lut_count,
 * 0 <= t <= logn, and n' = n / 2^t.
 *
 * Coarse modulus switch.  ms_t(x) = 2^t * (floor((2 x 2n' + p) / (2 p)) mod 2n'): the ms of cntt_prime_pbs.h for the ring size n',
 * shifted left by t.  Exact (no floating point); p is odd, so there are no ties.  ms_0 = ms, word for word.
 *   rot_t[i * batch + b] = ms_t(lwe[b][i])                  for i < L
 *   rot_t[L * batch + b] = (2n - ms_t(lwe[b][L])) mod 2n    (the body, negated; still a multiple of 2^t)
 * the transposed layout of cntt_prime*_lwe_modswitch_batch.
 *
 * Interleaved table.  For an exponent a = 0 mod 2^t and h < 2^t, coefficient h of X^(-a) v is v[a + h] for a < n and -v[a + h - n]
 * for a >= n: a + h never straddles n, because a and n are multiples of 2^t.  Function h of the table therefore lives at the
 * coefficients v[m * 2^t + h], m < n': a table of n' boxes per function, the 2^t functions interleaved.
 *
 * Multi-index extraction.  lwe_out[b][h], h < count, is exactly cntt_prime*_sample_extract_batch(glwe[b], index = h):
 *   lwe_out[b][h][q * n + j] = glwe[b][q][h - j]  for j <= h,  else  -glwe[b][q][h - j + n] mod p        (q < k, j < n)
 *   lwe_out[b][h][k * n]     = glwe[b][k][h]
 * The layout is batch x count x (k * n + 1) words.
 *
 * The many-LUT bootstrap is the coarse modulus switch, cntt_prime*_blind_rotate_batch UNCHANGED and the multi-index extraction with
 * count = lut_count, 1 <= lut_count <= 2^t.  Its workspace is exactly cntt_prime*_pbs_workspace_bytes (digits | rot_t | acc): there is
 * no new size function.  At t = 0, lut_count = 1 it equals cntt_prime*_bootstrap_batch word for word.  It allocates and may be
 * captured into a hipGraph under the conditions of cntt_prime*_bootstrap_batch.
 *
 * The one-rotation circuit bootstrap.  Arguments, input, output, keys and step 3 are those of cntt_prime*_circuit_bootstrap_batch
 * (cntt_prime_cbs.h), with G_l = 2^(W - cbs_base_log * l), H_l = G_l * 2^-1 mod p and Q4 = floor((p + 2) / 4):
 * 1. lwe'[b] = lwe_in[b] with Q4 added to the body mod p.
 * 2. ONE table shared by the batch (lut_per_element = 0): the mask polynomials zero, the body polynomial
 *      v[m * 2^t + h] = p - H_(h+1)  for h < Lc,   0  for Lc <= h < 2^t        (m < n').
 *    u[b][l] = the many-LUT bootstrap of lwe'[b] with this table and the PBS gadget, extracted at the index l - 1, and then H_l added
 *    to its body word mod p.  The blind rotation runs over batch elements, not over E = batch * Lc.
 *    With noise-free keys (and pbs_base_log * pbs_levels = W, so that nothing is rounded) the phase of u[b][l] is exactly 0 for the
 *    bit 0 and G_l for the bit 1:
 *      the accumulator is X^(-a) v with a = the coarsely switched phase of lwe' in Z_2n, a multiple of 2^t; its coefficient l - 1 is
 *      v[a + l - 1] = -H_l for a < n and -v[a + l - 1 - n] = +H_l for a >= n.  Q4 moves the bit 0 to a = n / 2 and the bit 1 to
 *      a = 3 n / 2, both on the coarse grid because 2^t <= n / 2, so the body is -H_l + H_l = 0 or H_l + H_l = G_l.
 *    The margin is n / 2^(t + 1) steps of the coarse switch (n / 2 exponents, as before, but a step is now 2^t exponents).  Every
 *    switched word that enters the exponent -- the body and the mask words whose key bit is 1, L + 1 at the most -- is off by less than
 *    half a step, and an input noise e, with the rounding of Q4 and of (p + 1) / 2, moves the phase by (|e| + 1) * 2n' / p steps: the
 *    exponent is a whole number of steps off by less than D = (L + 1) / 2 + (|e| + 1) * 2n' / p, and the bit is read right when
 *    D <= n / 2^(t + 1).
 * 3. Unchanged: the int32 digits of all Lin + 1 words of u[b][l] for (ks_base_log, Lk), element e = b * Lc + l - 1, the slot-wise sum
 *    against fpksk_ntt, the output layout of cntt_prime_cbs.h.
 * Valid: everything cntt_prime*_circuit_bootstrap_batch requires, plus Lc <= 2^t <= n / 2 (the n / 2 keeps the two bit values n / 2
 * and 3 n / 2 on the coarse grid).  The width refusal becomes batch * (k + 1) * pbs_levels >= 2^32.  At t = 0, Lc = 1 the call equals
 * cntt_prime*_circuit_bootstrap_batch word for word.  Exactness and the strict-range caveat are those of cntt_prime_cbs.h.
 *
 * Noise.  The output error does not depend on t: the rotation is the same algebra on another table.  With binary keys and a key noise
 * |e| < E_k in every row of bsk_ntt, and pbs_base_log * pbs_levels = W, a bootstrap output is off by less than
 *     L * (k + 1) * n * pbs_levels * 2^(pbs_base_log - 1) * E_k                                             (cntt_prime_pbs.h)
 * in every extracted index.  tests/test_gpu_prime_manylut.py decodes under noisy keys at p = 2^64 - 2^32 + 1:
 *   - 2^t = 4 tables on every message of a 3-bit space under one padding bit, n = 128, k = 1, L = 2, PBS gadget (32, 2), E_k = 2^4:
 *     the bound is 2 * 2 * 128 * 2 * 2^31 * 2^4 = 2^45 against half a step of 2^59.  A message owns a box of n' / 8 = 4 coarse steps,
 *     shifted by half a box; with an input noise below 2^20, D = 1.5 + (2^20 + 1) * 64 / p < 2 = half a box.
 *   - the address bits of a CMux tree at M = 8 through the one-rotation circuit bootstrap with the shapes and noises of the test of
 *     cntt_prime_cbs.h (n = 64, k = 1, L = 8, gadgets (16, 4), (22, 2), (8, 3), t = 2, E_k = 2^4, input noise 2^40): a row of a selector
 *     is off by less than 2^38 and the tree's output by less than 2^56, derived there; D = 4.5 + (2^40 + 1) * 32 / p < 4.6 against the
 *     margin n / 2^(t + 1) = 8 steps.
 * Worst errors observed: DESIGN.md.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word, a written operand disjoint from every other one.  Workspace of
 * the circuit bootstrap, with wb = sizeof(T), up(x) = x rounded up to a multiple of 256, E = batch * Lc and S from the slab rule of
 * cntt_prime_cbs.h for E elements (unchanged):
 *   cntt_prime*_circuit_bootstrap_manylut_workspace_bytes =
 *       up((L + 1) * batch * 4) + up((k + 1) * n * wb) + up(batch * (k + 1) * pbs_levels * n * wb) + up(batch * (k + 1) * n * wb)
 *       + up(E * R * 4) + up(S * (k + 1) * E * (k + 1) * n * wb)
 *   (rot_t | the table | the digits of the rotation | the accumulators | the int32 digits | the slab sums, in this order).
 *   16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device path is
 *   one stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain (n <= 2048 on 64-bit words,
 *   n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear chain of kernels and may be
 *   captured into a hipGraph.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call): log_lut_count > logn;
 * lut_count == 0 or lut_count > 2^log_lut_count; count == 0 or count > n; cbs_levels > 2^log_lut_count; 2^log_lut_count > n / 2 in the
 * circuit bootstrap; and the cases of the calls each one is made of.  batch == 0 does nothing.  where / stream as every other _batch
 * call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  The circuit bootstrap rotates batch elements where cntt_prime*_circuit_bootstrap_batch rotates batch * Lc; the rotation is
 * 28 of that call's 28 - 33 ms at n = 1024, L = 630 while it is launch-bound.
 * Measured on 64-bit words at p = 4611686018427322369, n = 1024, k = 1, lwe_dim = 630, PBS gadget (22, 2), keyswitch gadget (22, 1)
 * (profiles/r29_prime_manylut.txt; tools/prime_manylut_bench.py takes the figures; one run, 2.39 GHz after it), ms per call, the new
 * call / the call it replaces, batch 1, 64, 1024, 4096:
 *   circuit bootstrap, Lc = 2, t = 1:  28.24 / 28.33,   29.55 / 30.44,   43.37 / 61.71,    124.47 / 239.37    (1.00, 1.03, 1.42, 1.92 times faster)
 *                      Lc = 4, t = 2:  28.27 / 28.63,   29.85 / 33.57,   49.31 / 115.50,   144.67 / 463.19    (1.01, 1.12, 2.34, 3.20)
 *   bootstrap, lut_count = 2 / 2 calls: 28.03 / 56.08,  28.80 / 57.64,   37.45 / 74.91,    103.91 / 207.70    (2.00 in every row)
 *              lut_count = 4 / 4 calls: 28.13 / 112.45, 28.80 / 115.27,  37.54 / 150.18,   103.68 / 414.70    (4.00 in every row)
 *   extraction of Lc indices / Lc single extractions: 0.009 - 0.027 / 0.019 - 0.055 (2.0 and 4.0 times faster up to batch 1024, 1.60 and
 *   2.07 at batch 4096).
 * No measured row where a new call loses.  No gain while the rotation is launch-bound (batch * Lc in the tens); beyond, the gain approaches
 * Lc and stops short of it because the keyswitch half still runs over batch * Lc elements.  Other sizes, 32-bit words and k > 1 were not
 * measured.  The chunk of 8 rows of the extraction is an ASSUMPTION: no A/B has been recorded. */
#ifndef CNTT_PRIME_MANYLUT_H
#define CNTT_PRIME_MANYLUT_H

#include "cntt_prime_cbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* rot_t as cntt_prime64_lwe_modswitch_batch writes it, with ms_t.  CNTT_EINVAL for log_lut_count > logn and that call's cases. */
int cntt_prime64_lwe_modswitch_manylut_batch(const cntt_plan64_t *plan, uint32_t *rot_t, const uint64_t *lwe, size_t lwe_dim,
                                             unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream);

/* lwe_out: batch x count x (k * n + 1) words; glwe: batch x (k + 1) polynomials.  1 <= count <= n.  CNTT_EINVAL for a count outside
 * that range, a NULL argument and lwe_out overlapping glwe. */
int cntt_prime64_sample_extract_many_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *glwe, size_t glwe_dim, size_t count,
                                           size_t batch, cntt_mem_t where, void *stream);

/* the coarse modulus switch, cntt_prime64_blind_rotate_batch and the extraction of the indices 0 .. lut_count - 1 in one call: lwe_in is
 * batch x (L + 1) words, lwe_out batch x lut_count x (k * n + 1) words; workspace: cntt_prime64_pbs_workspace_bytes.
 * 1 <= lut_count <= 2^log_lut_count.  CNTT_EINVAL for the cases of the three calls and of cntt_prime64_bootstrap_batch. */
int cntt_prime64_bootstrap_manylut_batch(const cntt_plan64_t *plan, uint64_t *lwe_out, const uint64_t *lwe_in, const uint64_t *lut,
                                         int lut_per_element, const uint64_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                         unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch, void *workspace,
                                         size_t workspace_bytes, cntt_mem_t where, void *stream);

/* the arguments of cntt_prime64_circuit_bootstrap_batch and log_lut_count; cbs_levels <= 2^log_lut_count <= n / 2 */
int cntt_prime64_circuit_bootstrap_manylut_batch(const cntt_plan64_t *plan, uint64_t *ggsw_ntt_out, const uint64_t *lwe_in,
                                                 const uint64_t *bsk_ntt, const uint64_t *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,
                                                 unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                 unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut_count, size_t batch,
                                                 void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_prime64_circuit_bootstrap_manylut_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                              unsigned ks_levels, unsigned cbs_levels, size_t batch);

/* ---- prime32: the same five calls on 32-bit words --------------------------------------------------------------------------------- */
int cntt_prime32_lwe_modswitch_manylut_batch(const cntt_plan32_t *plan, uint32_t *rot_t, const uint32_t *lwe, size_t lwe_dim,
                                             unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_sample_extract_many_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *glwe, size_t glwe_dim, size_t count,
                                           size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_bootstrap_manylut_batch(const cntt_plan32_t *plan, uint32_t *lwe_out, const uint32_t *lwe_in, const uint32_t *lut,
                                         int lut_per_element, const uint32_t *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                         unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch, void *workspace,
                                         size_t workspace_bytes, cntt_mem_t where, void *stream);
int cntt_prime32_circuit_bootstrap_manylut_batch(const cntt_plan32_t *plan, uint32_t *ggsw_ntt_out, const uint32_t *lwe_in,
                                                 const uint32_t *bsk_ntt, const uint32_t *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,
                                                 unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                 unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut_count, size_t batch,
                                                 void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_circuit_bootstrap_manylut_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                              unsigned ks_levels, unsigned cbs_levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_MANYLUT_H */
