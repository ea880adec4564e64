/* The circuit bootstrap on the prime32 / prime64 plans: LWE encryptions of bits in, GGSW selectors in the NTT domain out -- what
 * cntt_prime*_glwe_cmux_batch and cntt_prime*_cmux_tree_batch (cntt_prime_cmux.h) and the fixed-row blind rotation of a table lookup
 * consume, and the first half of the bootstrap without padding (WoP-PBS) of Chillotti, Ligier, Orfila and Tap (Asiacrypt 2021): one
 * programmable bootstrap per level of the selector, then a functional packing keyswitch per row block.  No counterpart in the reference
 * (concrete-ntt has no decomposer); the convention below is this library's own, fixed to the last bit so that an integrator can generate
 * matching keys.  No key or noise generation: the caller brings the keys.  Include this file on its own (it includes cntt_prime_cmux.h);
 * it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_prime_pbs.h and cntt_prime_cmux.h: T = the plan's word, p = the modulus, W = the bit length of p,
 * n = ntt_size, k = glwe_dim, L = lwe_dim.  Three gadgets: the PBS gadget (pbs_base_log, pbs_levels) of bsk_ntt, the keyswitch gadget
 * (ks_base_log, Lk = ks_levels) of fpksk_ntt, and the gadget of the selectors that are produced, (cbs_base_log, Lc = cbs_levels).
 * Lin = k * n, R = (Lin + 1) * Lk, E = batch * Lc.
 *
 * Input.  lwe_in is batch x (L + 1) words, the body last; element b has the phase bit_b * (p + 1) / 2 + e.
 * Output.  ggsw_ntt_out is batch selectors back to back, each (k + 1) * Lc * (k + 1) polynomials in exactly the layout
 * cntt_prime*_cmux_tree_batch reads: row j = q * Lc + (l - 1) at polynomial j * (k + 1) + o.  A call with batch = d address bits
 * therefore writes the ggsw_ntt argument of a tree of depth d: bit i is element i.
 *
 * The words, per element b and level l = 1 .. Lc, with G_l = 2^(W - cbs_base_log * l) and H_l = G_l * 2^-1 mod p (p is odd, so H_l is
 * exact: 2^(W - cbs_base_log * l - 1), and (p + 1) / 2 when cbs_base_log * Lc = W and l = Lc):
 * 1. lwe'[b] = lwe_in[b] with Q4 = floor((p + 2) / 4) added to the body mod p.
 * 2. u[b][l] = cntt_prime*_bootstrap_batch(lwe'[b], lut = the trivial GLWE ciphertext whose body polynomial has EVERY coefficient
 *    p - H_l, the PBS gadget), and then H_l added to its body word mod p.  u has Lin + 1 words.  With noise-free keys (and
 *    pbs_base_log * pbs_levels = W, so that nothing is rounded) its phase is exactly 0 for the bit 0 and G_l for the bit 1:
 *      the accumulator is X^(-a) * v with a = the switched phase of lwe' in Z_2n and v the constant polynomial -H_l; its coefficient 0 is
 *      v[a] = -H_l for a < n, and, because X^n = -1, -v[a - n] = +H_l for a >= n.  Q4 moves the bit 0 to a = n / 2 and the bit 1 to
 *      a = 3 n / 2, so the body is -H_l + H_l = 0 or H_l + H_l = G_l, each with a margin of n / 2 exponents for the noise.
 *    One blind rotation runs over all E elements (e = b * Lc + l - 1), not Lc separate ones.
 * 3. All Lin + 1 words of u[b][l], the body included, are decomposed with the CNTT_SRC_PLAIN digits of cntt_prime_pbs.h for
 *    (ks_base_log, Lk): the signed digits d_{i,j}, i <= Lin, j = 1 .. Lk.  For q <= k and o <= k, slot by slot (c < n):
 *      out[b][(q * Lc + l - 1) * (k + 1) + o][c] = - sum_{i <= Lin} sum_{j = 1 .. Lk} d_{i,j} * F_q[(i * Lk + j - 1) * (k + 1) + o][c]  mod p,
 *    canonical.
 *
 * Key.  bsk_ntt is that of cntt_prime_pbs.h for (pbs_base_log, pbs_levels).  fpksk_ntt is k + 1 keys F_0 .. F_k back to back, each
 * R * (k + 1) NTT-domain polynomials holding n^-1 * fwd(key polynomial) (cntt_prime*_fwd_batch, then cntt_prime*_normalize_batch).  Row
 * (i, j) of key q, at polynomial (i * Lk + j - 1) * (k + 1), is a GLWE encryption under the OUTPUT key S (k mask polynomials, body last)
 *   for i < Lin of the polynomial  s_in[i] * M_q * 2^(W - ks_base_log * j),
 *   for i = Lin of the polynomial        - M_q * 2^(W - ks_base_log * j),
 * with s_in the flattened GLWE key under which u is encrypted, as cntt_prime*_sample_extract_batch defines it (s_in[q * n + t] =
 * coefficient t of key polynomial q), M_q = -S_q for q < k and M_k = 1.
 * Phase.  The forward transform of a constant polynomial d is d in every slot, so step 3 is, back in the coefficient domain,
 * row(q, l) = - sum_{i,j} d_{i,j} * (key row (i, j) of F_q), whose phase under S is
 *   - M_q * (sum_{i < Lin} s_in[i] * r_i - r_Lin) * 2^s + noise  =  M_q * (u_body - sum_i s_in[i] u_i) + M_q * rounding + noise
 *   =  M_q * bit * G_l + M_q * rounding + noise,
 * with r_i * 2^s = sum_j d_{i,j} 2^(W - ks_base_log * j), s = W - ks_base_log * Lk and |r_i * 2^s - lift(u_i)| <= 2^(s - 1) (= 0 when
 * s = 0): the selector convention of cntt_prime_cmux.h, -bit * S_q * G_l for q < k and bit * G_l for q = k.  With noise-free keys and
 * a binary s_in the rounding part is a polynomial M_q * c with |c| <= (Lin + 1) * 2^(s - 1), the keyswitch ROUNDING BOUND; for q < k
 * and a binary S every coefficient of it is below n * (Lin + 1) * 2^(s - 1).  With a key noise |e| < E_k every coefficient of the phase
 * adds less than R * 2^(ks_base_log - 1) * E_k.
 *
 * Equality with public calls.  Step 3 equals, word for word and for the primes outside the strict-range caveat of cntt_prime_pbs.h,
 * cntt_prime*_pack_keyswitch_batch on the ciphertext (u, 0) -- lwe_dim_in = Lin + 1, lwe_count = 1, the body word 0, the key F_q --
 * followed by cntt_prime*_fwd_batch and cntt_prime*_normalize_batch: with one ciphertext packed every digit polynomial is a constant,
 * its transform that constant in every slot, and fwd / mul_accumulate / inv / fwd / normalize collapses to the slot-wise sum above.
 *
 * Exactness.  Step 3 is exact integer arithmetic mod p for EVERY prime the plans accept, the strict range included: it never calls
 * cntt_prime*_mul_accumulate.  Steps 1 - 2 have exactly the words of cntt_prime*_bootstrap_batch and inherit the caveat of
 * cntt_prime_pbs.h: inside the strict range (2^62 <= p < 2^63, 2^30 <= p < 2^31) the blind rotation equals the reference's
 * composition, not necessarily the big-integer product.
 *
 * Valid: the PBS conditions of cntt_prime_pbs.h (pbs_base_log, pbs_levels >= 1, pbs_base_log * pbs_levels <= W, logn <= 29);
 * cbs_base_log, Lc >= 1, cbs_base_log * Lc <= W; ks_base_log, Lk >= 1, ks_base_log * Lk <= W and ks_base_log <= 31, so that a signed
 * digit, the top digit's +-2^(ks_base_log - 1) included, fits an int32; R < 2^32.  batch == 0 does nothing.  lwe_dim == 0 is valid
 * (bsk_ntt may then be NULL; the rotation is the set-up alone).  Words >= p are not rejected and not reduced: the call completes
 * without a fault and the affected outputs are unspecified.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word, a written operand disjoint from every other one.  Workspace, with
 * wb = sizeof(T), up(x) = x rounded up to a multiple of 256 and ceil(a / b) the quotient rounded up:
 *   cols  = ceil((k + 1) * n / (256 * 16 / wb))                  (column blocks of one key)
 *   tiles = ceil(E / 8)                                          (tiles of 8 elements)
 *   S0    = max(1, min(ceil(R / 64), floor(2048 / ((k + 1) * cols * tiles))))
 *   rows  = ceil(R / S0),  S = ceil(R / rows)                    (the slabs of key rows)
 *   cntt_prime*_circuit_bootstrap_workspace_bytes =
 *       up((L + 1) * E * 4) + up(E * (k + 1) * n * wb) + up(E * (k + 1) * pbs_levels * n * wb) + up(E * (k + 1) * n * wb)
 *       + up(E * R * 4) + up(S * (k + 1) * E * (k + 1) * n * wb)
 *   (rot_t | the tables | the digits of the rotation | the accumulators | the int32 digits | the slab sums, in this order).
 *   16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device path is
 *   one stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain (n <= 2048 on 64-bit words,
 *   n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear chain of kernels and may be
 *   captured into a hipGraph.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; a base_log or
 * levels of zero or a product above W in any of the three gadgets; ks_base_log > 31; logn > 29; R >= 2^32;
 * batch * Lc * (k + 1) * pbs_levels >= 2^32 (what the widest launch holds); a NULL argument (bsk_ntt only when L > 0); a misaligned
 * pointer; a written operand (ggsw_ntt_out, the workspace) overlapping any other operand (byte ranges); a non-NULL workspace that is
 * misaligned or too small; sizes whose ciphertexts, keys, selectors or workspace would pass 2^63 bytes (checked before they are
 * formed).  where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  The public-call recipe -- Lc bootstraps, (k + 1) * Lc packing keyswitches at lwe_count = 1, fwd and normalize -- runs a full NTT
 * external product per key row; this call reads every key word once per tile of 8 elements and multiplies it by a 32-bit digit.  The
 * functional key is (k + 1) * R * (k + 1) * n words: 67 MB at n = 1024, k = 1, Lk = 1 on 64-bit words.
 * Measured on 64-bit words at n = 1024, k = 1, lwe_dim = 630, PBS gadget (22, 2) (profiles/r24_prime_cbs.txt; tools/prime_cbs_bench.py
 * takes the figures), ms per call, this call / the public-call sequence, batch 1, 10, 64:
 *   keyswitch gadget (22, 1), Lc = 2:  28.31 / 84.97,   28.81 / 85.93,   30.48 / 87.68      (3.00, 2.98, 2.88 times faster)
 *                             Lc = 4:  28.64 / 170.02,  29.07 / 171.85,  33.12 / 175.49     (5.94, 5.91, 5.30)
 *   keyswitch gadget (11, 2), Lc = 2:  28.37 / 113.64,  28.92 / 114.76,  30.74 / 117.07     (4.01, 3.97, 3.81)
 *                             Lc = 4:  28.56 / 227.00,  29.23 / 229.43,  33.63 / 234.07     (7.95, 7.85, 6.96)
 * No measured shape at which the one-call form loses.  Most of the gain is the blind rotation run once over all levels instead of Lc
 * times (it is launch-bound at these batches); the keyswitch half alone takes 0.14 - 1.61 ms, 0.2 - 1.3 TB/s of key bytes per tile of 8
 * elements against the 6.29 TB/s a copy reaches: it is bound by integer multiplies and carry chains, not by bandwidth.  Other sizes,
 * 32-bit words and k > 1 were not measured.  The tile of 8 elements, the 64-row minimum of a slab and the grid cap are ASSUMPTIONS: no
 * A/B has been recorded. */
#ifndef CNTT_PRIME_CBS_H
#define CNTT_PRIME_CBS_H

#include "cntt_prime_cmux.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* ggsw_ntt_out: batch x (k + 1) * cbs_levels * (k + 1) polynomials, only written; lwe_in: batch x (L + 1) words; bsk_ntt as in
 * cntt_prime_pbs.h; fpksk_ntt: (k + 1) x R * (k + 1) polynomials as above */
int cntt_prime64_circuit_bootstrap_batch(const cntt_plan64_t *plan, uint64_t *ggsw_ntt_out, const uint64_t *lwe_in, const uint64_t *bsk_ntt,
                                         const uint64_t *fpksk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned pbs_base_log, unsigned pbs_levels,
                                         unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, size_t batch,
                                         void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_prime64_circuit_bootstrap_workspace_bytes(const cntt_plan64_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                      unsigned ks_levels, unsigned cbs_levels, size_t batch);

/* ---- prime32: the same two calls on 32-bit words ---------------------------------------------------------------------------------- */
int cntt_prime32_circuit_bootstrap_batch(const cntt_plan32_t *plan, uint32_t *ggsw_ntt_out, const uint32_t *lwe_in, const uint32_t *bsk_ntt,
                                         const uint32_t *fpksk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned pbs_base_log, unsigned pbs_levels,
                                         unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, size_t batch,
                                         void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_circuit_bootstrap_workspace_bytes(const cntt_plan32_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                      unsigned ks_levels, unsigned cbs_levels, size_t batch);

/* Workgroups the product kernel launches for `items` work items -- (k + 1) keys x tiles x cols x S of the formula above -- of 2^logn
 * words of word_bytes bytes (a grid-stride walk serves the rest): one per item up to 8 per CU of a 256-CU part.  For tests and tools,
 * like cntt_prime_cmux_grid: pure arithmetic, no device call. */
unsigned cntt_prime_cbs_grid(size_t items, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_CBS_H */
