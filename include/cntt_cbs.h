/* The circuit bootstrap on the native plans (ciphertext modulus 2^32 / 2^64 / 2^128): LWE encryptions of bits in, GGSW selectors as residue
 * planes out -- what cntt_native_glwe_cmux_batch and cntt_native_cmux_tree_batch (cntt_cmux.h) and the fixed-row blind rotation of a table
 * lookup consume, and the first half of the bootstrap without padding (WoP-PBS) of Chillotti, Ligier, Orfila and Tap (Asiacrypt 2021): one
 * programmable bootstrap per level of the selector, then a functional packing keyswitch per row block.  The counterpart mod p is
 * cntt_prime_cbs.h.  No counterpart in the reference (concrete-ntt has no decomposer); the convention below is this library's own, fixed
 * to the last bit so that an integrator can generate matching keys.  No key or noise generation: the caller brings the keys.  Include
 * this file on its own (it includes cntt_cmux.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_pbs.h and cntt_cmux.h: w = the word width of the plan's kind, wb = w / 8 = cntt_native_word_bytes, rb =
 * cntt_native_residue_bytes, n = ntt_size, k = glwe_dim, L = lwe_dim, every word little-endian (a 128-bit word: 16 bytes, low half
 * first).  Three gadgets: the PBS gadget (pbs_base_log, pbs_levels) of bsk_ntt, the keyswitch gadget (ks_base_log, Lk = ks_levels) of
 * fpksk, and the gadget of the selectors that are produced, (cbs_base_log, Lc = cbs_levels).  Lin = k * n, R = (Lin + 1) * Lk,
 * E = batch * Lc with element e = b * Lc + (l - 1), G_l = 2^(w - cbs_base_log * l), H_l = 2^(w - cbs_base_log * l - 1).
 *
 * Input.  lwe_in is batch x (L + 1) words, the body last; element b has the phase bit_b * 2^(w - 1) + noise.
 * Output.  ggsw_ntt_out is cntt_native_nprimes plane pointers; every plane holds batch selectors back to back, each (k + 1) * Lc * (k + 1)
 * residue polynomials in exactly the layout cntt_native_cmux_tree_batch reads: row j = q * Lc + (l - 1) at polynomial j * (k + 1) + o.  A
 * call with batch = d address bits therefore writes the ggsw_ntt argument of a tree of depth d: selector i = batch element i = address
 * bit i.
 *
 * The words, per element b and level l = 1 .. Lc:
 * 1. lwe'[b] = lwe_in[b] with 2^(w - 2) added to the body (wrapping).
 * 2. u[b][l] = cntt_native_bootstrap_batch(lwe'[b], lut = the trivial GLWE ciphertext whose body polynomial has EVERY coefficient
 *    2^w - H_l, the PBS gadget) word for word, and then H_l added to its body word mod 2^w.  u has Lin + 1 words.  With noise-free keys
 *    (and pbs_base_log * pbs_levels = w, so that nothing is rounded) its phase is exactly 0 for the bit 0 and G_l for the bit 1:
 *      the accumulator is X^(-a) * v with a = the sum of ms() (cntt_pbs.h) over the body and the masked words of lwe', the switched phase
 *      in Z_2n, and v the constant polynomial -H_l; its coefficient 0 is v[a] = -H_l for a < n, and, because X^n = -1, -v[a - n] = +H_l
 *      for a >= n.  ms(2^(w - 2)) = n / 2 and ms(2^(w - 1) + 2^(w - 2)) = 3 n / 2, so the bit 0 sits at a = n / 2 and the bit 1 at
 *      a = 3 n / 2, and the body is -H_l + H_l = 0 or H_l + H_l = G_l, each with a margin of n / 2 exponents for the noise and the drift
 *      of the L + 1 roundings of ms().
 *    One blind rotation runs over all E elements, not Lc separate ones.
 * 3. All Lin + 1 words of u[b][l], the body included, are decomposed into the signed CNTT_SRC_PLAIN digits of cntt_gadget.h for
 *    (ks_base_log, Lk): d_{i,j} in [-B / 2, B / 2), i <= Lin, j = 1 .. Lk.  For q <= k and o <= k, slot by slot (c < n), the selector WORDS
 *      sel[b][(q * Lc + l - 1) * (k + 1) + o][c] = - sum_{i <= Lin} sum_{j = 1 .. Lk} d_{i,j} * F_q[(i * Lk + j - 1) * (k + 1) + o][c]  mod 2^w.
 *    The digit polynomials are constants, so the negacyclic product is a scalar multiple: no transform is involved.
 * 4. ggsw_ntt_out is exactly what one cntt_native_fwd_batch over sel (batch * (k + 1) * Lc * (k + 1) polynomials) writes: unnormalised,
 *    bit-reversed, the layout of cntt_cmux.h.
 *
 * Key.  bsk_ntt is that of cntt_pbs.h for (pbs_base_log, pbs_levels).  fpksk is PLAIN WORDS IN THE COEFFICIENT DOMAIN, not residue
 * planes: k + 1 keys F_0 .. F_k back to back, each R * (k + 1) polynomials of n words.  Row (i, j) of key q, at polynomial
 * (i * Lk + j - 1) * (k + 1), is a GLWE encryption under the OUTPUT key S (k mask polynomials, body last)
 *   for i < Lin of the polynomial  s_in[i] * M_q * 2^(w - ks_base_log * j),
 *   for i = Lin of the polynomial        - M_q * 2^(w - ks_base_log * j),
 * with s_in the flattened GLWE key under which u is encrypted, as cntt_native_sample_extract_batch defines it (s_in[q * n + t] =
 * coefficient t of key polynomial q), M_q = -S_q for q < k and M_k = 1.  Why plain words: step 3 is wrapping word arithmetic with no
 * transform in it, so a residue form would cost cntt_native_nprimes planes of key traffic instead of one and a CRT per output word, for
 * nothing.  fpksk is read in 16-byte vectors and must be 16-byte aligned.
 * Phase.  row(q, l) = - sum_{i,j} d_{i,j} * (key row (i, j) of F_q), whose phase under S is
 *   - M_q * (sum_{i < Lin} s_in[i] * r_i - r_Lin) * 2^s + noise  =  M_q * (u_body - sum_i s_in[i] u_i) + M_q * rounding + noise
 *   =  M_q * bit * G_l + M_q * rounding + noise,
 * with r_i * 2^s = sum_j d_{i,j} 2^(w - ks_base_log * j) mod 2^w, s = w - ks_base_log * Lk and |r_i * 2^s - u_i| <= 2^(s - 1) mod 2^w (= 0
 * when s = 0): the selector convention of cntt_cmux.h, -bit * S_q * G_l for q < k and bit * G_l for q = k.  With noise-free keys and a
 * binary s_in the rounding part is a polynomial M_q * c with |c| <= (Lin + 1) * 2^(s - 1), the keyswitch ROUNDING BOUND; for q < k and a
 * binary S every coefficient of it is below n * (Lin + 1) * 2^(s - 1).  With a key noise |e| < E_k every coefficient of the phase adds
 * less than R * 2^(ks_base_log - 1) * E_k.
 *
 * Equality with public calls.  Steps 1 - 2 are cntt_native_bootstrap_batch per level.  Step 3 equals, word for word,
 * cntt_native_pack_keyswitch_batch on the ciphertext (u, 0) -- lwe_dim_in = Lin + 1, lwe_count = 1, the body word 0, the key planes
 * cntt_native_fwd_batch of F_q: with one ciphertext packed every digit polynomial is a constant, and the packing keyswitch is exact by
 * its chunking rule (cntt_pack.h).  Step 4 is cntt_native_fwd_batch.
 *
 * Exactness.  Step 3 is exact arithmetic mod 2^w for every gadget the call accepts: it never enters a residue plane.  Steps 1 - 2 have
 * the words of cntt_native_bootstrap_batch, exact while (k + 1) * pbs_levels <= cntt_native_max_terms(plan).  (k + 1) * Lc against
 * cntt_native_max_terms is NOT checked here: the selectors are valid words whatever Lc is, and the consuming CMux call refuses a gadget
 * it cannot sum exactly.
 *
 * Valid: the PBS rules of cntt_pbs.h (pbs_base_log, pbs_levels >= 1, pbs_base_log * pbs_levels <= w, (k + 1) * pbs_levels <=
 * cntt_native_max_terms, log2 n <= 30); ks_base_log, Lk >= 1, ks_base_log * Lk <= w and ks_base_log <= 31, so that a signed digit fits an
 * int32; cbs_base_log, Lc >= 1 and cbs_base_log * Lc <= w - 1: H_l = G_l / 2 must be a word, and 2 has no inverse mod 2^w (mod p the
 * bound is W, because there 2^-1 exists); R < 2^32.  The binary kinds (native_binary32 / 64 / 128, Plan32 and Plan52) are refused: a
 * produced selector has full-width words, and those kinds' exactness rests on 0/1 key words.  batch == 0 does nothing.  lwe_dim == 0 is
 * valid (bsk_ntt may then be NULL; the rotation is the set-up alone).
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word (a plane to its residue, fpksk to 16 bytes), a written operand
 * (every output plane, the workspace) disjoint from every other one.  Workspace, with up(x) = x rounded up to a multiple of 256 and
 * ceil(a / b) the quotient rounded up:
 *   cols  = ceil((k + 1) * n / (256 * 16 / wb))                  (column blocks of one key)
 *   tiles = ceil(E / 8)                                          (tiles of 8 elements)
 *   S0    = max(1, min(ceil(R / 64), floor(2048 / ((k + 1) * cols * max(tiles, 1)))))
 *   rows  = ceil(R / S0),  S = ceil(R / rows)                    (the slabs of key rows)
 *   cntt_native_circuit_bootstrap_workspace_bytes =
 *       up((L + 1) * E * 4) + up(E * (k + 1) * n * wb) + up(E * (k + 1) * pbs_levels * n * wb) + up(E * (k + 1) * n * wb)
 *       + up(E * R * 4) + up(S * (k + 1) * E * (k + 1) * n * wb) + up((k + 1) * E * (k + 1) * n * wb)
 *   (rot_t | the tables | the digits of the rotation | the accumulators | the int32 digits | the slab sums | the selector words, in
 *   this order).  16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the
 *   device path is one stream-ordered allocation for the whole call.  With a caller workspace the non-binary Plan32 kinds at
 *   32 <= n <= 4096 (the fused external product of the blind rotation; the split and the sub-plans' transforms never allocate) make no
 *   allocation anywhere in the call once the plan's tables exist on the device, i.e. after one eager call: it is then a linear chain of
 *   kernels and may be captured into a hipGraph (tested on native64 Plan32 at n = 1024).  Elsewhere (Plan52, n < 32, n > 4096) the
 *   external product keeps allocating its own scratch, as cntt_pbs.h says of the blind rotation.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; a plan of a
 * binary kind; a base_log or levels of zero or a product above w in any of the three gadgets; ks_base_log > 31;
 * cbs_base_log * Lc > w - 1; (k + 1) * pbs_levels > cntt_native_max_terms(plan); R >= 2^32; batch * Lc * (k + 1) * pbs_levels >= 2^32 or
 * batch * Lc * (k + 1)^2 * n >= 2^46 (what the widest launches hold); a NULL argument, output plane or key plane (bsk_ntt only when
 * L > 0); a misaligned pointer; a written operand overlapping any other operand (byte ranges); a non-NULL workspace that is misaligned or
 * too small; sizes whose ciphertexts, keys, selectors or workspace would pass 2^63 bytes (checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  The public-call recipe -- Lc bootstraps, (k + 1) * Lc packing keyswitches at lwe_count = 1, one fwd -- runs a full NTT external
 * product per key row; this call reads every key word once per tile of 8 elements and multiplies it by a 32-bit digit into one wrapping
 * word.  The functional key is (k + 1) * R * (k + 1) * n words: 67 MB at n = 1024, k = 1, Lk = 1 on 64-bit words.
 * Measured at n = 1024, k = 1, lwe_dim = 630 on the Plan32 kinds (profiles/r26_native_cbs.txt; tools/native_cbs_bench.py takes the figures;
 * one box, one run), ms per call, this call / the public-call sequence, batch 1, 10, 64.  native64, PBS gadget (22, 2):
 *   keyswitch gadget (22, 1), Lc = 2:  52.87 / 154.60,  54.55 / 161.58,  54.90 / 166.90      (2.92, 2.96, 3.04 times faster)
 *                             Lc = 4:  53.35 / 308.74,  54.36 / 323.91,  59.81 / 334.18      (5.79, 5.96, 5.59)
 *   keyswitch gadget (11, 2), Lc = 2:  52.35 / 212.83,  54.22 / 221.76,  55.10 / 238.22      (4.07, 4.09, 4.32)
 *                             Lc = 4:  52.97 / 425.58,  54.40 / 443.58,  59.73 / 475.39      (8.04, 8.15, 7.96)
 * native32, PBS gadget (11, 2):
 *   keyswitch gadget (22, 1), Lc = 2:  38.90 / 117.77,  41.41 / 125.88,  41.26 / 126.32      (3.03, 3.04, 3.06)
 *                             Lc = 4:  40.90 / 234.19,  41.59 / 251.57,  41.98 / 252.67      (5.73, 6.05, 6.02)
 *   keyswitch gadget (11, 2), Lc = 2:  38.99 / 156.93,  41.40 / 169.97,  41.38 / 170.48      (4.02, 4.11, 4.12)
 *                             Lc = 4:  40.82 / 314.03,  41.68 / 339.51,  42.19 / 340.78      (7.69, 8.15, 8.08)
 * No measured shape at which the one-call form loses.  Most of the gain is the blind rotation run once over all levels instead of Lc
 * times.  The keyswitch half alone (the call at lwe_dim = 0: set-up, extraction, product, slab sum, split, transforms) takes 0.06 - 0.51
 * ms; at batch 1 and 10 that is the latency of its nine launches, at batch 64 the key bytes per tile of 8 elements pass at 2.5 - 4.3 TB/s
 * against the 6.29 TB/s a copy reaches (mod p: 0.2 - 1.3 TB/s): much closer to bandwidth than the prime kernel, but NOT bandwidth-bound
 * by that yardstick, and the key fits the Infinity Cache, so these are not HBM figures.  Product kernel, gfx950: 68 / 70 / 89 VGPRs on
 * 32- / 64- / 128-bit words, no scratch, no spills.  The end-to-end lookup of tests/test_gpu_native_cbs.py (n = 32, noise-free keys,
 * gadgets (16, 4), (22, 2), (8, 3)) has a worst error of 2^42.59 against its derived bound of 2^47.66.  128-bit words, the Plan52 kinds,
 * k > 1 and other sizes were not measured.  The tile of 8 elements, the 64-row minimum of a slab and the grid cap are ASSUMPTIONS: no A/B
 * has been recorded. */
#ifndef CNTT_CBS_H
#define CNTT_CBS_H

#include "cntt_cmux.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ggsw_ntt_out: cntt_native_nprimes planes of batch x (k + 1) * cbs_levels * (k + 1) residue polynomials, only written; lwe_in:
 * batch x (L + 1) words; bsk_ntt as in cntt_pbs.h; fpksk: (k + 1) x R * (k + 1) polynomials of plain words as above */
int cntt_native_circuit_bootstrap_batch(const cntt_native_t *plan, void *const *ggsw_ntt_out, const void *lwe_in, const void *const *bsk_ntt,
                                        const void *fpksk, size_t lwe_dim, size_t glwe_dim, unsigned pbs_base_log, unsigned pbs_levels,
                                        unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, size_t batch,
                                        void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_native_circuit_bootstrap_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                     unsigned ks_levels, unsigned cbs_levels, size_t batch);

/* Workgroups the product kernel launches for `items` work items -- (k + 1) keys x tiles x cols x S of the formula above -- of 2^logn
 * words of word_bytes bytes (a grid-stride walk serves the rest): one per item up to 8 per CU of a 256-CU part.  The rule is that of
 * cntt_prime_cbs_grid: an assumption about what fills the chip, not a measured optimum.  For tests and tools: pure arithmetic, no device
 * call. */
unsigned cntt_native_cbs_grid(size_t items, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_CBS_H */
