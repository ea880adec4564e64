/* The many-LUT programmable bootstrap on the native plans (ciphertext modulus 2^32 / 2^64 / 2^128), and the circuit bootstrap that runs
 * ONE blind rotation per input bit instead of one per selector level: the PBSmanyLUT of Chillotti, Ligier, Orfila and Tap (Asiacrypt
 * 2021).  The modulus switch clears the low log_lut_count bits of every exponent, so that the rotated table keeps 2^log_lut_count
 * neighbouring coefficients intact, and one rotation evaluates up to 2^log_lut_count functions of the encrypted message, extracted at the
 * indices 0, 1, ...  The counterpart mod p is cntt_prime_manylut.h.  No counterpart in the reference; the convention below is this
 * library's own, fixed to the last bit.  No key or noise generation: the caller brings the keys.  Include this file on its own (it
 * includes cntt_cbs.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_pbs.h and cntt_cbs.h: w = the word width of the plan's kind, wb = w / 8, n = ntt_size = 2^logn, k = glwe_dim,
 * L = lwe_dim, Lin = k * n, Lk = ks_levels, R = (Lin + 1) * Lk, Lc = cbs_levels, E = batch * Lc, every word little-endian.  New:
 * t = log_lut_count, 0 <= t <= logn, and n' = n / 2^t.
 *
 * Coarse modulus switch.  ms_t(x) = 2^t * ((((x >> (w - (logn - t) - 2)) + 1) >> 1) mod 2n'): the ms of cntt_pbs.h for the ring size n',
 * shifted left by t.  Ties go up and a result of 2n' wraps to 0, as there.  Only the top 32 bits of a word are read (logn - t + 2 <= 32
 * follows from logn <= 30).  ms_0 = ms, word for word.
 *   rot_t[i * batch + b] = ms_t(lwe[b][i])                  for i < L
 *   rot_t[L * batch + b] = (2n - ms_t(lwe[b][L])) mod 2n    (the body, negated; still a multiple of 2^t)
 * the transposed layout of cntt_native_lwe_modswitch_batch.
 *
 * Interleaved table.  For an exponent a = 0 mod 2^t and h < 2^t, coefficient h of X^(-a) v is v[a + h] for a < n and -v[a + h - n]
 * for a >= n: a + h never straddles n, because a and n are multiples of 2^t.  Function h of the table therefore lives at the
 * coefficients v[m * 2^t + h], m < n': a table of n' boxes per function, the 2^t functions interleaved.
 *
 * Multi-index extraction.  lwe_out[b][h], h < count, is exactly cntt_native_sample_extract_batch(glwe[b], index = h):
 *   lwe_out[b][h][q * n + j] = glwe[b][q][h - j]  for j <= h,  else  -glwe[b][q][h - j + n] mod 2^w        (q < k, j < n)
 *   lwe_out[b][h][k * n]     = glwe[b][k][h]
 * The layout is batch x count x (k * n + 1) words.  1 <= count <= n.  (A plan whose polynomial is shorter than 16 bytes -- n * wb < 16 --
 * is refused by this call and by the two built on it.)
 *
 * The many-LUT bootstrap is the coarse modulus switch, cntt_native_blind_rotate_batch UNCHANGED and the multi-index extraction with
 * count = lut_count, 1 <= lut_count <= 2^t.  Its workspace is exactly cntt_native_pbs_workspace_bytes (digits | rot_t | acc): there is no
 * new size function.  It accepts every kind cntt_native_bootstrap_batch accepts, the binary kinds included.  At t = 0, lut_count = 1 it
 * equals cntt_native_bootstrap_batch word for word.  It allocates and may be captured into a hipGraph under the conditions of that call.
 *
 * The one-rotation circuit bootstrap.  Arguments, input, output layout, keys (fpksk as plain words, 16-byte aligned) and steps 3 - 4 are
 * those of cntt_native_circuit_bootstrap_batch (cntt_cbs.h), with G_l = 2^(w - cbs_base_log * l) and H_l = 2^(w - cbs_base_log * l - 1):
 * 1. lwe'[b] = lwe_in[b] with 2^(w - 2) added to the body (wrapping): only bit 30 of the top 32 bits is touched.
 * 2. ONE table shared by the batch (lut_per_element = 0): the mask polynomials zero, the body polynomial
 *      v[m * 2^t + h] = 2^w - H_(h+1)  for h < Lc,   0  for Lc <= h < 2^t        (m < n').
 *    u[b][l] = the many-LUT bootstrap of lwe'[b] with this table and the PBS gadget, extracted at the index l - 1, and then H_l added
 *    to its body word mod 2^w.  The blind rotation runs over batch elements, not over E = batch * Lc.
 *    With noise-free keys (and pbs_base_log * pbs_levels = w, so that nothing is rounded) the phase of u[b][l] is exactly 0 for the
 *    bit 0 and G_l for the bit 1:
 *      the accumulator is X^(-a) v with a = the coarsely switched phase of lwe' in Z_2n, a multiple of 2^t; its coefficient l - 1 is
 *      v[a + l - 1] = -H_l for a < n and -v[a + l - 1 - n] = +H_l for a >= n.  ms_t(2^(w - 2)) = n / 2 and
 *      ms_t(2^(w - 1) + 2^(w - 2)) = 3 n / 2, both on the coarse grid because 2^t <= n / 2, so the bit 0 sits at a = n / 2, the bit 1 at
 *      a = 3 n / 2, and the body is -H_l + H_l = 0 or H_l + H_l = G_l.
 *    The margin is n / 2^(t + 1) steps of the coarse switch (n / 2 exponents, as before, but a step is now 2^t exponents).  Every
 *    switched word that enters the exponent -- the body and the mask words whose key bit is 1, L + 1 at the most -- is off by at most
 *    half a step (ties exist mod 2^w, unlike mod p), and an input noise e moves the phase by |e| * 2n' / 2^w steps: the exponent is a
 *    whole number of steps off by at most D = (L + 1) / 2 + |e| * 2n' / 2^w, and the bit is read right when D < n / 2^(t + 1).
 * 3. Unchanged: the int32 digits of all Lin + 1 words of u[b][l] for (ks_base_log, Lk), element e = b * Lc + l - 1, the wrapping
 *    digit x key product in slabs and the negated sum of the slabs (native_cbs_ks_kernel, native_cbs_sum_kernel, called as they are).
 * 4. Unchanged: the split into residues and the forward transforms into the caller's planes, the output layout of cntt_cbs.h.
 * Valid: everything cntt_native_circuit_bootstrap_batch requires (the binary kinds refused, cbs_base_log * Lc <= w - 1,
 * ks_base_log <= 31, R < 2^32, (k + 1) * pbs_levels <= cntt_native_max_terms), plus Lc <= 2^t <= n / 2 (the n / 2 keeps the two bit
 * values n / 2 and 3 n / 2 on the coarse grid).  The width refusals become batch * (k + 1) * pbs_levels >= 2^32 for the rotation and
 * batch * Lc * (k + 1)^2 * n >= 2^46 for the transforms (the second unchanged).  At t = 0, Lc = 1 the call equals
 * cntt_native_circuit_bootstrap_batch word for word.  Exactness is that of cntt_cbs.h.  The output error does not depend on t: the
 * rotation is the same algebra on another table, and u has the same exact phase.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word (a plane to its residue, fpksk to 16 bytes), a written operand
 * disjoint from every other one.  Workspace of the circuit bootstrap, with up(x) = x rounded up to a multiple of 256 and S from the slab
 * rule of cntt_cbs.h for E elements (unchanged):
 *   cntt_native_circuit_bootstrap_manylut_workspace_bytes =
 *       up((L + 1) * batch * 4) + up((k + 1) * n * wb) + up(batch * (k + 1) * pbs_levels * n * wb) + up(batch * (k + 1) * n * wb)
 *       + up(E * R * 4) + up(S * (k + 1) * E * (k + 1) * n * wb) + up((k + 1) * E * (k + 1) * n * wb)
 *   (rot_t | the table | the digits of the rotation | the accumulators | the int32 digits | the slab sums | the selector words, in this
 *   order).  16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device
 *   path is one stream-ordered allocation for the whole call.  The graph-capture conditions are those of cntt_cbs.h: with a caller
 *   workspace the non-binary Plan32 kinds at 32 <= n <= 4096 make no allocation anywhere in the call after one eager call, which is then
 *   a linear chain of kernels (tested on native64 Plan32 at n = 1024).
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call): log_lut_count > logn;
 * lut_count == 0 or lut_count > 2^log_lut_count; count == 0 or count > n; cbs_levels > 2^log_lut_count; 2^log_lut_count > n / 2 in the
 * circuit bootstrap; and the cases of the calls each one is made of, the sizes that would pass 2^63 bytes included (checked before the
 * products are formed).  batch == 0 does nothing.  where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device
 * path, copies out and synchronises.
 *
 * Cost.  The circuit bootstrap rotates batch elements where cntt_native_circuit_bootstrap_batch rotates batch * Lc.
 * Measured on the Plan32 kinds at n = 1024, k = 1, lwe_dim = 630, keyswitch gadget (22, 1), cbs_base_log = 4
 * (profiles/r30_native_manylut.txt; tools/native_manylut_bench.py takes the figures; one box, one run, every route in one process with
 * caller workspaces, 2.41 GHz after it), ms per call, the new call / the call or calls it replaces, batch 1, 64, 1024.
 * native64, PBS gadget (22, 2):
 *   circuit bootstrap, Lc = 2, t = 1:    51.61 / 52.87,    54.40 / 54.79,    72.23 / 101.73     (1.02, 1.01, 1.41 times faster)
 *                      Lc = 4, t = 2:    51.58 / 53.76,    54.47 / 58.42,    74.15 / 191.91     (1.04, 1.07, 2.59)
 *   bootstrap, lut_count = 2 / 2 calls:  51.44 / 102.81,   54.05 / 108.18,   67.22 / 134.37     (2.00 in every row)
 *              lut_count = 4 / 4 calls:  51.45 / 205.77,   54.05 / 216.48,   67.27 / 268.83     (4.00, 4.01, 4.00)
 * native32, PBS gadget (11, 2):
 *   circuit bootstrap, Lc = 2, t = 1:    38.95 / 39.18,    41.34 / 41.22,    54.31 / 70.41      (1.01, 1.00, 1.30)
 *                      Lc = 4, t = 2:    38.90 / 41.20,    41.42 / 41.92,    55.09 / 129.02     (1.06, 1.01, 2.34)
 *   bootstrap, lut_count = 2 / 2 calls:  38.72 / 77.43,    41.18 / 82.35,    49.71 / 99.41      (2.00 in every row)
 *              lut_count = 4 / 4 calls:  38.82 / 155.20,   41.16 / 164.59,   49.74 / 198.78     (4.00 in every row)
 *   extraction of Lc indices / Lc single extractions, both widths: 0.010 - 0.011 / 0.021 - 0.043 (2.0 and 4.0 times faster; every one of
 *   these launches is launch-bound at these sizes).
 * ONE measured row where a new call loses: native32, Lc = 2, batch 64, 41.34 against 41.22 ms, 0.3 %; a single run cannot tell that
 * from parity, and it has not been tuned away.  As on the prime plans there is no gain while the rotation is launch-bound (batch * Lc in
 * the tens to hundreds: 630 iterations of two launches take 39 - 55 ms whatever the batch); beyond, the gain approaches Lc and stops short
 * of it because the keyswitch half and the transforms still run over batch * Lc elements.  128-bit words, the Plan52 kinds, k > 1, other
 * sizes and batches above 1024 were not measured.
 * Kernels, gfx950: the modulus switch 17 VGPRs (23 with the circuit bootstrap's set-up) and 4224 bytes of LDS; the extraction of several
 * indices 34 / 42 / 55 VGPRs on 32- / 64- / 128-bit words; the circuit bootstrap's extraction 22 - 38; occupancy 8, no scratch, no spills
 * in all fifteen.  The chunk of 8 rows of the extraction is an ASSUMPTION carried over from cntt_prime_manylut.h: no A/B has been
 * recorded. */
#ifndef CNTT_MANYLUT_H
#define CNTT_MANYLUT_H

#include "cntt_cbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rot_t as cntt_native_lwe_modswitch_batch writes it, with ms_t.  CNTT_EINVAL for log_lut_count > logn and that call's cases. */
int cntt_native_lwe_modswitch_manylut_batch(const cntt_native_t *plan, uint32_t *rot_t, const void *lwe, size_t lwe_dim,
                                            unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream);

/* lwe_out: batch x count x (k * n + 1) words; glwe: batch x (k + 1) polynomials.  1 <= count <= n.  CNTT_EINVAL for a count outside
 * that range, a NULL argument and lwe_out overlapping glwe. */
int cntt_native_sample_extract_many_batch(const cntt_native_t *plan, void *lwe_out, const void *glwe, size_t glwe_dim, size_t count,
                                          size_t batch, cntt_mem_t where, void *stream);

/* the coarse modulus switch, cntt_native_blind_rotate_batch and the extraction of the indices 0 .. lut_count - 1 in one call: lwe_in is
 * batch x (L + 1) words, lwe_out batch x lut_count x (k * n + 1) words; workspace: cntt_native_pbs_workspace_bytes.
 * 1 <= lut_count <= 2^log_lut_count.  CNTT_EINVAL for the cases of the three calls and of cntt_native_bootstrap_batch. */
int cntt_native_bootstrap_manylut_batch(const cntt_native_t *plan, void *lwe_out, const void *lwe_in, const void *lut, int lut_per_element,
                                        const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                        unsigned log_lut_count, size_t lut_count, size_t batch, void *workspace, size_t workspace_bytes,
                                        cntt_mem_t where, void *stream);

/* the arguments of cntt_native_circuit_bootstrap_batch and log_lut_count; cbs_levels <= 2^log_lut_count <= n / 2 */
int cntt_native_circuit_bootstrap_manylut_batch(const cntt_native_t *plan, void *const *ggsw_ntt_out, const void *lwe_in,
                                                const void *const *bsk_ntt, const void *fpksk, size_t lwe_dim, size_t glwe_dim,
                                                unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut_count, size_t batch,
                                                void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_native_circuit_bootstrap_manylut_workspace_bytes(const cntt_native_t *plan, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                             unsigned ks_levels, unsigned cbs_levels, size_t batch);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_MANYLUT_H */
