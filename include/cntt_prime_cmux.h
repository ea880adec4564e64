/* The CMux and the CMux tree against GGSW selectors on the prime32 / prime64 plans: out = c0 + ExtProd(GGSW(b), c1 - c0) on two
 * DIFFERENT GLWE ciphertexts, and the binary tree of such nodes that selects one of M = lut_count plaintext table entries by log2 M
 * encrypted address bits -- the tree of "vertical packing", the second half of the bootstrap without padding (WoP-PBS) of Chillotti,
 * Ligier, Orfila and Tap ("Improved programmable bootstrapping with larger precision and efficient arithmetic circuits for TFHE",
 * Asiacrypt 2021).  CNTT_SRC_CMUX of cntt_prime_pbs.h is only the special case c1 = X^a c0 inside the blind rotation.  No counterpart
 * in the reference (concrete-ntt has no decomposer); the convention below is this library's own, fixed to the last bit.  No key or noise
 * generation: the caller brings the selectors.  Include this file on its own (it includes cntt_prime_pbs.h); it is not part of cntt.h
 * or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_prime_pbs.h: T = the plan's word, p = the modulus, W = the bit length of p, n = ntt_size, k = glwe_dim,
 * B = 2^base_log, a GLWE ciphertext = its k mask polynomials with the body polynomial last.  A SELECTOR is one GGSW ciphertext in the
 * NTT domain, (k + 1) * levels * (k + 1) polynomials: row j = q * levels + (l - 1) sits at polynomial j * (k + 1) + o and holds
 * n^-1 * fwd(a GLWE encryption of zero with bit * 2^(W - base_log * l) added to its polynomial q: a mask polynomial for q < k, the
 * body for q = k) -- exactly the layout and the convention of one iteration's slice of bsk_ntt in cntt_prime_pbs.h.  The phase of row
 * (q, l) is -bit * S_q * 2^(W - base_log * l) for q < k and bit * 2^(W - base_log * l) for q = k, plus the row's noise.  A selector is
 * shared by the whole batch, because the key of cntt_prime*_external_product_batch is.
 *
 * 1. glwe_cmux_batch.  For every batch element b, out = c0 + ExtProd(sel, c1 - c0) with c0 = glwe0[b], c1 = glwe1[b].  The words are
 *    exactly those of this sequence:
 *      glwe_out[b] = glwe0[b];
 *      d[b][q] = glwe1[b][q] - glwe0[b][q] mod p, canonical, for q <= k;
 *      cntt_prime*_gadget_decompose_batch(terms, d, CNTT_SRC_PLAIN, npolys = k + 1)   -- the digits are NOT negated;
 *      cntt_prime*_external_product_batch(glwe_out, terms, ggsw_ntt, nterms = (k + 1) * levels, nout = k + 1, accumulate = 1).
 *    One kernel reads c0 and c1 once and writes the prefill and the terms; d is never stored.  k == 0 is valid: one polynomial is
 *    decomposed.  Phase: with a noise-free selector of the bit a and base_log * levels = W, phase(out) = phase(c0) + a (phase(c1) -
 *    phase(c0)): c0 for a = 0, c1 for a = 1.
 *
 * 2. cmux_tree_batch.  M = lut_count is a power of two, M >= 1, depth = log2 M.  lut_in is batch x M PLAIN polynomials of n words, the
 *    table entries: plaintexts, not ciphertexts.  ggsw_ntt holds `depth` selectors back to back; selector i belongs to address bit i
 *    (the least significant bit is bit 0).  With c_0[j] = the trivial GLWE ciphertext of lut_in[b][j] (zero masks, the body is the
 *    polynomial):
 *      for s = 1 .. depth, h = M / 2^s:  c_s[j] = cmux(sel = selector depth - s, c0 = c_(s-1)[j], c1 = c_(s-1)[j + h])  for j < h;
 *      glwe_out[b] = c_depth[0].
 *    With noise-free selectors of the bits a_i, glwe_out[b] is the trivial encryption of lut_in[b][a], a = sum a_i 2^i; with noisy ones
 *    it is that plus noise.  The top address bit is consumed first, so entry j and entry j + M / 2 meet in stage 1.
 *    STAGE 1 (the leaf form) never materialises the trivial ciphertexts and never decomposes their zero masks.  Its words are DEFINED
 *    as: out masks = 0; out body = lut[j]; terms = the `levels` CNTT_SRC_PLAIN digit polynomials of lut[j + h] - lut[j] mod p;
 *    cntt_prime*_external_product_batch(nterms = levels, nout = k + 1, accumulate = 1) against the selector's BODY rows only: the key
 *    pointer is advanced by k * levels * (k + 1) polynomials.  The digits of a zero polynomial are all zero and a zero term adds zero to
 *    an exact sum, so for the primes outside the strict-range caveat of cntt_prime_pbs.h this equals call 1 on the trivial ciphertexts;
 *    inside the strict range the wrapping reduction of the reference may differ between the two, and the definition above holds.
 *    Stages >= 2 are call 1 on the batch * h pairs of that stage.  M == 1 writes the trivial ciphertext: no key is read, ggsw_ntt may be
 *    NULL and no allocation is made.
 *
 * From the tree to a whole table lookup.  A table of M * n entries (one per coefficient) under an address of log2 M + log2 n bits:
 * the tree over the TOP log2 M bits leaves the GLWE ciphertext of polynomial a_hi of the table; the LOW log2 n bits then rotate it with
 * cntt_prime*_blind_rotate_batch -- lut = the tree's output with lut_per_element = 1, lwe_dim = log2 n, bsk_ntt = the selectors of the
 * low bits (bit i is iteration i), and rot_t set by the caller, NOT by the modulus switch: rot_t[i * batch + b] = 2n - 2^i for
 * i < log2 n (iteration i multiplies by X^(-2^i) where bit i is set) and the body row rot_t[log2 n * batch + b] = 0 -- and
 * cntt_prime*_sample_extract_batch(index = 0) returns the LWE ciphertext of entry a.  examples/lookup_prime.c does exactly that.
 *
 * Exactness: that of cntt_prime_pbs.h.  The difference and the digits are exact integer arithmetic for every prime the plans accept;
 * the external product is cntt_prime*_external_product_batch word for word, so the calls equal the public-call sequences above for
 * EVERY prime and the big-integer formulas outside the strict-range caveat of cntt_prime_pbs.h.
 *
 * Valid: lut_count a power of two >= 1; base_log >= 1, levels >= 1, base_log * levels <= W; every size the external product accepts.
 * batch == 0 does nothing.  Words >= p are not rejected and not reduced: the call completes without a fault and the affected outputs
 * are unspecified.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word, a written operand disjoint from every other one.  No call here
 * runs in place.  Workspace, with up(x) = x rounded up to a multiple of 256, H = M / 2, Q = M / 4 (integer division, 0 allowed):
 *   cntt_prime*_glwe_cmux_workspace_bytes = up(batch * (k + 1) * levels * n * sizeof(T))                          (the digit polynomials)
 *   cntt_prime*_cmux_tree_workspace_bytes = up(max(batch * H * levels, batch * Q * (k + 1) * levels) * n * sizeof(T))
 *                                           + up(batch * H * (k + 1) * n * sizeof(T)) + up(batch * Q * (k + 1) * n * sizeof(T))
 *   (the digits of the widest stage and two ciphertext buffers: the stages alternate between them and the last stage writes glwe_out).
 *   16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device path is
 *   one stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain (n <= 2048 on 64-bit words,
 *   n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear chain of kernels and may be
 *   captured into a hipGraph.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; base_log == 0,
 * levels == 0, base_log * levels > W; lut_count zero or not a power of two; a NULL argument (ggsw_ntt only when M > 1); a misaligned
 * pointer; a written operand (glwe_out, the workspace) overlapping any other operand (byte ranges); a non-NULL workspace that is
 * misaligned or too small; batch * max(H, 1) * (k + 1) * levels >= 2^32 (H = 1 in call 1: what the widest launch of the external
 * product holds); sizes whose ciphertexts, table, digits or selectors would pass 2^63 bytes (checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  Against the public-call sequence a node saves the stored difference, its read by the decomposition and the copy of c0: three
 * passes over the ciphertexts; the external product, which dominates, is the same.  Measured on 64-bit words at n = 1024, k = 1,
 * levels 2 and 4 (profiles/r23_prime_cmux.txt; tools/prime_cmux_bench.py takes the figures): the tree at M = 256, batch 64 is 1.49 and
 * 1.28 times faster than its public-call sequence, one CMux at batch 4096 1.59 and 1.32 times; no measured shape at which the one-call
 * form loses.  Other sizes, 32-bit words and k > 1 were not measured. */
#ifndef CNTT_PRIME_CMUX_H
#define CNTT_PRIME_CMUX_H

#include "cntt_prime_pbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* glwe0, glwe1, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ggsw_ntt: (k + 1) * levels * (k + 1) polynomials, one selector */
int cntt_prime64_glwe_cmux_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *glwe0, const uint64_t *glwe1,
                                 const uint64_t *ggsw_ntt, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_prime64_glwe_cmux_workspace_bytes(const cntt_plan64_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* lut_in: batch x lut_count polynomials; glwe_out: batch x (k + 1) polynomials; ggsw_ntt: log2 lut_count selectors back to back */
int cntt_prime64_cmux_tree_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *lut_in, const uint64_t *ggsw_ntt,
                                 size_t lut_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime64_cmux_tree_workspace_bytes(const cntt_plan64_t *plan, size_t lut_count, size_t glwe_dim, unsigned levels, size_t batch);

/* ---- prime32: the same four calls on 32-bit words --------------------------------------------------------------------------------- */
int cntt_prime32_glwe_cmux_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *glwe0, const uint32_t *glwe1,
                                 const uint32_t *ggsw_ntt, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_glwe_cmux_workspace_bytes(const cntt_plan32_t *plan, size_t glwe_dim, unsigned levels, size_t batch);
int cntt_prime32_cmux_tree_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *lut_in, const uint32_t *ggsw_ntt,
                                 size_t lut_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                 size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_cmux_tree_workspace_bytes(const cntt_plan32_t *plan, size_t lut_count, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the kernel of these calls launches for `polys` output polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest): one per polynomial up to 8 per CU of a 256-CU part; nothing is staged, so the size does not enter.  For tests and
 * tools, like cntt_prime_ring_pack_grid: pure arithmetic, no device call. */
unsigned cntt_prime_cmux_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_CMUX_H */
