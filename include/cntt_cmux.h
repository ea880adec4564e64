/* The CMux and the CMux tree against GGSW selectors on the native plans (ciphertext modulus 2^32 / 2^64 / 2^128): out = c0 +
 * ExtProd(GGSW(b), c1 - c0) on two DIFFERENT GLWE ciphertexts, and the binary tree of such nodes that selects one of M = lut_count
 * plaintext table entries by log2 M encrypted address bits -- the tree of "vertical packing", the second half of the bootstrap without
 * padding (WoP-PBS) of Chillotti, Ligier, Orfila and Tap ("Improved programmable bootstrapping with larger precision and efficient
 * arithmetic circuits for TFHE", Asiacrypt 2021).  CNTT_SRC_CMUX of cntt_gadget.h is only the special case c1 = X^a c0 inside the blind
 * rotation.  The counterpart mod p is cntt_prime_cmux.h.  No counterpart in the reference; the convention below is this library's own,
 * fixed to the last bit.  No key or noise generation: the caller brings the selectors.  Include this file on its own (it includes
 * cntt_ext.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_pbs.h and cntt_gadget.h: w = the word width of the plan's kind, wb = w / 8 = cntt_native_word_bytes,
 * n = ntt_size, k = glwe_dim, B = 2^base_log, s = w - base_log * levels, a GLWE ciphertext = its k mask polynomials with the body
 * polynomial last, every word little-endian (a 128-bit word: 16 bytes, low half first).  A SELECTOR is one GGSW ciphertext in the key
 * form of cntt_native_external_product_batch: cntt_native_nprimes residue planes, each of (k + 1) * levels * (k + 1) residue
 * polynomials; row j = q * levels + (l - 1) sits at polynomial j * (k + 1) + o and is a GLWE encryption of zero with
 * bit * 2^(w - base_log * l) added to its polynomial q (a mask polynomial for q < k, the body for q = k).  The planes are unnormalised
 * and bit-reversed: exactly what one cntt_native_fwd_batch over the selector's polynomials writes (cntt_native_fwd_binary_batch for the
 * binary kinds, where the call is defined on the words only, as every call on those kinds) -- the layout and the convention of one
 * iteration's slice of bsk_ntt in cntt_pbs.h.  A selector is shared by the whole batch, because the key of the external product is.
 *
 * 1. cntt_native_glwe_cmux_batch.  For every batch element b, out = c0 + ExtProd(sel, c1 - c0) with c0 = glwe0[b], c1 = glwe1[b].  The
 *    words are exactly those of this sequence:
 *      glwe_out[b] = glwe0[b];
 *      d[b][q] = glwe1[b][q] - glwe0[b][q] mod 2^w, for q <= k;
 *      cntt_native_gadget_decompose_batch(terms, d, CNTT_SRC_PLAIN, npolys = k + 1);
 *      cntt_native_external_product_batch(glwe_out, terms, ggsw_ntt, nterms = (k + 1) * levels, nout = k + 1, accumulate = 1).
 *    One kernel reads c0 and c1 once and writes the prefill and the terms; d is never stored.  k == 0 is valid: one polynomial is
 *    decomposed.  Phase: with a noise-free selector of the bit a and base_log * levels = w, phase(out) = phase(c0) + a (phase(c1) -
 *    phase(c0)): c0 for a = 0, c1 for a = 1; with s > 0 the difference is rounded to a multiple of 2^s first.
 *
 * 2. cntt_native_cmux_tree_batch.  M = lut_count is a power of two, M >= 1, depth = log2 M.  lut_in is batch x M PLAIN polynomials of
 *    n words, the table entries: plaintexts, not ciphertexts.  Every plane of ggsw_ntt holds `depth` selectors back to back; selector i
 *    belongs to address bit i (the least significant bit is bit 0).  With c_0[j] = the trivial GLWE ciphertext of lut_in[b][j] (zero
 *    masks, the body is the polynomial):
 *      for s = 1 .. depth, h = M / 2^s:  c_s[j] = cmux(sel = selector depth - s, c0 = c_(s-1)[j], c1 = c_(s-1)[j + h])  for j < h;
 *      glwe_out[b] = c_depth[0].
 *    With noise-free selectors of the bits a_i and base_log * levels = w, glwe_out[b] is the trivial encryption of lut_in[b][a],
 *    a = sum a_i 2^i; with noisy ones it is that plus noise.  The top address bit is consumed first, so entry j and entry j + M / 2
 *    meet in stage 1.
 *    STAGE 1 (the leaf form) never materialises the trivial ciphertexts and never decomposes their zero masks.  Its words are DEFINED
 *    as: out masks = 0; out body = lut[j]; terms = the `levels` CNTT_SRC_PLAIN digit polynomials of lut[j + h] - lut[j] mod 2^w;
 *    cntt_native_external_product_batch(nterms = levels, nout = k + 1, accumulate = 1) against the selector's BODY rows only: every
 *    plane pointer is advanced by k * levels * (k + 1) residue polynomials.  The digits of a zero polynomial are all zero (its word y
 *    is the offset alone, whose fields are B / 2 each), a zero term adds zero to an exact integer sum, and the torus arithmetic is
 *    exact within cntt_native_max_terms; so the leaf form EQUALS call 1 on the trivial ciphertexts, word for word, for every kind.
 *    Stages >= 2 are call 1 on the batch * h pairs of that stage.  M == 1 writes the trivial ciphertext: no key is read, ggsw_ntt may
 *    be NULL and no allocation is made.
 *
 * From the tree to a whole table lookup.  A table of M * n entries (one per coefficient) under an address of log2 M + log2 n bits:
 * the tree over the TOP log2 M bits leaves the GLWE ciphertext of polynomial a_hi of the table; the LOW log2 n bits then rotate it with
 * cntt_native_blind_rotate_batch -- lut = the tree's output with lut_per_element = 1, lwe_dim = log2 n, bsk_ntt = the selectors of the
 * low bits (bit i is iteration i), and rot_t set by the caller, NOT by the modulus switch: rot_t[i * batch + b] = 2n - 2^i for
 * i < log2 n (iteration i multiplies by X^(-2^i) where bit i is set) and the body row rot_t[log2 n * batch + b] = 0 -- and
 * cntt_native_sample_extract_batch(index = 0) returns the LWE ciphertext of entry a.  examples/lookup_native.c does exactly that.
 *
 * Exactness: that of cntt_ext.h.  The difference and the digits are wrapping word arithmetic; the external product is
 * cntt_native_external_product_batch word for word, exact while (k + 1) * levels <= cntt_native_max_terms(plan).  ONE rule for both
 * calls: beyond it call 1 and every tree with M >= 2 return CNTT_EINVAL, the message giving both numbers -- the leaf stage, which sums
 * `levels` terms only, included, so that a tree is accepted or refused whatever its depth.
 *
 * Valid: lut_count a power of two >= 1; base_log >= 1, levels >= 1, base_log * levels <= w; every size the external product accepts.
 * batch == 0 does nothing.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word (a key plane to its residue), a written operand disjoint from
 * every other one.  No call here runs in place.  Workspace, with up(x) = x rounded up to a multiple of 256, H = M / 2, Q = M / 4
 * (integer division, 0 allowed):
 *   cntt_native_glwe_cmux_workspace_bytes = up(batch * (k + 1) * levels * n * wb)                                  (the digit polynomials)
 *   cntt_native_cmux_tree_workspace_bytes = up(max(batch * H * levels, batch * Q * (k + 1) * levels) * n * wb)
 *                                           + up(batch * H * (k + 1) * n * wb) + up(batch * Q * (k + 1) * n * wb)
 *   (the digits of the widest stage and two ciphertext buffers: the stages alternate between them and the last stage writes glwe_out).
 *   16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device path is
 *   one stream-ordered allocation for the whole call.  With a caller workspace the Plan32 kinds at 32 <= n <= 4096 (the fused external
 *   product) make no allocation anywhere in the call, which is then a linear chain of kernels and may be captured into a hipGraph;
 *   elsewhere the external product keeps allocating its own scratch, as cntt_pbs.h says of the blind rotation.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; base_log == 0,
 * levels == 0, base_log * levels > w; lut_count zero or not a power of two; (k + 1) * levels > cntt_native_max_terms(plan) (call 1,
 * and call 2 with M >= 2); a NULL argument or a NULL key plane (ggsw_ntt only when M > 1); a misaligned pointer; a written operand
 * (glwe_out, the workspace) overlapping any other operand (byte ranges); a non-NULL workspace that is misaligned or too small;
 * batch * max(H, 1) * (k + 1) * levels >= 2^32 (H = 1 in call 1: what the widest launch of the external product holds); sizes whose
 * ciphertexts, table, digits or selectors would pass 2^63 bytes (checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  Against the public-call sequence a node saves the stored difference, its read by the decomposition and the copy of c0: three
 * passes over the ciphertexts; the external product, which dominates, is the same.
 * Measured at n = 1024, k = 1, levels 2 and 4 (profiles/r25_native_cmux.txt; tools/native_cmux_bench.py takes the figures), the
 * difference of the sequence taken by torch on the device: on 64-bit words (base_log 22 / 15) the tree at M = 256, batch 64 is 1.08
 * and 1.04 times faster than its public-call sequence, one CMux at batch 4096 1.15 and 1.08 times; on 32-bit words (base_log 12 / 7)
 * the tree is 1.14 and 1.05 times faster, one CMux 1.09 and 1.09 times; no measured shape at which the one-call form loses.  The
 * gain is smaller than mod p (cntt_prime_cmux.h) because the native external product, which both routes share, costs more per word.
 * Other sizes, 128-bit words, the Plan52 and the binary kinds and k > 1 were not measured. */
#ifndef CNTT_CMUX_H
#define CNTT_CMUX_H

#include "cntt_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* glwe0, glwe1, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ggsw_ntt: the residue planes of one selector */
int cntt_native_glwe_cmux_batch(const cntt_native_t *plan, void *glwe_out, const void *glwe0, const void *glwe1, const void *const *ggsw_ntt,
                                size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_native_glwe_cmux_workspace_bytes(const cntt_native_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* lut_in: batch x lut_count polynomials; glwe_out: batch x (k + 1) polynomials; ggsw_ntt: planes of log2 lut_count selectors back to back */
int cntt_native_cmux_tree_batch(const cntt_native_t *plan, void *glwe_out, const void *lut_in, const void *const *ggsw_ntt, size_t lut_count,
                                size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                cntt_mem_t where, void *stream);
size_t cntt_native_cmux_tree_workspace_bytes(const cntt_native_t *plan, size_t lut_count, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the kernel of these calls launches for `polys` output polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest): one per polynomial up to 8 per CU of a 256-CU part; nothing is staged, so neither the size nor the word enters.  The
 * rule is carried over from cntt_prime_cmux_grid: an assumption about what fills the chip, not a measured optimum.  For tests and tools:
 * pure arithmetic, no device call. */
unsigned cntt_native_cmux_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_CMUX_H */
