/* The ring automorphism X -> X^t of the native plans (ciphertext modulus 2^32 / 2^64 / 2^128) on the device, on coefficient words and
 * on residue planes, the Galois keyswitch of a GLWE ciphertext built on it, and the homomorphic trace built on that -- the RLWE-side
 * primitive next to the LWE-side calls of cntt_pbs.h, cntt_keyswitch.h and cntt_pack.h.  The counterpart mod p is
 * cntt_prime_automorphism.h, which this file mirrors call for call.  No counterpart in the reference; the convention below is this
 * library's own, fixed to the last bit so that an integrator can generate matching keys.  No key or noise generation: the caller brings
 * the keys.  Include this file on its own (it includes cntt_ext.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols are those of cntt_cmux.h: w = the word width of the plan's kind, wb = w / 8 = cntt_native_word_bytes, n = ntt_size,
 * k = glwe_dim, B = 2^base_log, s = w - base_log * levels, a GLWE ciphertext = its k mask polynomials with the body polynomial last,
 * every word little-endian (a 128-bit word: 16 bytes, low half first).  t is always an odd exponent with 1 <= t < 2n.  sigma_t is the
 * ring automorphism f(X) -> f(X^t) of Z/2^w[X]/(X^n + 1): it sends X^i to (-1)^floor(i t / n) X^(i t mod n).
 * sigma_s sigma_t = sigma_(s t mod 2n), sigma_1 is the identity and sigma_(2n-1) is X -> X^-1.
 *
 * 1. cntt_native_automorphism_batch: out = sigma_t(in) on coefficient-domain polynomials, every kind.  In gather form, with
 *    tinv = t^-1 mod 2n and u = j tinv mod 2n:   out[j] = in[u mod n], negated mod 2^w iff u >= n.
 *
 * 2. cntt_native_automorphism_ntt_batch: the same map on residue planes, where it is a pure permutation with no sign and no arithmetic.
 *    in_planes and out_planes are cntt_native_nprimes pointers; each plane holds batch * npolys residue polynomials of
 *    cntt_native_residue_bytes words.  Slot c of a forward transform holds the evaluation at psi^(2 bitrev(c) + 1), bitrev reversing
 *    log2 n bits (the order cntt_multibit.h documents for the Plan32 kinds; tests/test_native_automorphism_model.py checks it against the
 *    CPU oracle for the Plan52 kinds too, and it holds there), so in every plane
 *      out[c] = in[c']   with   2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n.
 *    The permutation does not look at the words: one kernel on 4-byte and 8-byte words serves every kind.
 *    What it means.  Plane i of cntt_native_fwd_batch(f) is the forward transform mod P_i of the words of f read as unsigned integers.
 *    Call 2 on those planes gives, plane for plane and word for word, the forward transform of sigma_t applied to that INTEGER polynomial,
 *    the sign taken mod P_i.  So cntt_native_fwd_batch(sigma_t f) equals call 2 on cntt_native_fwd_batch(f) word for word wherever
 *    sigma_t negates no non-zero word (t = 1; polynomials whose negated coefficients are zero), and in general the two differ by the
 *    planes of 2^w times a 0 / 1 polynomial: -x mod 2^w is 2^w - x, not -x.  Both stand for the same polynomial mod 2^w:
 *    cntt_native_inv_batch of either returns sigma_t(f), and as the key of an external product either gives the same words, as long as
 *    the sum stays in the exact range (cntt_native_max_terms counts unsigned words of either sign).  This is what rotates a key a caller
 *    keeps transformed.
 *
 * 3. cntt_native_glwe_automorphism_keyswitch_batch (the Galois keyswitch), the five non-binary kinds.  For q <= k, mod 2^w:
 *      out[b][q] = [q == k] sigma_t(in[b][k]) + [add_input] in[b][q]
 *                  - sum_{r < k} sum_{l = 1 .. levels} d_l(sigma_t(in[b][r])) (*) AK[r * levels + l - 1][q]
 *    d_1 .. d_levels are exactly the CNTT_SRC_PLAIN digits of cntt_gadget.h, taken from the PERMUTED polynomial: rounded to 2^s, in
 *    [-B/2, B/2), d_1 most significant.  (*) is the negacyclic product.
 *    Key layout.  ak_ntt is cntt_native_nprimes residue planes, each of k * levels * (k + 1) residue polynomials, AK[j][q] at index
 *    j * (k + 1) + q, unnormalised and bit-reversed: exactly what one cntt_native_fwd_batch over all key polynomials in that order
 *    writes -- the convention of bsk_ntt in cntt_pbs.h and of pksk_ntt in cntt_pack.h.  Row j = r * levels + (l - 1) is a GLWE
 *    encryption under S (k mask polynomials, body last) of the polynomial sigma_t(S_r) * 2^(w - base_log * l) mod 2^w.
 *    Phase.  With phase(c) = body - sum_r mask_r (*) S_r and a noise-free key, phase(out) = sigma_t(phase(in)) (+ phase(in) with
 *    add_input), up to the decomposition's rounding: with a binary key every coefficient of phase(out) - sigma_t(phase(in)) lies within
 *    k * n * 2^(s-1), and the difference is 0 when s = 0.
 *    The words are DEFINED as those of this sequence of public calls: glwe_out starts as the prefill -- the mask polynomials in[b][q]
 *    with add_input and 0 without, the body sigma_t(in[b][k]), plus in[b][k] mod 2^w with add_input --; cntt_native_automorphism_batch on
 *    the k mask polynomials; cntt_native_gadget_decompose_batch(CNTT_SRC_PLAIN, npolys = k); every digit word negated mod 2^w;
 *    cntt_native_external_product_batch(glwe_out, those terms, ak_ntt, nterms = k * levels, nout = k + 1, accumulate = 1).
 *    One kernel reads the input once and writes the prefill and the negated digits; the permuted polynomials and the un-negated digits
 *    are never stored.  k == 0 writes sigma_t(body) (+ body) only; ak_ntt may then be NULL.
 *    The binary kinds are refused, as cntt_cbs.h refuses them: a keyswitching key is never binary, and the exactness bound of those
 *    kinds assumes a 0 / 1 key.
 *
 * 4. cntt_native_glwe_trace_batch.  0 <= steps <= log2 n.  cur starts as glwe_in; for r = 0 .. steps - 1: cur <- cur + AutoKS_(t_r)(cur)
 *    with t_r = n / 2^r + 1, which is call 3 with add_input = 1; key r sits at residue polynomial r * k * levels * (k + 1) of every plane
 *    (steps keys of the layout above, back to back).  The words are exactly those of `steps` calls of 3; the stages alternate between
 *    glwe_out and a second ciphertext in the workspace so that the last one lands in glwe_out; steps == 0 copies.  With noise-free keys
 *    and s = 0, coefficient i of the phase becomes 2^steps * phase[i] mod 2^w when 2^steps divides i and 0 otherwise: steps = log2 n
 *    leaves n times the constant coefficient.
 *    WHAT DIFFERS FROM THE PRIME PLANS.  Modulo a prime 2^steps is a unit and the caller scales it away.  2^steps is NOT a unit mod 2^w:
 *    the surviving coefficients come out as 2^steps * phase[i] mod 2^w, and the top `steps` bits of phase[i] are gone for good.  The
 *    caller therefore encodes with `steps` bits of headroom BELOW the message -- a message of m bits sits at bit w - steps - m, not at
 *    bit w - m -- so that the factor moves it to the top of the word; the noise of the input grows by the same factor 2^steps, and the
 *    noise of keyswitch r by 2^(steps - 1 - r).  examples/trace_native.c decodes that way.
 *
 * Exactness: that of cntt_ext.h.  The permutation, the digits and the prefill are wrapping word arithmetic; the external product is
 * cntt_native_external_product_batch word for word, exact while k * levels <= cntt_native_max_terms(plan).  Beyond it calls 3 and 4
 * return CNTT_EINVAL, the message giving both numbers.
 *
 * Valid: t odd and below 2n; base_log >= 1, levels >= 1, base_log * levels <= w; steps <= log2 n; every size the external product
 * accepts.  batch == 0 (and npolys == 0 in calls 1 and 2) does nothing.
 *
 * Operands: the rules of cntt.h and cntt_cmux.h -- every pointer aligned to its word (a plane to its residue), a written operand
 * disjoint from every other one.  No call here runs in place: out may not overlap in, no out plane any other plane, glwe_out may not
 * overlap glwe_in.
 * Workspace, with up(x) = x rounded up to a multiple of 256:
 *   cntt_native_glwe_automorphism_keyswitch_workspace_bytes = up(batch * k * levels * n * wb)           (the negated digit polynomials)
 *   cntt_native_glwe_trace_workspace_bytes                  = that + up(batch * (k + 1) * n * wb)       (and the second ciphertext)
 *   16-byte aligned, living where the other buffers live; on the host path it is checked and then not used.  NULL on the device path is
 *   one stream-ordered allocation for the whole call.  With a caller workspace the Plan32 kinds at 32 <= n <= 4096 (the fused external
 *   product) make no allocation anywhere in the call, which is then a linear chain of kernels and may be captured into a hipGraph;
 *   elsewhere the external product keeps allocating its own scratch.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan; t even or
 * t >= 2n; steps > log2 n; base_log == 0, levels == 0, base_log * levels > w; a binary kind (calls 3 and 4);
 * k * levels > cntt_native_max_terms(plan); a NULL argument or a NULL plane (ak_ntt only when k > 0, and in the trace only when
 * steps > 0 as well); a misaligned pointer; a written operand (out, an out plane, glwe_out, the workspace) overlapping any other operand
 * (byte ranges); a non-NULL workspace that is misaligned or too small; batch * max(k * levels, k + 1) >= 2^32 (what one launch of the
 * external product holds); sizes whose polynomials, digits or keys would pass 2^63 bytes (checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  A full trace needs log2 n * k * levels * (k + 1) key polynomials where the packing key of cntt_pack.h at Lin = k n needs
 * k n * levels * (k + 1): n / log2 n times fewer (102 times at n = 1024, 186 times at n = 2048).  Against its public-call sequence
 * call 3 saves the stored permuted masks, their read by the decomposition, the pass that negates the digits and the prefill passes;
 * the external product, which dominates, is the same.
 * Measured at k = 1, n = 1024 / 2048, levels 2 / 4, batch 1 / 256 / 4096 (profiles/r27_native_automorphism.txt;
 * tools/native_automorphism_bench.py takes the figures; one box, one run, the prefill and the negation of the sequence taken by torch on
 * the device): call 3 is 1.14 to 1.55 times faster than its public-call sequence on 64-bit words and 1.18 to 2.03 times on 32-bit
 * words, most at small batches and two levels, least at four levels; no measured shape at which the one-call form loses.  Call 4 takes
 * the time of its log2 n calls of 3 (1.00 to 1.01): it saves the caller the buffers and the key offsets, not time.  Staging through LDS
 * against the global gather: 0.99 to 1.01, no difference at these sizes; the shared default stays.  One
 * cntt_native_pack_keyswitch_batch at Lin = k n, lwe_count = n takes 47 to 147 times as long as one full trace (a different job: n LWE
 * ciphertexts in; the figure sizes what ring packing on these keys has to beat).  128-bit words, the Plan52 kinds and k > 1 were not
 * measured. */
#ifndef CNTT_AUTOMORPHISM_H
#define CNTT_AUTOMORPHISM_H

#include "cntt_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* in, out: batch * npolys polynomials; out is only written */
int cntt_native_automorphism_batch(const cntt_native_t *plan, void *out, const void *in, size_t t, size_t npolys, size_t batch,
                                   cntt_mem_t where, void *stream);
/* in_planes, out_planes: cntt_native_nprimes planes of batch * npolys residue polynomials each; the out planes are only written */
int cntt_native_automorphism_ntt_batch(const cntt_native_t *plan, void *const *out_planes, const void *const *in_planes, size_t t,
                                       size_t npolys, size_t batch, cntt_mem_t where, void *stream);

/* glwe_in, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ak_ntt: planes of k * levels * (k + 1) residue polynomials */
int cntt_native_glwe_automorphism_keyswitch_batch(const cntt_native_t *plan, void *glwe_out, const void *glwe_in, const void *const *ak_ntt,
                                                  size_t t, size_t glwe_dim, unsigned base_log, unsigned levels, int add_input, size_t batch,
                                                  void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_native_glwe_automorphism_keyswitch_workspace_bytes(const cntt_native_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* ak_ntt: planes of steps * k * levels * (k + 1) residue polynomials, the key of t_r = n / 2^r + 1 at polynomial r * k * levels * (k + 1) */
int cntt_native_glwe_trace_batch(const cntt_native_t *plan, void *glwe_out, const void *glwe_in, const void *const *ak_ntt, unsigned steps,
                                 size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                 cntt_mem_t where, void *stream);
size_t cntt_native_glwe_trace_workspace_bytes(const cntt_native_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the three kernels of these calls launch for `polys` polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest): one per polynomial up to 8 per CU of a 256-CU part, fewer where the polynomial staged through LDS (up to 64 KiB)
 * limits residency at 160 KiB of LDS per CU.  The rule of cntt_prime_automorphism_grid: an assumption about what fills the chip, not a
 * measured optimum.  For tests and tools: pure arithmetic, no device call. */
unsigned cntt_native_automorphism_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_AUTOMORPHISM_H */
