/* The ring automorphism X -> X^t of the prime32 / prime64 plans on the device, in the coefficient and in the NTT domain, the Galois
 * keyswitch of a GLWE ciphertext built on it, and the homomorphic trace built on that -- the RLWE-side primitive next to the LWE-side
 * calls of cntt_prime_pbs.h, cntt_prime_keyswitch.h and cntt_prime_pack.h.  No counterpart in the reference; the convention below is
 * this library's own, fixed to the last bit so that an integrator can generate matching keys.  No key or noise generation: the caller
 * brings the keys.  Include this file on its own (it includes cntt_prime_pbs.h); it is not part of cntt.h or cntt_ext.h.  Plain C11.
 *
 * Symbols: T = the plan's word (uint32_t / uint64_t), p = the modulus, W = the bit length of p, n = ntt_size, k = glwe_dim,
 * B = 2^base_log.  A GLWE ciphertext is its k mask polynomials with the body polynomial last, as in cntt_prime_pbs.h.  t is always an
 * odd exponent with 1 <= t < 2n.  sigma_t is the ring automorphism f(X) -> f(X^t) of Z_p[X]/(X^n + 1): it sends X^i to
 * (-1)^floor(i t / n) X^(i t mod n).  sigma_s sigma_t = sigma_(s t mod 2n), sigma_1 is the identity and sigma_(2n-1) is X -> X^-1.
 *
 * 1. automorphism_batch: out = sigma_t(in) on coefficient-domain polynomials.  In gather form, with tinv = t^-1 mod 2n and
 *    u = j tinv mod 2n:   out[j] = in[u mod n], negated mod p (0 stays 0) iff u >= n.
 *
 * 2. automorphism_ntt_batch: the same map on NTT-domain polynomials, where it is a pure permutation with no sign and no arithmetic.
 *    Slot c of a forward transform holds the evaluation at psi^(2 bitrev(c) + 1), bitrev reversing log2 n bits (the order
 *    cntt_prime_multibit.h documents), so
 *      out_ntt[c] = in_ntt[c']   with   2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n.
 *    fwd(sigma_t f) = automorphism_ntt(fwd f) word for word; the permutation does not look at the words, so it holds for normalised
 *    (n^-1 fwd) and unnormalised words alike -- it rotates NTT-domain keys and ciphertexts a caller keeps transformed.
 *
 * 3. glwe_automorphism_keyswitch_batch (the Galois keyswitch).  For q <= k, mod p:
 *      out[b][q] = [q == k] sigma_t(in[b][k]) + [add_input] in[b][q]
 *                  - sum_{r < k} sum_{l = 1 .. levels} d_l(sigma_t(in[b][r])) (*) AK[r * levels + l - 1][q]
 *    d_1 .. d_levels are exactly the CNTT_SRC_PLAIN digits of cntt_prime_pbs.h, taken from the PERMUTED polynomial: from the balanced
 *    lift, rounded to 2^(W - base_log * levels), d_1 most significant and unmasked.  (*) is the negacyclic product.  Every output word
 *    is canonical (< p).
 *    Key layout.  ak_ntt is ONE array of k * levels * (k + 1) NTT-domain polynomials, AK[j][q] at index j * (k + 1) + q, holding
 *    n^-1 * fwd(key polynomial): exactly what one cntt_prime*_fwd_batch followed by one cntt_prime*_normalize_batch over all key
 *    polynomials in that order writes -- the convention of bsk_ntt in cntt_prime_pbs.h and of pksk_ntt in cntt_prime_pack.h.  Row
 *    j = r * levels + (l - 1) is a GLWE encryption under S (k mask polynomials, body last) of the polynomial
 *    sigma_t(S_r) * 2^(W - base_log * l) mod p.
 *    Phase.  With phase(c) = body - sum_r mask_r (*) S_r and a noise-free key, phase(out) = sigma_t(phase(in)) (+ phase(in) with
 *    add_input), up to the decomposition's rounding: with s = W - base_log * levels and a binary key every coefficient of
 *    phase(out) - sigma_t(phase(in)) lies within k * n * 2^(s-1), and the difference is 0 when s = 0.
 *    The words are exactly those of this sequence of public calls: glwe_out starts as the prefill -- the mask polynomials in[b][q]
 *    with add_input and 0 without, the body sigma_t(in[b][k]), plus in[b][k] mod p with add_input --; automorphism_batch on the k mask
 *    polynomials; cntt_prime*_gadget_decompose_batch(CNTT_SRC_PLAIN, npolys = k); every digit negated mod p, with 0 staying 0;
 *    cntt_prime*_external_product_batch(glwe_out, those terms, ak_ntt, nterms = k * levels, nout = k + 1, accumulate = 1).
 *    k == 0 writes sigma_t(body) (+ body) only; ak_ntt may then be NULL.
 *
 * 4. glwe_trace_batch.  0 <= steps <= log2 n.  cur starts as glwe_in; for r = 0 .. steps - 1: cur <- cur + AutoKS_(t_r)(cur) with
 *    t_r = n / 2^r + 1, which is call 3 with add_input = 1; key r sits at polynomial r * k * levels * (k + 1) of ak_ntt (steps keys of
 *    the layout above, back to back).  The words are exactly those of `steps` calls of 3; steps == 0 copies.  With noise-free keys
 *    coefficient i of the phase becomes 2^steps * phase[i] when 2^steps divides i and 0 otherwise: steps = log2 n leaves n times the
 *    constant coefficient.  Modulo a prime 2^steps is a unit, where modulo 2^64 the same factor would have destroyed message bits:
 *    the caller removes it by scaling with the inverse of 2^steps mod p.  With noisy keys scale the INPUT ciphertext, every word
 *    times that inverse, before the call -- the trace is linear in the phase, so the surviving coefficients come out unscaled with
 *    the keyswitch noise on top; scaling the output instead multiplies that noise by the inverse too, which is not a small number.
 *
 * Exactness.  The permutation, the decomposition and the prefill are exact integer arithmetic for every prime the plans accept.  The
 * external product is cntt_prime*_external_product_batch word for word, so the "Exactness" caveat of cntt_prime_pbs.h applies: for
 * primes of the reference's strict range (2^62 <= p < 2^63 on 64-bit words, 2^30 <= p < 2^31 on 32-bit words) it is the reference's
 * composition fwd / mul_accumulate / inv with its wrapping Barrett product.  Calls 3 and 4 therefore equal the public-call sequences
 * above for EVERY prime, and equal the big-integer formulas only outside that caveat.
 *
 * Valid: t odd and below 2n; base_log >= 1, levels >= 1, base_log * levels <= W; steps <= log2 n; every size the external product
 * accepts.  batch == 0 (and npolys == 0 in calls 1 and 2) does nothing.  Input or key words >= p are not rejected and not reduced:
 * the call completes without a fault and the affected outputs are unspecified.
 *
 * Operands: the rules of cntt.h -- every pointer aligned to its word, a written operand disjoint from every other one.  No call here
 * runs in place: out may not overlap in, glwe_out may not overlap glwe_in.
 * Workspace, with up(x) = x rounded up to a multiple of 256:
 *   cntt_prime*_glwe_automorphism_keyswitch_workspace_bytes = up(batch * k * levels * n * sizeof(T))      (the negated digit polynomials)
 *   cntt_prime*_glwe_trace_workspace_bytes                  = that + up(batch * (k + 1) * n * sizeof(T))  (and the second ciphertext the
 *                                                             steps alternate with, so that the last one lands in glwe_out)
 * The rules are those of cntt_prime_pbs.h: 16-byte aligned, living where the other buffers live; NULL on the device path is one
 * stream-ordered allocation for the whole call.  With a caller workspace the shapes of the fused chain (n <= 2048 on 64-bit words,
 * n <= 4096 on 32-bit words, k + 1 <= 4) make no allocation anywhere in the call, which is then a linear chain of kernels and may be
 * captured into a hipGraph; elsewhere the composed external product keeps its own per-call scratch.
 * CNTT_EINVAL (outputs untouched, cntt_last_error names the argument, refused before any device call) for a NULL plan, t even or
 * t >= 2n, steps > log2 n, base_log == 0, levels == 0, base_log * levels > W, a NULL argument (ak_ntt only when k > 0, and in the trace
 * only when steps > 0 as well), a misaligned pointer, a written operand (out, glwe_out, the workspace) overlapping any other operand
 * (byte ranges), a non-NULL workspace that is misaligned or too small, batch * max(k * levels, k + 1) >= 2^32 (what one launch of the
 * external product holds), and sizes whose polynomials, digits or keys would pass 2^63 bytes (checked before they are formed).
 * where / stream as every other _batch call: CNTT_MEM_HOST copies in, runs the device path, copies out and synchronises.
 *
 * Cost.  A full trace needs log2 n * k * levels * (k + 1) key polynomials where the packing key of cntt_prime_pack.h at Lin = k n needs
 * k n * levels * (k + 1); measured times of calls 3 and 4 against their public-call sequences, and of the kernels' two gather forms:
 * profiles/r19_prime_automorphism.txt (tools/prime_automorphism_bench.py takes the figures). */
#ifndef CNTT_PRIME_AUTOMORPHISM_H
#define CNTT_PRIME_AUTOMORPHISM_H

#include "cntt_prime_pbs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- prime64 ------------------------------------------------------------------------------------------------------------------ */

/* in, out: batch * npolys polynomials; out is only written */
int cntt_prime64_automorphism_batch(const cntt_plan64_t *plan, uint64_t *out, const uint64_t *in, size_t t, size_t npolys, size_t batch,
                                    cntt_mem_t where, void *stream);
int cntt_prime64_automorphism_ntt_batch(const cntt_plan64_t *plan, uint64_t *out_ntt, const uint64_t *in_ntt, size_t t, size_t npolys,
                                        size_t batch, cntt_mem_t where, void *stream);

/* glwe_in, glwe_out: batch x (k + 1) polynomials, glwe_out only written; ak_ntt: k * levels * (k + 1) polynomials as above */
int cntt_prime64_glwe_automorphism_keyswitch_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *glwe_in,
                                                   const uint64_t *ak_ntt, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,
                                                   int add_input, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                                   void *stream);
/* the formula above; 0 for a NULL plan */
size_t cntt_prime64_glwe_automorphism_keyswitch_workspace_bytes(const cntt_plan64_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* ak_ntt: steps * k * levels * (k + 1) polynomials, the key of t_r = n / 2^r + 1 at polynomial r * k * levels * (k + 1) */
int cntt_prime64_glwe_trace_batch(const cntt_plan64_t *plan, uint64_t *glwe_out, const uint64_t *glwe_in, const uint64_t *ak_ntt,
                                  unsigned steps, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                  size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime64_glwe_trace_workspace_bytes(const cntt_plan64_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* ---- prime32: the same six calls on 32-bit words ---------------------------------------------------------------------------------- */
int cntt_prime32_automorphism_batch(const cntt_plan32_t *plan, uint32_t *out, const uint32_t *in, size_t t, size_t npolys, size_t batch,
                                    cntt_mem_t where, void *stream);
int cntt_prime32_automorphism_ntt_batch(const cntt_plan32_t *plan, uint32_t *out_ntt, const uint32_t *in_ntt, size_t t, size_t npolys,
                                        size_t batch, cntt_mem_t where, void *stream);
int cntt_prime32_glwe_automorphism_keyswitch_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *glwe_in,
                                                   const uint32_t *ak_ntt, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,
                                                   int add_input, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                                   void *stream);
size_t cntt_prime32_glwe_automorphism_keyswitch_workspace_bytes(const cntt_plan32_t *plan, size_t glwe_dim, unsigned levels, size_t batch);
int cntt_prime32_glwe_trace_batch(const cntt_plan32_t *plan, uint32_t *glwe_out, const uint32_t *glwe_in, const uint32_t *ak_ntt,
                                  unsigned steps, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                  size_t workspace_bytes, cntt_mem_t where, void *stream);
size_t cntt_prime32_glwe_trace_workspace_bytes(const cntt_plan32_t *plan, size_t glwe_dim, unsigned levels, size_t batch);

/* Workgroups the three kernels of these calls launch for `polys` polynomials of 2^logn words of word_bytes bytes (a grid-stride walk
 * serves the rest).  For tests and tools, like cntt_prime_multibit_grid: pure arithmetic, no device call. */
unsigned cntt_prime_automorphism_grid(size_t polys, int logn, size_t word_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_PRIME_AUTOMORPHISM_H */
