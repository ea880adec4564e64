/* Part of cntt_ext.h (which includes this file; include that one): rotation, CMux difference and signed gadget decomposition of the
 * native / native_binary plans on the device, and the external product that derives its terms from undecomposed polynomials --
 * together one iteration of a TFHE blind rotation on the torus Z/2^w per call.  No counterpart in the reference (concrete-ntt has
 * no decomposer): the convention below is this library's own, fixed to the last bit so that an integrator can generate matching
 * keys.  Plain C11.
 *
 * w = word width of the plan's kind (32, 64, 128), n = ntt_size, B = 2^base_log.  Valid: base_log >= 1, levels >= 1,
 * base_log * levels <= w.
 *
 * Source polynomial g of an input polynomial f (n words) and an exponent a < 2n (one per batch element, rot[b], shared by the
 * element's npolys polynomials; rot lives where the polynomials live; a >= 2n is CNTT_EINVAL on the host path, the device path
 * takes a mod 2n):
 *   CNTT_SRC_PLAIN   g = f                       (rot may be NULL and is not read)
 *   CNTT_SRC_ROTATE  g = X^a f  in Z/2^w[X]/(X^n + 1): for a < n, g[i] = f[i - a] if i >= a else -f[i - a + n]; for a >= n the
 *                    negation of the result for a - n.  Negation is mod 2^w.
 *   CNTT_SRC_CMUX    g = X^a f - f  mod 2^w
 *
 * Digits of a word x: s = w - base_log * levels; r = ((x + 2^(s-1)) mod 2^w) >> s (r = x when s = 0), a (base_log * levels)-bit
 * number: the closest multiple of 2^s, ties up, wrapping at the top.  The digits d_1 .. d_levels (d_1 most significant) are the
 * unique ones with d_l in [-B/2, B/2) and sum_l d_l B^(levels - l) = r (mod B^levels).  From the low level up: d = state mod B,
 * state >>= base_log, and if d >= B/2 then d -= B, state += 1; the carry out of level 1 is dropped.  Digits are stored as w-bit
 * words in two's complement, which is what cntt_native_external_product_batch expects of `terms`.
 *
 * Term order: term j = p * levels + (l - 1) is level l of polynomial p, so key row j belongs to the gadget factor
 * 2^(w - base_log * l) of polynomial p. */
#ifndef CNTT_GADGET_H
#define CNTT_GADGET_H

#include "cntt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cntt_src_mode { CNTT_SRC_PLAIN = 0, CNTT_SRC_ROTATE = 1, CNTT_SRC_CMUX = 2 } cntt_src_mode_t;

/* terms[b][p * levels + l - 1] = level l of the digits of src_mode(polys[b][p], rot[b]);  batch x npolys polynomials in,
 * batch x npolys * levels out.  Every kind, every size.  CNTT_EINVAL (terms untouched, cntt_last_error names the argument) for
 * base_log == 0, levels == 0, base_log * levels > w, an unknown mode, rot == NULL with a mode that reads it, or terms overlapping
 * polys (byte ranges).  batch == 0 or npolys == 0 does nothing.  where / stream as every other _batch call. */
int cntt_native_gadget_decompose_batch(const cntt_native_t *plan, void *terms, const void *polys, const uint32_t *rot,
                                       size_t npolys, unsigned base_log, unsigned levels, cntt_src_mode_t src_mode,
                                       size_t batch, cntt_mem_t where, void *stream);

/* out[b][o] = (addend ? addend[b][o] : 0) + sum_{p,l} digit_l(src_mode(polys[b][p], rot[b])) (*) key[p * levels + l - 1][o]  mod 2^w
 * The same words, bit for bit, as cntt_native_gadget_decompose_batch followed by cntt_native_external_product_batch on its
 * output with nterms = npolys * levels, and a word-wise add of addend.  key_ntt as for that call.
 * addend: NULL, or batch x nout polynomials; it may be `out` itself (accumulate in place) or `polys` (then nout == npolys: the
 * blind-rotation update acc' = acc + ExtProd(key, X^a acc - acc) from buffer `polys` into buffer `out`); otherwise it must not
 * overlap out.  out must not overlap polys: the call goes over the outputs in launches of two, and every launch reads all of
 * polys -- which is also why addend is a pointer and not a flag.
 * CNTT_EINVAL (out untouched) for the cases of the decomposition, for npolys * levels > cntt_native_max_terms(plan) (the digits
 * counted as full words: far from tight for small digits), for out overlapping polys, and for an addend that overlaps out
 * without being out.  npolys == 0 is the empty sum (out = addend, or zero); batch == 0 or nout == 0 does nothing.
 * Device path: the digits go into a stream-ordered scratch allocation (hipMallocAsync) and cntt_native_external_product_batch
 * runs on them.  With the testing switch "native_gadget" = 1 (default 0) the 32- and 64-bit Plan32 kinds at 32 <= n <= 4096 with
 * base_log <= 31 run one fused kernel per two outputs instead, which derives rotation, difference and digits while loading -- no
 * workspace, may be captured into a hipGraph -- but measured 0.66 ... 0.98 x the speed of the composed path on every shape tried
 * (profiles/r07_native_gadget_ab.txt), hence off by default. */
int cntt_native_external_product_decomposed_batch(const cntt_native_t *plan, void *out, const void *polys,
                                                  const uint32_t *rot, const void *addend, const void *const *key_ntt,
                                                  size_t npolys, unsigned base_log, unsigned levels,
                                                  cntt_src_mode_t src_mode, size_t nout, size_t batch,
                                                  cntt_mem_t where, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CNTT_GADGET_H */
