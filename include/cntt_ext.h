/* Device extensions of the C ABI with no counterpart in the reference (concrete-ntt has no batched external product for its
 * native plans).  Plain C11; the 87 entry points of cntt.h -- the reference's surface, which rust/src/ffi.rs is generated from --
 * stay as they are, so the Rust binding does not cover what is declared here. */
#ifndef CNTT_EXT_H
#define CNTT_EXT_H

#include "cntt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------- */
/* External product of the native / native_binary plans (the tfhe-rs external-product      */
/* step on the torus Z/2^w): the key is given once, forward-transformed, and shared by the */
/* whole batch.                                                                            */
/* ------------------------------------------------------------------------------------- */
/* out[b][o] = sum_{j<nterms} terms[b][j] (*) key[j][o]   in Z/2^w[X]/(X^n+1)   (accumulate == 0)
 * out[b][o] = out[b][o] + that  mod 2^w                                      (accumulate != 0)
 * (*) is negacyclic_polymul, w the word width of the kind (32, 64 or 128).
 * terms:      batch x nterms coefficient polynomials (u32 / u64 / u128 words of the kind), element b's terms back to back
 * key_ntt:    nprimes pointers; plane i = nterms*nout residue polynomials, key[j][o] at index j*nout + o, exactly what
 *             cntt_native_fwd_batch (cntt_native_fwd_binary_batch for the binary kinds: the key is the binary operand)
 *             writes for a batch of nterms*nout key polynomials -- unnormalised, bit-reversed, as the reference leaves them
 * out:        batch x nout polynomials.  Same words as nterms*nout calls of negacyclic_polymul summed mod 2^w.
 * CNTT_EINVAL when nterms > cntt_native_max_terms(plan) (out untouched); nterms == 0 is the empty sum (out zeroed, or left
 * as it is when accumulating); batch == 0 or nout == 0 does nothing.
 * where / stream follow the other _batch calls (CNTT_MEM_HOST: host buffers, synchronous; CNTT_MEM_DEVICE: device buffers,
 * enqueued on `stream`).  Device path: the Plan32 kinds at 32 <= n <= 4096 run one fused kernel per two outputs (one per
 * output for the 128-bit kinds) with no workspace, and may be captured into a hipGraph.  Other sizes, the Plan52 kinds and
 * the testing switch "native_ext" = 0 compose residue split, one mul_accumulate chain per prime and one CRT through a
 * stream-ordered scratch allocation (hipMallocAsync).
 *
 * Exactness bound.  With A = 2^w - 1, a sum of T products of size n has integer coefficients in (-T n A^2, T n A^2]
 * (T n A for the binary kinds, whose key words are 0 / 1).  The result is exact while that bound D T stays inside the range the
 * kind's reconstruction maps back exactly.  With M the product of the kind's primes and Mt its top mixed-radix digit
 * (the last prime, or the last prime pair of native64 / native128 / native_binary128 Plan32):
 *   every kind (the reference's sign rule on the top digit):      D T <= (M - M / Mt) / 2   and   D T <= (M + M / Mt) / 2 - 1
 *   Plan32 kinds also (accumulating CRT: k primes each add < 1.5 units of 2^-27 to the rounded fraction sum):
 *                                                                 D T <= (M - 1) / 2   and   D T <= floor(M (2^27 - 3 k) / 2^28)
 * cntt_native_max_terms() is the largest such T (exact big-integer arithmetic on the host), but at least 1: nterms == 1 is
 * the plan's own negacyclic_polymul at every n.  E.g. native64 Plan32: 1964 at n = 1024, 61 at n = 32768. */
int cntt_native_external_product_batch(const cntt_native_t *plan, void *out, const void *terms,
                                       const void *const *key_ntt, size_t nterms, size_t nout, size_t batch,
                                       int accumulate, cntt_mem_t where, void *stream);
/* largest nterms for which every accumulated coefficient stays inside the kind's exact CRT range (>= 1); 0 for a NULL plan */
size_t cntt_native_max_terms(const cntt_native_t *plan);

#ifdef __cplusplus
}
#endif

/* Rotation / CMux difference / signed gadget decomposition (cntt_src_mode_t, cntt_native_gadget_decompose_batch) and the external
 * product on undecomposed polynomials (cntt_native_external_product_decomposed_batch) are declared here through a file of their own,
 * which carries their semantics. */
#include "cntt_gadget.h"

/* The programmable bootstrap built on them -- LWE modulus switch, blind rotation in place, sample extraction, and all of it in one
 * call -- is declared the same way, through a file of its own that carries the conventions. */
#include "cntt_pbs.h"

/* The LWE keyswitch that takes a bootstrap's output back to the dimension the next one takes, and keyswitch + bootstrap in one call
 * that chains with itself, likewise. */
#include "cntt_keyswitch.h"

/* The packing keyswitch that takes LWE ciphertexts back into one GLWE ciphertext, through the NTT, likewise. */
#include "cntt_pack.h"

#endif /* CNTT_EXT_H */
