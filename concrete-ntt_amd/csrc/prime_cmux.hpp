// The CMux against a GGSW selector on the prime plans (include/cntt_prime_cmux.h), one kernel on the walk of prime_ring_merge_kernel:
//     prime_cmux_diff_kernel    per output polynomial ONE pass over the two sources c0 and c1 that writes the prefilled output c0[q] and the
//                               `levels` digit polynomials of c1[q] - c0[q].  The difference exists in registers only.
// The external product after it is host code (host_prime_cmux.inc) over external_product_device.  The kernel is instantiated in
// prime_cmux.hip; host_prime.hip sees the launcher only.
//
// The walk: one 256-thread workgroup per output polynomial, grid-stride; a thread owns 16 bytes of consecutive coefficients and every
// load and every store is a coalesced 16-byte one.  Coefficient j of the output needs coefficient j of the two sources and nothing else:
// there is no gather, hence no LDS.
//
// The two source forms (LEAF).  false: c0 and c1 are GLWE ciphertexts of k + 1 polynomials; output ciphertext c = g h + j (j < h) takes
// ciphertext g gs + j of `c0` and of `c1` (one tree stage of a batch: gs = 2 h and c1 = c0 + h ciphertexts; the public CMux:
// h = gs = 1).  true: the sources are PLAIN polynomials, the table entries, standing for their trivial ciphertexts -- output ciphertext c
// takes polynomial g gs + j of each; the mask workgroups (q < k) store zeros and read nothing, the body workgroup stores lut[j] and the
// `levels` digit polynomials of lut[j + h] - lut[j] at terms[c levels + l - 1]: the zero masks are neither written as sources nor
// decomposed.
//
// The digits are those of prime_gadget_kernel (prime_pbs.hpp) in the form of PrimePackConst (prime_pack.hpp), restated here word for
// word and NOT negated: y = x' + off, the bit `neg`, a shift per level, the top digit unmasked, canonical storage (d >= 0 -> d,
// d < 0 -> p + d).  Words >= p are not reduced; no address depends on a data word.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "prime_pack.hpp"

namespace cntt {

constexpr unsigned CMUX_CUS = 256;   // CUs of the part the grid rule is written for

// Workgroups of the kernel for `polys` output polynomials (the size and the word do not enter: nothing is staged): one per polynomial up
// to 8 per CU, a grid-stride walk beyond.  An ASSUMPTION about what fills the chip, carried over from prime_ring_pack_grid, not a measured
// optimum.  cntt_prime_cmux_grid exports it.
inline unsigned prime_cmux_grid(size_t polys, int /*logn*/, size_t /*word_bytes*/) {
    const size_t cap = (size_t)8 * CMUX_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

// terms: nct x (k + 1) * levels polynomials (LEAF: nct x levels); out: nct x (k + 1) polynomials; c0, c1: the sources in the form LEAF
// says (above); nct = the number of output ciphertexts, a multiple of h.  Polynomial (c, q):
//   out[c][q] = c0[q],  terms[c][q levels + l - 1] = d_l(c1[q] - c0[q]) mod p                           (LEAF: q = k only; out[c][q < k] = 0)
// LEAF with terms == nullptr writes the trivial ciphertexts only and does not read c1 (a tree of one entry).
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once (the output keeps the default policy: the external
// product reads it back at once).
template <class T, bool STREAM, bool LEAF>
__global__ __launch_bounds__(256) void prime_cmux_diff_kernel(T *__restrict__ terms, T *__restrict__ out, const T *__restrict__ c0,
                                                              const T *__restrict__ c1, const PrimePackConst<T> G, uint32_t logn, uint32_t k,
                                                              size_t h, size_t gs, size_t nct) {
    using S = typename std::make_signed<T>::type;
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t n = 1u << logn, nvec = 1u << (logn - LOGV);
    const size_t npoly_total = nct * ((size_t)k + 1);
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t c = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - c * (k + 1u));
        V *o = reinterpret_cast<V *>(out + (i << logn));
        if (LEAF && q != k) {   // (the same for the whole workgroup) a mask of the trivial ciphertext
            const V zero = {0u, 0u, 0u, 0u};
            for (uint32_t v = threadIdx.x; v < nvec; v += 256u) o[v] = zero;
            continue;
        }
        const size_t src = (c / h) * gs + c % h;   // the source ciphertext; LEAF: the source polynomial
        const size_t sp = LEAF ? src : src * ((size_t)k + 1) + q;
        const V *s0 = reinterpret_cast<const V *>(c0 + (sp << logn)), *s1 = reinterpret_cast<const V *>(c1 + (sp << logn));
        T *tbase = terms + (((LEAF ? c : i) * G.levels) << logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            union {
                T w[NV];
                V v;
            } a, b, d;
            const bool prefill_only = LEAF && !terms;   // (the same for the whole grid) lut_count = 1: the trivial ciphertext, no digits
            a.v = s0[v];
            if (!prefill_only) b.v = s1[v];
            o[v] = a.v;
            if (prefill_only) continue;
            T y[NV];
            T *dst = tbase + (v << LOGV);
#pragma unroll
            for (int e = 0; e < NV; ++e) {
                const T x = (T)(b.w[e] - a.w[e] + (b.w[e] < a.w[e] ? G.p : (T)0));
                const bool hi = x >= (T)(G.p - x);
                y[e] = (T)(x + G.off - (hi ? G.p : (T)0));
                const bool neg = hi && (S)y[e] < 0;
                // d_1: the floor of a negative y is the arithmetic shift, stored as p + d_1
                d.w[e] = neg ? (T)(G.p + (T)((S)y[e] >> G.sh1)) : (T)(y[e] >> G.sh1);
            }
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
            else *reinterpret_cast<V *>(dst) = d.v;
            uint32_t sh = G.sh1;
            for (uint32_t l = 1; l < G.levels; ++l) {
                sh -= G.base_log;
                dst += n;
#pragma unroll
                for (int e = 0; e < NV; ++e) {
                    const T f = (T)((y[e] >> sh) & G.mask);   // the digit + B / 2
                    d.w[e] = f >= G.half ? (T)(f - G.half) : (T)(G.p - G.half + f);
                }
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launcher (prime_cmux.hip), T = uint32_t / uint64_t; stream: the STREAM_BYTES policy decided by the caller
template <class T>
hipError_t launch_prime_cmux_diff(T *terms, T *out, const T *c0, const T *c1, bool leaf, const PrimePackConst<T> &G, int logn, size_t glwe_dim,
                                  size_t h, size_t gs, size_t nct, bool stream, hipStream_t st);

}  // namespace cntt
