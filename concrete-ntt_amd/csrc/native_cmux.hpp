// The CMux against a GGSW selector on the native / native_binary plans (include/cntt_cmux.h), one kernel on the walk of
// prime_cmux_diff_kernel (prime_cmux.hpp):
//     native_cmux_diff_kernel   per output polynomial ONE pass over the two sources c0 and c1 that writes the prefilled output c0[q] and the
//                               `levels` digit polynomials of c1[q] - c0[q] mod 2^w.  The difference exists in registers only.
// The external product after it is host code (host_native_cmux.inc) over native_ext_device.  The kernel is instantiated in
// native_cmux.hip; host_native_ext.hip sees the launcher only.
//
// The walk: one 256-thread workgroup per output polynomial, grid-stride; a thread owns 16 bytes of consecutive coefficients (4, 2 or 1
// words) and every load and every store is a coalesced 16-byte one.  Coefficient j of the output needs coefficient j of the two sources
// and nothing else: there is no gather, hence no LDS, and no address depends on a data word.
//
// The two source forms (LEAF).  false: c0 and c1 are GLWE ciphertexts of k + 1 polynomials; output ciphertext c = g h + j (j < h) takes
// ciphertext g gs + j of `c0` and of `c1` (one tree stage of a batch: gs = 2 h and c1 = c0 + h ciphertexts; the public CMux:
// h = gs = 1).  true: the sources are PLAIN polynomials, the table entries, standing for their trivial ciphertexts -- output ciphertext c
// takes polynomial g gs + j of each; the mask workgroups (q < k) store zeros and read nothing, the body workgroup stores lut[j] and the
// `levels` digit polynomials of lut[j + h] - lut[j] at terms[c levels + l - 1]: the zero masks are neither written as sources nor
// decomposed.
//
// The digits are those of native_gadget_kernel (native_gadget.hpp) through the same WordOps and GadgetConst: y = x + off, then per level
// ((y >> sh) & mask) - half, stored as the w-bit two's complement.
#pragma once
#include "native_gadget.hpp"

namespace cntt {

constexpr unsigned NATIVE_CMUX_CUS = 256;   // CUs of the part the grid rule is written for

// Workgroups of the kernel for `polys` output polynomials (the size and the word do not enter: nothing is staged): one per polynomial up
// to 8 per CU, a grid-stride walk beyond.  An ASSUMPTION about what fills the chip, carried over from prime_cmux_grid, not a measured
// optimum.  cntt_native_cmux_grid exports it.
inline unsigned native_cmux_grid(size_t polys, int /*logn*/, size_t /*word_bytes*/) {
    const size_t cap = (size_t)8 * NATIVE_CMUX_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

// terms: nct x (k + 1) * levels polynomials (LEAF: nct x levels); out: nct x (k + 1) polynomials; c0, c1: the sources in the form LEAF
// says (above); nct = the number of output ciphertexts, a multiple of h.  Polynomial (c, q):
//   out[c][q] = c0[q],  terms[c][q levels + l - 1] = d_l(c1[q] - c0[q] mod 2^w)                         (LEAF: q = k only; out[c][q < k] = 0)
// LEAF with terms == nullptr writes the trivial ciphertexts only and does not read c1 (a tree of one entry).
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once (the output keeps the default policy: the external
// product reads it back at once).  G: off, mask, half, base_log and levels are read; the source fields of GadgetConst are not.
template <class W, bool STREAM, bool LEAF>
__global__ __launch_bounds__(256) void native_cmux_diff_kernel(W *__restrict__ terms, W *__restrict__ out, const W *__restrict__ c0,
                                                               const W *__restrict__ c1, const GadgetConst<W> G, uint32_t logn, uint32_t k,
                                                               size_t h, size_t gs, size_t nct) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;   // 16 bytes of any word type
    const uint32_t nvec = 1u << (logn - LOGV);
    const size_t npoly_total = nct * ((size_t)k + 1);
    const bool prefill_only = LEAF && !terms;   // (the same for the whole grid) lut_count = 1: the trivial ciphertext, no digits
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
        W *tbase = terms + (((LEAF ? c : i) * G.levels) << logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            union {
                W w[NV];
                V v;
            } a, b, d;
            a.v = s0[v];
            o[v] = a.v;
            if (prefill_only) continue;
            b.v = s1[v];
            W y[NV];
#pragma unroll
            for (int e = 0; e < NV; ++e) y[e] = O::add(O::sub(b.w[e], a.w[e]), G.off);
            W *dst = tbase + ((size_t)v << LOGV);
            uint32_t sh = (uint32_t)O::BITS;
            for (uint32_t l = 0; l < G.levels; ++l, dst += (size_t)1 << logn) {
                sh -= G.base_log;
#pragma unroll
                for (int e = 0; e < NV; ++e) d.w[e] = O::sub(O::band(O::shr(y[e], sh), G.mask), G.half);
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launcher (native_cmux.hip): word = 4 / 8 / 16 bytes; off = the word gadget_offset gives (host_native_ext.hip), in two halves; stream:
// the STREAM_BYTES policy decided by the caller
hipError_t launch_native_cmux_diff(int word, void *terms, void *out, const void *c0, const void *c1, bool leaf, uint64_t off_lo,
                                   uint64_t off_hi, unsigned base_log, unsigned levels, int logn, size_t glwe_dim, size_t h, size_t gs,
                                   size_t nct, bool stream, hipStream_t st);

}  // namespace cntt
