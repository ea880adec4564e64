// Rotation, CMux difference and signed gadget decomposition of the native / native_binary plans (include/cntt_gadget.h):
//     g      = f,  X^a f  or  X^a f - f                      in Z/2^w[X]/(X^n + 1)          (source modes PLAIN, ROTATE, CMUX)
//     digits = the `levels` signed digits of base_log bits of every coefficient of g        (d_1 most significant, in [-B/2, B/2))
// as a stand-alone batched kernel (native_gadget_kernel: polys read once, `levels` term polynomials written) and as the operand load
// of the fused external product (native_ext_gadget_kernel: the body of native_ext_kernel, native_ext_body.inc, with the term load
// replaced, so the digits never exist in memory).
//
// The digits without a carry chain: with s = w - base_log levels, B = 2^base_log and K = sum_l (B/2) B^(levels-l), the word
//     y = x + 2^(s-1) + K 2^s   (mod 2^w)                      [s = 0: no rounding term]
// holds digit l, offset by B/2, in its bits [w - base_log l, w - base_log (l-1)):  d_l = ((y >> (w - base_log l)) & (B-1)) - B/2.
// (Adding B/2 at every level turns "d >= B/2: d -= B, carry 1" of the sequential rule into the plain carries of one addition.)
// The host passes `off` = 2^(s-1) + K 2^s (GadgetCall, ntt_launch.hpp).
//
// The rotation is a gather: destination coefficient i of X^a f is f[(i - a) mod n], negated when bit log2 n of (i - a) mod 2n is set.
#pragma once
#include "native_ext.hpp"

namespace cntt {

// w-bit word arithmetic for u32 / u64 / Word128 (shift counts below the word width)
template <class W> struct WordOps {
    static constexpr int BITS = sizeof(W) * 8;
    static __device__ __forceinline__ W add(W a, W b) { return a + b; }
    static __device__ __forceinline__ W sub(W a, W b) { return a - b; }
    static __device__ __forceinline__ W neg_if(W a, bool n) { return n ? (W)0 - a : a; }
    static __device__ __forceinline__ W shr(W a, uint32_t s) { return a >> s; }
    static __device__ __forceinline__ W band(W a, W b) { return a & b; }
};
template <> struct WordOps<Word128> {
    static constexpr int BITS = 128;
    static __device__ __forceinline__ Word128 add(Word128 a, Word128 b) { return word_add<Word128>(a, b); }
    static __device__ __forceinline__ Word128 sub(Word128 a, Word128 b) {
        return Word128{a.lo - b.lo, a.hi - b.hi - (a.lo < b.lo ? 1u : 0u)};
    }
    static __device__ __forceinline__ Word128 neg_if(Word128 a, bool n) { return n ? sub(Word128{0, 0}, a) : a; }
    static __device__ __forceinline__ Word128 shr(Word128 a, uint32_t s) {
        if (s >= 64) return Word128{a.hi >> (s - 64), 0};
        if (s == 0) return a;
        return Word128{(a.lo >> s) | (a.hi << (64 - s)), a.hi >> s};
    }
    static __device__ __forceinline__ Word128 band(Word128 a, Word128 b) { return Word128{a.lo & b.lo, a.hi & b.hi}; }
};

// coefficient `pos` of the source polynomial of f (n = 2^logn words) for the exponent a < 2n (0 for the PLAIN mode)
template <class W>
__device__ __forceinline__ W gadget_source(const W *__restrict__ f, uint32_t pos, uint32_t a, uint32_t logn, bool cmux) {
    const uint32_t n = 1u << logn, t = (pos - a) & (2 * n - 1);
    W x = WordOps<W>::neg_if(f[t & (n - 1)], (t & n) != 0);
    if (cmux) x = WordOps<W>::sub(x, f[pos]);
    return x;
}

// constants of one decomposition call (stand-alone kernel: any base_log <= w)
template <class W> struct GadgetConst {
    W off, mask, half;   // 2^(s-1) + K 2^s,  B - 1,  B / 2
    uint32_t base_log, levels, npolys, rotated, cmux;
};

// terms[b][p * levels + l - 1] = digit l of source(polys[b][p], rot[b]): one thread per 16 bytes of destination coefficients of one
// polynomial, grid-stride over batch * npolys polynomials; STREAM: the terms are larger than STREAM_BYTES and pass through once
template <class W, bool STREAM>
__global__ __launch_bounds__(256) void native_gadget_kernel(W *__restrict__ terms, const W *__restrict__ polys,
                                                            const uint32_t *__restrict__ rot, const GadgetConst<W> G, uint32_t logn,
                                                            size_t npoly_total) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;   // 16 bytes of any word type
    const uint32_t lv = logn - LOGV;   // log2 vectors per polynomial (n >= 32)
    const size_t total = npoly_total << lv, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t q = i >> lv;   // b * npolys + p
        const uint32_t pos0 = (uint32_t)(i & (((size_t)1 << lv) - 1)) << LOGV;
        const uint32_t a = G.rotated ? rot[q / G.npolys] & ((2u << logn) - 1u) : 0u;
        const W *f = polys + (q << logn);
        W y[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) y[k] = O::add(gadget_source<W>(f, pos0 + (uint32_t)k, a, logn, G.cmux != 0), G.off);
        W *dst = terms + ((q * G.levels) << logn) + pos0;
        uint32_t sh = (uint32_t)O::BITS;
        for (uint32_t l = 0; l < G.levels; ++l, dst += (size_t)1 << logn) {
            sh -= G.base_log;
            union {
                W w[NV];
                V v;
            } d;
#pragma unroll
            for (int k = 0; k < NV; ++k) d.w[k] = O::sub(O::band(O::shr(y[k], sh), G.mask), G.half);
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
            else *reinterpret_cast<V *>(dst) = d.v;
        }
    }
}

// native_ext_kernel on undecomposed polynomials, u32 / u64 words and base_log <= 31: term j = (p, l) is digit l + 1 of polynomial p.  The
// digit fits a signed 32-bit register (|d| <= 2^30), so its lazy residue in [0, 2 P_i) is d + (d < 0 ? 2 P_i : 0) -- P_i alone would not
// do: P_i < 2^30 leaves -2^30 + P_i negative -- and no split30_lazy is needed.
// The addend may be `out` itself (add_out != 0: every thread reads a position through the pointer it then stores to, and nobody else
// touches it) or any buffer that does not overlap out, `polys` included, which is only read; out must not overlap polys (each launch of
// NOUT outputs reads all of polys).
template <int KIND, int LOGN, int BLK, int WPS, int NOUT>
__global__ __launch_bounds__(BLK, WPS) void native_ext_gadget_kernel(typename NativeShape<KIND>::W *__restrict__ out,
                                                                     const typename NativeShape<KIND>::W *polys, const uint32_t *rot,
                                                                     const typename NativeShape<KIND>::W *addend, const KeyPlanes K,
                                                                     const FusedTables<NativeShape<KIND>::KP> F, const SplitArgs S,
                                                                     const AccArgs C, typename NativeShape<KIND>::W off, uint32_t batch,
                                                                     uint32_t npolys, uint32_t levels, uint32_t base_log, uint32_t cmux,
                                                                     uint32_t add_out, uint32_t nout, uint32_t o0) {
    static_assert(sizeof(typename NativeShape<KIND>::W) <= 8, "the fused decomposition covers the 32- and 64-bit kinds");
    const uint32_t nterms = npolys * levels;
#define NATIVE_EXT_LOAD_TERM(a)                                                                                                          \
    const uint32_t gp = j / levels, gl = j - gp * levels;                                                                                \
    const uint32_t gsh = (uint32_t)sizeof(W) * 8u - base_log * (gl + 1u), gmask = (1u << base_log) - 1u, ghalf = 1u << (base_log - 1u);  \
    const uint32_t gr = rot ? rot[subc] & ((2u << LOGN) - 1u) : 0u;   /* rot == nullptr: PLAIN */                                        \
    const W *gf = polys + (((size_t)subc * npolys + gp) << LOGN);                                                                        \
    _Pragma("unroll") for (int e = 0; e < E; ++e) {                                                                                      \
        const uint32_t pos = eb | cdep((uint32_t)e, RM0), gt = (pos - gr) & ((2u << LOGN) - 1u);                                         \
        const W gm = (W)0 - (W)((gt >> LOGN) & 1u);   /* all ones: the coefficient wrapped around X^n = -1 */                            \
        W gx = (W)((gf[gt & ((1u << LOGN) - 1u)] ^ gm) - gm);                                                                            \
        if (cmux) gx = (W)(gx - gf[pos]);                                                                                                \
        const int32_t gd = (int32_t)((uint32_t)((W)(gx + off) >> gsh) & gmask) - (int32_t)ghalf;                                         \
        a[e] = (uint32_t)gd + ((uint32_t)(gd >> 31) & (uint32_t)Pv.two_p);                                                               \
    }
#define NATIVE_EXT_ADD(w, dst)                      \
    if (add_out) w = (W)(w + *dst);                 \
    else if (addend) w = (W)(w + addend[dst - out]);
#include "native_ext_body.inc"
#undef NATIVE_EXT_LOAD_TERM
#undef NATIVE_EXT_ADD
}

}  // namespace cntt
