// Fused external product of the native / native_binary Plan32 kinds (include/cntt_ext.h, cntt_native_external_product_batch):
//     out[b][o] (+)= sum_j terms[b][j] (*) key[j][o]      in Z/2^w[X]/(X^n + 1)
// with the key given once, already forward-transformed per prime (what cntt_native_fwd_batch / fwd_binary_batch write) and shared by
// the whole batch.  The sum of the products is ONE CRT of the summed residue products while the summed integer stays inside the exact
// range of the reconstruction (cntt_native_max_terms), so per element and prime the kernel runs nterms forward transforms, a lazy
// multiply-accumulate against the key residues (read straight from global memory: L2-resident, shared by every workgroup), NOUT
// inverse transforms with 1/n and (M / P_i)^-1 in their last stage, and folds each output into its own accumulating-CRT state
// (native_fused.hpp, native_product_acc: AccWord + 27-bit fraction sum).  One HBM pass: terms read once per prime (L2 / MALL hits
// after the first), outputs written once.
#pragma once
#include "native_fused.hpp"

namespace cntt {

struct KeyPlanes {
    const uint32_t *k[10];   // per prime: nterms x nout_total forward-transformed residue polynomials, key[j][o] at j * nout_total + o
};

// a + b modulo 2^bits(W)
template <class W> __device__ __forceinline__ W word_add(W a, W b) { return a + b; }
template <> __device__ __forceinline__ Word128 word_add<Word128>(Word128 a, Word128 b) {
    const uint64_t lo = a.lo + b.lo;
    return Word128{lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

// one workgroup = PPB elements of the batch (TPP threads each, E = 16 coefficients per thread), NOUT outputs o0 .. o0 + NOUT - 1
template <int KIND, int LOGN, int BLK, int WPS, int NOUT>
__global__ __launch_bounds__(BLK, WPS) void native_ext_kernel(typename NativeShape<KIND>::W *__restrict__ out,
                                                              const typename NativeShape<KIND>::W *__restrict__ terms,
                                                              const KeyPlanes K, const FusedTables<NativeShape<KIND>::KP> F,
                                                              const SplitArgs S, const AccArgs C, uint32_t batch, uint32_t nterms,
                                                              uint32_t nout, uint32_t o0, int accumulate) {
    // the term load and the accumulation of this kernel: ready-made terms, split into lazy residues; out (+)= the sum
#define NATIVE_EXT_LOAD_TERM(a)                                                                                        \
    const W *tp = terms + (((size_t)subc * nterms + j) << LOGN);                                                        \
    _Pragma("unroll") for (int e = 0; e < E; ++e) a[e] = split30_lazy<W>(tp[eb | cdep((uint32_t)e, RM0)], S, C, i);
#define NATIVE_EXT_ADD(w, dst) \
    if (accumulate) w = word_add<W>(w, *dst);
#include "native_ext_body.inc"
#undef NATIVE_EXT_LOAD_TERM
#undef NATIVE_EXT_ADD
}

// composed path: a[i] = a[i] + b[i] modulo 2^bits(W) (accumulate onto the caller's output)
template <class W> __global__ void native_word_add_kernel(W *__restrict__ a, const W *__restrict__ b, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        a[i] = word_add<W>(a[i], b[i]);
}

}  // namespace cntt
