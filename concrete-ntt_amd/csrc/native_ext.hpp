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
    using SH = NativeShape<KIND>;
    using W = typename SH::W;
    using AW = AccWord<W>;
    using Wf = NttWp<uint32_t, LOGN, false, CLS_LAZY, BLK, ACC_FAM>;
    using Wi = NttWp<uint32_t, LOGN, true, CLS_LAZY, BLK, ACC_FAM>;
    constexpr int E = Wf::E, TPP = Wf::TPP, NPASS = Wf::NPASS, KP = SH::KP, PPB = BLK / TPP;
    static_assert(BLK % TPP == 0 && PPB >= 1, "whole elements per workgroup");
    constexpr uint32_t FULL = Wf::FULL, RM0 = Wf::S::RMASK[0], RML = Wf::S::RMASK[NPASS - 1];
    static_assert(RM0 == Wi::S::RMASK[NPASS - 1] && RML == Wi::S::RMASK[0], "forward and inverse schedules must mirror each other");
    static_assert(2ull * KP * (1ull << ACC_FRAC_BITS) + (1ull << (ACC_FRAC_BITS - 1)) <= (1ull << 32),
                  "the fraction sum of lazy residues (each below 2 P_i) and its rounding constant fit 32 bits");
    __shared__ __attribute__((aligned(16))) uint32_t lds_all[(size_t)PPB * Wf::B::LDS_WORDS_1];
    const uint32_t tid = threadIdx.x & (TPP - 1), pl = threadIdx.x / TPP;
    uint32_t *lds = lds_all + (size_t)pl * Wf::B::LDS_WORDS_1;
    const uint32_t sub0 = blockIdx.x * PPB, sub = sub0 + pl;
    const uint32_t subc = sub < batch ? sub : batch - 1;   // ragged tail: recompute the last element, store nothing
    typename AW::A acc[NOUT][E];
    uint32_t frac[NOUT][E];
#pragma unroll
    for (int o = 0; o < NOUT; ++o)
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc[o][e] = 0;
            frac[o][e] = 0;
        }
    // the primes and the terms are runtime loops: one copy of the forward and of the inverse transform
#pragma clang loop unroll(disable)
    for (int i = 0; i < KP; ++i) {
        const ModParams<uint32_t> &Pv = F.P[i];
        const uint32_t *key = K.k[i];
        uint32_t s[NOUT][E];   // sum_j fwd(terms[j]) key[j][o] / 2^32, lazy in [0, 2 P_i)
#pragma unroll
        for (int o = 0; o < NOUT; ++o)
#pragma unroll
            for (int e = 0; e < E; ++e) s[o][e] = 0;
#pragma clang loop unroll(disable)
        for (uint32_t j = 0; j < nterms; ++j) {
            // offsets from an opaque copy of the thread index per term: hoisted out of the loops they stay live next to the accumulators
            uint32_t tidf = tid;
            asm volatile("" : "+v"(tidf));
            const uint32_t eb = pdep<FULL & ~RM0>(tidf);
            const W *tp = terms + (((size_t)subc * nterms + j) << LOGN);
            uint32_t a[E];
#pragma unroll
            for (int e = 0; e < E; ++e) a[e] = split30_lazy<W>(tp[eb | cdep((uint32_t)e, RM0)], S, C, i);
            __builtin_amdgcn_sched_barrier(0);
            Wf::template pass<0, false, false, false, 0>(a, lds, tidf, F.twf[i], nullptr, Pv);   // lazy outputs in [0, 4p)
            Wf::wsync();   // the exchange buffer is reused by the next transform
            __builtin_amdgcn_sched_barrier(0);
            // the forward transform leaves coefficient e of this thread at position ebk | cdep(e, RML) of the bit-reversed order the
            // key residues are stored in (the order NttWp::run writes)
            const uint32_t ebk = pdep<FULL & ~RML>(tidf);
#pragma unroll
            for (int o = 0; o < NOUT; ++o) {
                const uint32_t *kp = key + (((size_t)j * nout + o0 + o) << LOGN);
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const uint32_t t = s[o][e] + acc_mont_lazy(a[e], kp[ebk | cdep((uint32_t)e, RML)], Pv);
                    s[o][e] = umin<uint32_t>(t, t - Pv.two_p);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        const uint64_t clo = C.c_lo[i], chi = C.c_hi[i];
        const uint32_t fi = C.f[i];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            uint32_t tidi = tid;
            asm volatile("" : "+v"(tidi));
            // FIN = false: the lazy outputs in [0, 2 P_i) are gamma_i (the last stage's constants carry (M / P_i)^-1 / n)
            Wi::template pass<0, true, false, false, 0>(s[o], lds, tidi, F.twi[i], nullptr, Pv);
            Wf::wsync();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                acc[o][e] = AW::mad(acc[o][e], s[o][e], clo, chi);
                frac[o][e] += __umulhi(s[o][e], fi);
                AW::pin(acc[o][e]);   // (opaque: otherwise hipcc sinks the sums to the store and keeps the residue tiles instead)
                asm volatile("" : "+v"(frac[o][e]));
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (sub < batch) {
        uint32_t tx = tid;
        asm volatile("" : "+v"(tx));
        const uint32_t ebo = pdep<FULL & ~RM0>(tx);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            W *op = out + (((size_t)sub * nout + o0 + o) << LOGN);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const uint32_t k = (frac[o][e] + (1u << (ACC_FRAC_BITS - 1))) >> ACC_FRAC_BITS;
                W w = AW::out(acc[o][e], k, C.m_lo, C.m_hi);
                W *dst = op + (ebo | cdep((uint32_t)e, RM0));
                if (accumulate) w = word_add<W>(w, *dst);
                *dst = w;
            }
        }
    }
}

// composed path: a[i] = a[i] + b[i] modulo 2^bits(W) (accumulate onto the caller's output)
template <class W> __global__ void native_word_add_kernel(W *__restrict__ a, const W *__restrict__ b, size_t count) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        a[i] = word_add<W>(a[i], b[i]);
}

}  // namespace cntt
