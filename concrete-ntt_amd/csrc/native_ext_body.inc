// Body of the fused external-product kernels, included textually by native_ext_kernel (native_ext.hpp) and native_ext_gadget_kernel
// (native_gadget.hpp) inside their function bodies.  In scope: KIND, LOGN, BLK, NOUT, out, K, F, S, C, batch, nterms, nout, o0, and two macros
//   NATIVE_EXT_LOAD_TERM(a)   fills uint32_t a[E] with the thread's coefficients (positions eb | cdep(e, RM0)) of term j of element subc as
//                             lazy residues of prime i in [0, 2 P_i); sees subc, j, eb, i, Pv
//   NATIVE_EXT_ADD(w, dst)    adds what the call accumulates onto to the word w about to be stored at dst (a pointer into out)
// Shared as text and not through a functor: these kernels sit at the edge of their register budgets, and with the load behind a template
// parameter one native128 instance of the existing kernel went from 0 to 52 bytes of scratch.  As text, native_ext_kernel compiles to the
// instructions it had before the load was factored out.
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
            uint32_t a[E];
            NATIVE_EXT_LOAD_TERM(a)
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
                NATIVE_EXT_ADD(w, dst)
                *dst = w;
            }
        }
    }
