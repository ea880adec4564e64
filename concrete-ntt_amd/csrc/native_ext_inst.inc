// Shared body of the fused external-product instantiation units (one per native Plan32 kind).  Requires: INST_KIND.
#include "native_ext.hpp"
#include "ntt_launch.hpp"

namespace cntt {

template <int KIND, int LOGN, int NOUT>
static void ext_launch(void *out, const void *terms, const KeyPlanes &K, const FusedTables<NativeShape<KIND>::KP> &F, const SplitArgs &S,
                       const AccArgs &C, uint32_t batch, uint32_t nterms, uint32_t nout, uint32_t o0, bool accumulate, hipStream_t st) {
    using W = typename NativeShape<KIND>::W;
    using K0 = NttKernel<uint32_t, LOGN, false, CLS_LAZY, false, ACC_FAM>;
    constexpr int BLK = 256, PPB = BLK / K0::TPP;
    // one output: three 256-thread workgroups per compute unit (<= 168 VGPRs, 130 used) as the whole-product kernel; two outputs: two
    // workgroups (at three, the second set of accumulators spilled 32 registers)
    constexpr int WPS = NOUT == 2 ? 2 : 3;
    const uint32_t grid = (batch + PPB - 1) / PPB;
    hipLaunchKernelGGL((native_ext_kernel<KIND, LOGN, BLK, WPS, NOUT>), dim3(grid), dim3(BLK), 0, st, (W *)out, (const W *)terms, K, F, S,
                       C, batch, nterms, nout, o0, accumulate ? 1 : 0);
}

template <int KIND, int LOGN>
static hipError_t ext_logn(int logn, void *out, const void *terms, const KeyPlanes &K, const FusedTables<NativeShape<KIND>::KP> &F,
                           const SplitArgs &S, const AccArgs &C, uint32_t batch, uint32_t nterms, uint32_t nout, bool accumulate,
                           hipStream_t st) {
    if constexpr (LOGN > NATIVE_EXT_MAX_LOGN) {
        return hipErrorNotSupported;
    } else {
        if (logn == LOGN) {
            using K0 = NttKernel<uint32_t, LOGN, false, CLS_LAZY, false, ACC_FAM>;
            if constexpr (native_fused_acc(KIND, LOGN) && K0::NPASS > 1 && K0::LOGE == 4 && K0::TPP <= 256) {
                // outputs in launches of two (the accumulators grow with NOUT; the prime-plan chains split the same way), an odd last one
                // alone; one per launch for 16-byte words, whose two-output kernel spills 7 ... 13 registers even at 256 VGPRs
                constexpr uint32_t NMAX = sizeof(typename NativeShape<KIND>::W) == 16 ? 1 : 2;
                for (uint32_t o0 = 0; o0 < nout; o0 += NMAX) {
                    if constexpr (NMAX == 2) {
                        if (nout - o0 >= 2) {
                            ext_launch<KIND, LOGN, 2>(out, terms, K, F, S, C, batch, nterms, nout, o0, accumulate, st);
                        } else {
                            ext_launch<KIND, LOGN, 1>(out, terms, K, F, S, C, batch, nterms, nout, o0, accumulate, st);
                        }
                    } else {
                        ext_launch<KIND, LOGN, 1>(out, terms, K, F, S, C, batch, nterms, nout, o0, accumulate, st);
                    }
                    const hipError_t e = hipGetLastError();
                    if (e != hipSuccess) return e;
                }
                return hipSuccess;
            } else {
                return hipErrorNotSupported;
            }
        }
        return ext_logn<KIND, LOGN + 1>(logn, out, terms, K, F, S, C, batch, nterms, nout, accumulate, st);
    }
}

template <>
hipError_t launch_native_ext<INST_KIND>(int logn, void *out, const void *terms, const KeyPlanes &K, const void *tables_acc,
                                        const SplitArgs &S, const AccArgs &C, uint32_t batch, uint32_t nterms, uint32_t nout,
                                        bool accumulate, hipStream_t st) {
    if (batch == 0 || nout == 0) return hipSuccess;
    if (logn < 5 || logn > NATIVE_EXT_MAX_LOGN) return hipErrorNotSupported;
    using FT = FusedTables<NativeShape<INST_KIND>::KP>;
    return ext_logn<INST_KIND, 5>(logn, out, terms, K, *static_cast<const FT *>(tables_acc), S, C, batch, nterms, nout, accumulate, st);
}

}  // namespace cntt
