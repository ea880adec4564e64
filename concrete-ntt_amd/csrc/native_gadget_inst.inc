// Shared body of the fused decomposing external-product instantiation units (one per 32- / 64-bit native Plan32 kind).  Requires: INST_KIND.
#include "native_gadget.hpp"
#include "ntt_launch.hpp"

namespace cntt {

template <int KIND, int LOGN, int NOUT>
static void gadget_launch(void *out, const GadgetCall &G, const KeyPlanes &K, const FusedTables<NativeShape<KIND>::KP> &F,
                          const SplitArgs &S, const AccArgs &C, uint32_t batch, uint32_t nout, uint32_t o0, hipStream_t st) {
    using W = typename NativeShape<KIND>::W;
    using K0 = NttKernel<uint32_t, LOGN, false, CLS_LAZY, false, ACC_FAM>;
    constexpr int BLK = 256, PPB = BLK / K0::TPP;
    constexpr int WPS = NOUT == 2 ? 2 : 3;   // the register budgets of native_ext_kernel (native_ext_inst.inc)
    const uint32_t grid = (batch + PPB - 1) / PPB;
    hipLaunchKernelGGL((native_ext_gadget_kernel<KIND, LOGN, BLK, WPS, NOUT>), dim3(grid), dim3(BLK), 0, st, (W *)out, (const W *)G.polys,
                       G.rot, (const W *)G.addend, K, F, S, C, (W)G.off, batch, G.npolys, G.levels, G.base_log, G.cmux, G.add_out, nout, o0);
}

template <int KIND, int LOGN>
static hipError_t gadget_logn(int logn, void *out, const GadgetCall &G, const KeyPlanes &K, const FusedTables<NativeShape<KIND>::KP> &F,
                              const SplitArgs &S, const AccArgs &C, uint32_t batch, uint32_t nout, hipStream_t st) {
    if constexpr (LOGN > NATIVE_EXT_MAX_LOGN) {
        return hipErrorNotSupported;
    } else {
        if (logn == LOGN) {
            using K0 = NttKernel<uint32_t, LOGN, false, CLS_LAZY, false, ACC_FAM>;
            if constexpr (native_fused_acc(KIND, LOGN) && K0::NPASS > 1 && K0::LOGE == 4 && K0::TPP <= 256) {
                // outputs in launches of two, an odd last one alone, as the external product on ready-made terms
                for (uint32_t o0 = 0; o0 < nout; o0 += 2) {
                    if (nout - o0 >= 2) gadget_launch<KIND, LOGN, 2>(out, G, K, F, S, C, batch, nout, o0, st);
                    else gadget_launch<KIND, LOGN, 1>(out, G, K, F, S, C, batch, nout, o0, st);
                    const hipError_t e = hipGetLastError();
                    if (e != hipSuccess) return e;
                }
                return hipSuccess;
            } else {
                return hipErrorNotSupported;
            }
        }
        return gadget_logn<KIND, LOGN + 1>(logn, out, G, K, F, S, C, batch, nout, st);
    }
}

template <>
hipError_t launch_native_ext_gadget<INST_KIND>(int logn, void *out, const GadgetCall &G, const KeyPlanes &K, const void *tables_acc,
                                               const SplitArgs &S, const AccArgs &C, uint32_t batch, uint32_t nout, hipStream_t st) {
    static_assert(sizeof(NativeShape<INST_KIND>::W) <= 8, "32- and 64-bit kinds only");
    if (batch == 0 || nout == 0) return hipSuccess;
    if (logn < 5 || logn > NATIVE_EXT_MAX_LOGN || G.base_log < 1 || G.base_log > 31) return hipErrorNotSupported;
    using FT = FusedTables<NativeShape<INST_KIND>::KP>;
    return gadget_logn<INST_KIND, 5>(logn, out, G, K, *static_cast<const FT *>(tables_acc), S, C, batch, nout, st);
}

}  // namespace cntt
