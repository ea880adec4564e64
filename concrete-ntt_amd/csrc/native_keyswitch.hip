// kernel instantiations and the launcher of the LWE keyswitch (native_keyswitch.hpp): u32 / u64 / Word128 words
#include "native_keyswitch.hpp"

namespace cntt {

template <class W>
static void keyswitch_w(void *out, const void *in, const void *ksk, W off, unsigned base_log, unsigned levels, size_t lin, size_t lout,
                        size_t row_stride, size_t batch, hipStream_t st) {
    constexpr size_t BM = 4 * KsTile<W>::TB, BN = 64 * KsTile<W>::TC;
    const size_t tiles = ((lout + BN) / BN) * ((batch + BM - 1) / BM);   // (lout + 1 columns)
    const unsigned grid = (unsigned)(tiles < ((size_t)1 << 24) ? tiles : ((size_t)1 << 24) - 1);
    hipLaunchKernelGGL((native_keyswitch_kernel<W>), dim3(grid), dim3(256), 0, st, (W *)out, (const W *)in, (const W *)ksk, off,
                       (uint32_t)base_log, (uint32_t)levels, lin, lout, row_stride, batch);
}

hipError_t launch_native_keyswitch(int word, void *out, const void *in, const void *ksk, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                   unsigned levels, size_t lin, size_t lout, size_t row_stride, size_t batch, hipStream_t st) {
    if (levels == 0 || levels > (unsigned)KS_ROWS || base_log == 0 || base_log > 31 || batch == 0) return hipErrorInvalidValue;
    if (word == 4) keyswitch_w<uint32_t>(out, in, ksk, (uint32_t)off_lo, base_log, levels, lin, lout, row_stride, batch, st);
    else if (word == 8) keyswitch_w<uint64_t>(out, in, ksk, off_lo, base_log, levels, lin, lout, row_stride, batch, st);
    else keyswitch_w<Word128>(out, in, ksk, Word128{off_lo, off_hi}, base_log, levels, lin, lout, row_stride, batch, st);
    return hipGetLastError();
}

}  // namespace cntt
