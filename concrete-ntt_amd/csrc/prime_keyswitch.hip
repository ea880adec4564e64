// kernel instantiations and the launcher of the prime plans' LWE keyswitch (prime_keyswitch.hpp): u32 / u64 words
#include "prime_keyswitch.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_keyswitch(T *out, const T *in, const T *ksk, const PrimeKsConst<T> &K, size_t lin, size_t lout, size_t row_stride,
                                  size_t batch, hipStream_t st) {
    const uint32_t base_log = K.base_log, levels = K.levels;
    if (levels == 0 || base_log == 0 || base_log > 31 || levels > prime_ks_chunk_rows(base_log) || batch == 0) return hipErrorInvalidValue;
    constexpr size_t BM = 4 * PrimeKsTile<T>::TB, BN = 64 * PrimeKsTile<T>::TC;
    using u128 = unsigned __int128;
    const u128 tiles = (u128)((lout + BN) / BN) * ((batch + BM - 1) / BM);   // (lout + 1 columns)
    // the kernel counts key rows and tiles in 32 bits, and steps its tile counter by the grid (sizes past these fit no device's memory)
    if ((u128)lin * levels >> 32 || tiles >= ((u128)1 << 32) - ((u128)1 << 24)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)(tiles < ((u128)1 << 24) ? tiles : ((u128)1 << 24) - 1);
    hipLaunchKernelGGL((prime_keyswitch_kernel<T>), dim3(grid), dim3(256), 0, st, out, in, ksk, K, (uint32_t)lin, lout, row_stride, batch);
    return hipGetLastError();
}

template hipError_t launch_prime_keyswitch<uint32_t>(uint32_t *, const uint32_t *, const uint32_t *, const PrimeKsConst<uint32_t> &, size_t,
                                                     size_t, size_t, size_t, hipStream_t);
template hipError_t launch_prime_keyswitch<uint64_t>(uint64_t *, const uint64_t *, const uint64_t *, const PrimeKsConst<uint64_t> &, size_t,
                                                     size_t, size_t, size_t, hipStream_t);

}  // namespace cntt
