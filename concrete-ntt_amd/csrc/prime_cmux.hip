// kernel instantiations and the launcher of the prime plans' CMux (prime_cmux.hpp): u32 / u64 words
#include "prime_cmux.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_cmux_diff(T *terms, T *out, const T *c0, const T *c1, bool leaf, const PrimePackConst<T> &G, int logn, size_t glwe_dim,
                                  size_t h, size_t gs, size_t nct, bool stream, hipStream_t st) {
    if (logn < 4 || logn > 30 || nct == 0 || h == 0 || nct % h || gs < h || glwe_dim + 1 >= ((size_t)1 << 32) || G.levels == 0 ||
        G.base_log == 0 || (uint64_t)G.base_log * G.levels > sizeof(T) * 8)
        return hipErrorInvalidValue;
    const dim3 grid(prime_cmux_grid(nct * (glwe_dim + 1), logn, sizeof(T))), block(256);
    const uint32_t ln = (uint32_t)logn, k = (uint32_t)glwe_dim;
#define CNTT_CMUX_LAUNCH(STREAM, LEAF) \
    hipLaunchKernelGGL((prime_cmux_diff_kernel<T, STREAM, LEAF>), grid, block, 0, st, terms, out, c0, c1, G, ln, k, h, gs, nct)
    if (stream && leaf) CNTT_CMUX_LAUNCH(true, true);
    else if (stream) CNTT_CMUX_LAUNCH(true, false);
    else if (leaf) CNTT_CMUX_LAUNCH(false, true);
    else CNTT_CMUX_LAUNCH(false, false);
#undef CNTT_CMUX_LAUNCH
    return hipGetLastError();
}

#define CNTT_PRIME_CMUX_INST(T)                                                                                                              \
    template hipError_t launch_prime_cmux_diff<T>(T *, T *, const T *, const T *, bool, const PrimePackConst<T> &, int, size_t, size_t, size_t, \
                                                  size_t, bool, hipStream_t);
CNTT_PRIME_CMUX_INST(uint32_t)
CNTT_PRIME_CMUX_INST(uint64_t)
#undef CNTT_PRIME_CMUX_INST

}  // namespace cntt
