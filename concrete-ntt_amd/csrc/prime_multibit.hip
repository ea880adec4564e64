// kernel instantiations and the launcher of the prime plans' multi-bit accumulate (prime_multibit.hpp): u32 / u64 words
#include "prime_multibit.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_multibit_accumulate(T *out, const T *terms, const uint32_t *rot_rows, const T *key, const T *tab, T p, T pinv_neg,
                                            int logn, size_t nterms, size_t nout, unsigned grouping, size_t batch, hipStream_t st) {
    constexpr int LOGV = sizeof(T) == 4 ? 2 : 1;
    if (grouping == 0 || grouping > PRIME_MULTIBIT_MAX_GROUPING || logn < 4 || logn > 30 || batch == 0 || nout == 0 || nterms == 0 ||
        nterms >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32))
        return hipErrorInvalidValue;
    const size_t vectors = (batch * nout) << (logn - LOGV);
    hipLaunchKernelGGL((prime_multibit_accumulate_kernel<T>), dim3(prime_multibit_grid(vectors)), dim3(256), 0, st, out, terms, rot_rows, key,
                       tab, p, pinv_neg, (uint32_t)logn, (uint32_t)nterms, (uint32_t)nout, (uint32_t)grouping, batch);
    return hipGetLastError();
}

template hipError_t launch_prime_multibit_accumulate<uint32_t>(uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *,
                                                               const uint32_t *, uint32_t, uint32_t, int, size_t, size_t, unsigned, size_t,
                                                               hipStream_t);
template hipError_t launch_prime_multibit_accumulate<uint64_t>(uint64_t *, const uint64_t *, const uint32_t *, const uint64_t *,
                                                               const uint64_t *, uint64_t, uint64_t, int, size_t, size_t, unsigned, size_t,
                                                               hipStream_t);

}  // namespace cntt
