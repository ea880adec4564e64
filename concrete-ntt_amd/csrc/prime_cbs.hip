// kernel instantiations and launchers of the prime plans' circuit bootstrap (prime_cbs.hpp): u32 / u64 words
#include "prime_cbs.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_cbs_setup(uint32_t *rot_t, T *table, const T *lwe, const PrimeCbsSetup<T> &C, size_t lwe_dim, size_t elements, unsigned grid,
                                  hipStream_t st) {
    if (C.logn < 4 || C.logn > 29 || elements == 0 || C.cbs_levels == 0 || elements % C.cbs_levels) return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_cbs_setup_kernel<T>), dim3(grid), dim3(256), 0, st, rot_t, table, lwe, C, lwe_dim, elements);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_cbs_extract(int32_t *digits, const T *acc, const PrimePackConst<T> &G, const PrimeCbsSetup<T> &C, size_t elements,
                                    unsigned grid, hipStream_t st) {
    if (elements == 0 || G.levels == 0 || G.base_log == 0 || G.base_log > 31 || (uint64_t)G.base_log * G.levels > C.wbits) return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_cbs_extract_kernel<T>), dim3(grid), dim3(256), 0, st, digits, acc, G, C, elements);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_cbs_ks(T *part, const int32_t *digits, const T *key, T p, int logn, size_t glwe_dim, size_t rows, size_t elements,
                               const CbsShape &Z, unsigned bits, hipStream_t st) {
    // the shape must cover the rows, the elements and the columns it is launched for, and the reduction the accumulator
    if (logn < 4 || logn > 30 || rows == 0 || elements == 0 || glwe_dim + 1 >= ((size_t)1 << 32) || Z.rows == 0 || Z.rows * Z.slabs < rows ||
        Z.tiles * CBS_ET < elements || Z.cols * 256 * (16 / sizeof(T)) < ((glwe_dim + 1) << logn) || bits == 0 || bits > (sizeof(T) == 8 ? 127u : 95u))
        return hipErrorInvalidValue;
    const dim3 grid(prime_cbs_grid(Z.items(glwe_dim), logn, sizeof(T)));
    hipLaunchKernelGGL((prime_cbs_ks_kernel<T>), grid, dim3(256), 0, st, part, digits, key, p, (uint32_t)logn, (uint32_t)glwe_dim, rows, elements, Z,
                       (uint32_t)bits);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_cbs_sum(T *out, const T *part, T p, int logn, size_t glwe_dim, unsigned cbs_levels, size_t elements, size_t slabs,
                                unsigned grid, hipStream_t st) {
    if (elements == 0 || slabs == 0 || cbs_levels == 0 || elements % cbs_levels) return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_cbs_sum_kernel<T>), dim3(grid), dim3(256), 0, st, out, part, p, (uint32_t)logn, (uint32_t)glwe_dim, (uint32_t)cbs_levels,
                       elements, slabs);
    return hipGetLastError();
}

#define CNTT_PRIME_CBS_INST(T)                                                                                                                \
    template hipError_t launch_prime_cbs_setup<T>(uint32_t *, T *, const T *, const PrimeCbsSetup<T> &, size_t, size_t, unsigned, hipStream_t); \
    template hipError_t launch_prime_cbs_extract<T>(int32_t *, const T *, const PrimePackConst<T> &, const PrimeCbsSetup<T> &, size_t, unsigned, \
                                                    hipStream_t);                                                                             \
    template hipError_t launch_prime_cbs_ks<T>(T *, const int32_t *, const T *, T, int, size_t, size_t, size_t, const CbsShape &, unsigned,    \
                                               hipStream_t);                                                                                  \
    template hipError_t launch_prime_cbs_sum<T>(T *, const T *, T, int, size_t, unsigned, size_t, size_t, unsigned, hipStream_t);
CNTT_PRIME_CBS_INST(uint32_t)
CNTT_PRIME_CBS_INST(uint64_t)
#undef CNTT_PRIME_CBS_INST

}  // namespace cntt
