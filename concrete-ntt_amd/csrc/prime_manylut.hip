// kernel instantiations and launchers of the prime plans' many-LUT bootstrap and one-rotation circuit bootstrap (prime_manylut.hpp):
// u32 / u64 words
#include "prime_manylut.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_modswitch_manylut(uint32_t *rot_t, const T *lwe, T p, int logn, unsigned log_lut, size_t lwe_dim, size_t batch,
                                          unsigned grid, hipStream_t st) {
    if (logn < 4 || logn > 29 || log_lut > (unsigned)logn || batch == 0) return hipErrorInvalidValue;
    PrimeCbsSetup<T> C{};
    C.p = p;
    C.logn = (uint32_t)logn;
    hipLaunchKernelGGL((prime_modswitch_manylut_kernel<T, false>), dim3(grid), dim3(256), 0, st, rot_t, (T *)nullptr, lwe, C, (uint32_t)log_lut,
                       lwe_dim, batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_cbs_manylut_setup(uint32_t *rot_t, T *table, const T *lwe, const PrimeCbsSetup<T> &C, unsigned log_lut, size_t lwe_dim,
                                          size_t batch, unsigned grid, hipStream_t st) {
    // the levels fit the interleaved table, and the two bit values n / 2 and 3 n / 2 lie on the coarse grid
    if (C.logn < 4 || C.logn > 29 || log_lut + 1u > C.logn || batch == 0 || C.cbs_levels == 0 || C.cbs_levels > (1u << log_lut))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_modswitch_manylut_kernel<T, true>), dim3(grid), dim3(256), 0, st, rot_t, table, lwe, C, (uint32_t)log_lut, lwe_dim,
                       batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_sample_extract_many(T *lwe_out, const T *glwe, T p, int logn, size_t glwe_dim, size_t count, size_t batch, bool stream,
                                            unsigned grid, hipStream_t st) {
    if (logn < 4 || logn > 30 || count == 0 || count > ((size_t)1 << logn) || batch == 0) return hipErrorInvalidValue;
    if (stream)
        hipLaunchKernelGGL((prime_sample_extract_many_kernel<T, true>), dim3(grid), dim3(256), 0, st, lwe_out, glwe, p, (uint32_t)logn, glwe_dim,
                           count, batch);
    else
        hipLaunchKernelGGL((prime_sample_extract_many_kernel<T, false>), dim3(grid), dim3(256), 0, st, lwe_out, glwe, p, (uint32_t)logn, glwe_dim,
                           count, batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_cbs_manylut_extract(int32_t *digits, const T *acc, const PrimePackConst<T> &G, const PrimeCbsSetup<T> &C, size_t batch,
                                            unsigned grid, hipStream_t st) {
    if (batch == 0 || C.logn < 4 || C.cbs_levels == 0 || C.cbs_levels > (1u << (C.logn - 1u)) || G.levels == 0 || G.base_log == 0 ||
        G.base_log > 31 || (uint64_t)G.base_log * G.levels > C.wbits)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_cbs_manylut_extract_kernel<T>), dim3(grid), dim3(256), 0, st, digits, acc, G, C, batch);
    return hipGetLastError();
}

#define CNTT_PRIME_MANYLUT_INST(T)                                                                                                              \
    template hipError_t launch_prime_modswitch_manylut<T>(uint32_t *, const T *, T, int, unsigned, size_t, size_t, unsigned, hipStream_t);      \
    template hipError_t launch_prime_cbs_manylut_setup<T>(uint32_t *, T *, const T *, const PrimeCbsSetup<T> &, unsigned, size_t, size_t,      \
                                                          unsigned, hipStream_t);                                                               \
    template hipError_t launch_prime_sample_extract_many<T>(T *, const T *, T, int, size_t, size_t, size_t, bool, unsigned, hipStream_t);       \
    template hipError_t launch_prime_cbs_manylut_extract<T>(int32_t *, const T *, const PrimePackConst<T> &, const PrimeCbsSetup<T> &, size_t, \
                                                            unsigned, hipStream_t);
CNTT_PRIME_MANYLUT_INST(uint32_t)
CNTT_PRIME_MANYLUT_INST(uint64_t)
#undef CNTT_PRIME_MANYLUT_INST

}  // namespace cntt
