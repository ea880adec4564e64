// kernel instantiations and launchers of the prime plans' bootstrap kernels (prime_pbs.hpp): u32 / u64 words
#include "prime_pbs.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_gadget(T *terms, const T *polys, const uint32_t *rot, const PrimeGadgetConst<T> &G, int logn, size_t npoly_total,
                               bool stream, unsigned grid, hipStream_t st) {
    if (stream)
        hipLaunchKernelGGL((prime_gadget_kernel<T, true>), dim3(grid), dim3(256), 0, st, terms, polys, rot, G, (uint32_t)logn, npoly_total);
    else
        hipLaunchKernelGGL((prime_gadget_kernel<T, false>), dim3(grid), dim3(256), 0, st, terms, polys, rot, G, (uint32_t)logn, npoly_total);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_lwe_modswitch(uint32_t *rot_t, const T *lwe, T p, int logn, size_t lwe_dim, size_t batch, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((prime_lwe_modswitch_kernel<T>), dim3(grid), dim3(256), 0, st, rot_t, lwe, p, (uint32_t)logn, lwe_dim, batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_pbs_init(T *acc, const T *lut, const uint32_t *rot, T p, int logn, uint32_t npolys, bool per_element, size_t batch,
                                 bool stream, unsigned grid, hipStream_t st) {
    const uint32_t ls = per_element ? npolys : 0u;
    if (stream)
        hipLaunchKernelGGL((prime_pbs_init_kernel<T, true>), dim3(grid), dim3(256), 0, st, acc, lut, rot, p, (uint32_t)logn, npolys, ls,
                           batch * npolys);
    else
        hipLaunchKernelGGL((prime_pbs_init_kernel<T, false>), dim3(grid), dim3(256), 0, st, acc, lut, rot, p, (uint32_t)logn, npolys, ls,
                           batch * npolys);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_sample_extract(T *lwe_out, const T *glwe, T p, int logn, size_t glwe_dim, uint32_t index, size_t batch, unsigned grid,
                                       hipStream_t st) {
    hipLaunchKernelGGL((prime_sample_extract_kernel<T>), dim3(grid), dim3(256), 0, st, lwe_out, glwe, p, (uint32_t)logn, glwe_dim, index, batch);
    return hipGetLastError();
}

#define CNTT_PRIME_PBS_INST(T)                                                                                                               \
    template hipError_t launch_prime_gadget<T>(T *, const T *, const uint32_t *, const PrimeGadgetConst<T> &, int, size_t, bool, unsigned,  \
                                               hipStream_t);                                                                                 \
    template hipError_t launch_prime_lwe_modswitch<T>(uint32_t *, const T *, T, int, size_t, size_t, unsigned, hipStream_t);                 \
    template hipError_t launch_prime_pbs_init<T>(T *, const T *, const uint32_t *, T, int, uint32_t, bool, size_t, bool, unsigned,          \
                                                 hipStream_t);                                                                               \
    template hipError_t launch_prime_sample_extract<T>(T *, const T *, T, int, size_t, uint32_t, size_t, unsigned, hipStream_t);
CNTT_PRIME_PBS_INST(uint32_t)
CNTT_PRIME_PBS_INST(uint64_t)
#undef CNTT_PRIME_PBS_INST

}  // namespace cntt
