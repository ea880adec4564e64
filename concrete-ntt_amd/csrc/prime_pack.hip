// kernel instantiations and the launchers of the prime plans' packing keyswitch (prime_pack.hpp): u32 / u64 words
#include "prime_pack.hpp"

namespace cntt {

template <class T>
hipError_t launch_prime_pack_decompose(T *terms, const T *in, const PrimePackConst<T> &G, int logn, size_t lin, size_t m, size_t i0, size_t nw,
                                       size_t batch, hipStream_t st) {
    constexpr size_t TT = PPACK_TT, TI = PPACK_TI;
    if (G.levels == 0 || G.base_log == 0 || (uint64_t)G.base_log * G.levels > sizeof(T) * 8 || batch == 0 || nw == 0 ||
        nw >= ((size_t)1 << 32) || i0 + nw > lin || m == 0 || m > ((size_t)1 << logn))
        return hipErrorInvalidValue;
    const size_t n = (size_t)1 << logn, tiles = batch * ((n + TT - 1) / TT) * ((nw + TI - 1) / TI);
    const unsigned grid = (unsigned)(tiles < ((size_t)1 << 24) ? tiles : ((size_t)1 << 24) - 1);
    hipLaunchKernelGGL((prime_pack_decompose_kernel<T>), dim3(grid), dim3(256), 0, st, terms, in, G, (uint32_t)logn, lin, m, i0, (uint32_t)nw,
                       batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_pack_body(T *out, const T *in, int logn, size_t glwe_dim, size_t lin, size_t m, size_t batch, unsigned grid,
                                  hipStream_t st) {
    if (batch == 0 || m == 0 || m > ((size_t)1 << logn)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((prime_pack_body_kernel<T>), dim3(grid), dim3(256), 0, st, out, in, (uint32_t)logn, glwe_dim, lin, m, batch);
    return hipGetLastError();
}

template hipError_t launch_prime_pack_decompose<uint32_t>(uint32_t *, const uint32_t *, const PrimePackConst<uint32_t> &, int, size_t, size_t,
                                                          size_t, size_t, size_t, hipStream_t);
template hipError_t launch_prime_pack_decompose<uint64_t>(uint64_t *, const uint64_t *, const PrimePackConst<uint64_t> &, int, size_t, size_t,
                                                          size_t, size_t, size_t, hipStream_t);
template hipError_t launch_prime_pack_body<uint32_t>(uint32_t *, const uint32_t *, int, size_t, size_t, size_t, size_t, unsigned, hipStream_t);
template hipError_t launch_prime_pack_body<uint64_t>(uint64_t *, const uint64_t *, int, size_t, size_t, size_t, size_t, unsigned, hipStream_t);

}  // namespace cntt
