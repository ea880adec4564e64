// kernel instantiations and the launchers of the prime plans' ring packing (prime_ring_pack.hpp): u32 / u64 words
#include "prime_ring_pack.hpp"

namespace cntt {

// t^-1 mod 2n for odd t: Newton's iteration doubles the correct low bits (t t = 1 mod 8 to start with)
static uint32_t inverse_mod_2n(uint32_t t, int logn) {
    uint32_t x = t;
    for (int i = 0; i < 5; ++i) x *= 2u - t * x;
    return x & ((2u << logn) - 1u);
}

template <class T> hipError_t launch_prime_glwe_embed(T *glwe, const T *lwe, T p, int logn, size_t glwe_dim, size_t batch, hipStream_t st) {
    if (logn < 4 || logn > 30 || batch == 0 || glwe_dim + 1 >= ((size_t)1 << 32)) return hipErrorInvalidValue;
    const dim3 grid(prime_ring_pack_grid(batch * (glwe_dim + 1), logn, sizeof(T))), block(256);
    hipLaunchKernelGGL((prime_glwe_embed_kernel<T>), grid, block, 0, st, glwe, lwe, p, (uint32_t)logn, (uint32_t)glwe_dim, batch);
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_ring_merge(T *terms, T *out, const T *even, const T *odd, bool leaf, const PrimePackConst<T> &G, uint32_t t, uint32_t shift,
                                   int logn, size_t glwe_dim, size_t h, size_t gs, size_t nct, bool stream, bool lds, hipStream_t st) {
    if (logn < 4 || logn > 30 || (t & 1u) == 0 || t >= (2u << logn) || shift >= (2u << logn) || nct == 0 || h == 0 || nct % h || gs < h ||
        glwe_dim + 1 >= ((size_t)1 << 32) || G.levels == 0 || G.base_log == 0 || (uint64_t)G.base_log * G.levels > sizeof(T) * 8)
        return hipErrorInvalidValue;
    const size_t bytes = (2 * sizeof(T)) << logn;
    const bool use_lds = lds && bytes <= AUTOM_LDS_BYTES;
    const dim3 grid(prime_ring_pack_grid(nct * (glwe_dim + 1), logn, sizeof(T))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = inverse_mod_2n(t, logn), ln = (uint32_t)logn, k = (uint32_t)glwe_dim;
#define CNTT_RING_LAUNCH(STREAM, LDS)                                                                                                        \
    do {                                                                                                                                     \
        if (leaf)                                                                                                                            \
            hipLaunchKernelGGL((prime_ring_merge_kernel<T, STREAM, LDS, true>), grid, block, shm, st, terms, out, even, odd, G, tinv, shift, \
                               ln, k, h, gs, nct);                                                                                           \
        else                                                                                                                                 \
            hipLaunchKernelGGL((prime_ring_merge_kernel<T, STREAM, LDS, false>), grid, block, shm, st, terms, out, even, odd, G, tinv,       \
                               shift, ln, k, h, gs, nct);                                                                                    \
    } while (0)
    if (stream && use_lds) CNTT_RING_LAUNCH(true, true);
    else if (stream) CNTT_RING_LAUNCH(true, false);
    else if (use_lds) CNTT_RING_LAUNCH(false, true);
    else CNTT_RING_LAUNCH(false, false);
#undef CNTT_RING_LAUNCH
    return hipGetLastError();
}

#define CNTT_PRIME_RING_INST(T)                                                                                                              \
    template hipError_t launch_prime_glwe_embed<T>(T *, const T *, T, int, size_t, size_t, hipStream_t);                                     \
    template hipError_t launch_prime_ring_merge<T>(T *, T *, const T *, const T *, bool, const PrimePackConst<T> &, uint32_t, uint32_t, int, \
                                                   size_t, size_t, size_t, size_t, bool, bool, hipStream_t);
CNTT_PRIME_RING_INST(uint32_t)
CNTT_PRIME_RING_INST(uint64_t)
#undef CNTT_PRIME_RING_INST

}  // namespace cntt
