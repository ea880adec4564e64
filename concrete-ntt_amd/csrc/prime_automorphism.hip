// kernel instantiations and the launchers of the prime plans' ring automorphism (prime_automorphism.hpp): u32 / u64 words
#include "prime_automorphism.hpp"

namespace cntt {

// t^-1 mod 2n for odd t: Newton's iteration doubles the correct low bits (t t = 1 mod 8 to start with)
static uint32_t inverse_mod_2n(uint32_t t, int logn) {
    uint32_t x = t;
    for (int i = 0; i < 5; ++i) x *= 2u - t * x;
    return x & ((2u << logn) - 1u);
}

template <class T>
hipError_t launch_prime_automorphism(T *out, const T *in, T p, uint32_t t, bool ntt, int logn, size_t npoly_total, bool stream, bool lds,
                                     hipStream_t st) {
    if (logn < 4 || logn > 30 || (t & 1u) == 0 || t >= (2u << logn) || npoly_total == 0) return hipErrorInvalidValue;
    const size_t bytes = sizeof(T) << logn;
    const bool use_lds = lds && bytes <= AUTOM_LDS_BYTES;
    const dim3 grid(prime_automorphism_grid(npoly_total, logn, sizeof(T))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = inverse_mod_2n(t, logn), ln = (uint32_t)logn;
#define CNTT_AUTOM_LAUNCH(STREAM, LDS)                                                                                                       \
    do {                                                                                                                                     \
        if (ntt) hipLaunchKernelGGL((prime_automorphism_ntt_kernel<T, STREAM, LDS>), grid, block, shm, st, out, in, t, ln, npoly_total);     \
        else hipLaunchKernelGGL((prime_automorphism_kernel<T, STREAM, LDS>), grid, block, shm, st, out, in, p, tinv, ln, npoly_total);       \
    } while (0)
    if (stream && use_lds) CNTT_AUTOM_LAUNCH(true, true);
    else if (stream) CNTT_AUTOM_LAUNCH(true, false);
    else if (use_lds) CNTT_AUTOM_LAUNCH(false, true);
    else CNTT_AUTOM_LAUNCH(false, false);
#undef CNTT_AUTOM_LAUNCH
    return hipGetLastError();
}

template <class T>
hipError_t launch_prime_automorphism_gadget(T *terms, T *out, const T *in, const PrimePackConst<T> &G, uint32_t t, int logn, size_t glwe_dim,
                                            bool add_input, size_t batch, bool stream, bool lds, hipStream_t st) {
    if (logn < 4 || logn > 30 || (t & 1u) == 0 || t >= (2u << logn) || batch == 0 || glwe_dim + 1 >= ((size_t)1 << 32) || G.levels == 0 ||
        G.base_log == 0 || (uint64_t)G.base_log * G.levels > sizeof(T) * 8)
        return hipErrorInvalidValue;
    const size_t bytes = sizeof(T) << logn;
    const bool use_lds = lds && bytes <= AUTOM_LDS_BYTES;
    const dim3 grid(prime_automorphism_grid(batch * (glwe_dim + 1), logn, sizeof(T))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = inverse_mod_2n(t, logn), ln = (uint32_t)logn, k = (uint32_t)glwe_dim, add = add_input ? 1u : 0u;
#define CNTT_AUTOM_LAUNCH(STREAM, LDS)                                                                                                       \
    hipLaunchKernelGGL((prime_automorphism_gadget_kernel<T, STREAM, LDS>), grid, block, shm, st, terms, out, in, G, tinv, ln, k, add, batch)
    if (stream && use_lds) CNTT_AUTOM_LAUNCH(true, true);
    else if (stream) CNTT_AUTOM_LAUNCH(true, false);
    else if (use_lds) CNTT_AUTOM_LAUNCH(false, true);
    else CNTT_AUTOM_LAUNCH(false, false);
#undef CNTT_AUTOM_LAUNCH
    return hipGetLastError();
}

#define CNTT_PRIME_AUTOM_INST(T)                                                                                                             \
    template hipError_t launch_prime_automorphism<T>(T *, const T *, T, uint32_t, bool, int, size_t, bool, bool, hipStream_t);               \
    template hipError_t launch_prime_automorphism_gadget<T>(T *, T *, const T *, const PrimePackConst<T> &, uint32_t, int, size_t, bool,    \
                                                            size_t, bool, bool, hipStream_t);
CNTT_PRIME_AUTOM_INST(uint32_t)
CNTT_PRIME_AUTOM_INST(uint64_t)
#undef CNTT_PRIME_AUTOM_INST

}  // namespace cntt
