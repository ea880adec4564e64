// Part of host_prime.hip (included at its end, after host_prime_pbs.inc): the LWE keyswitch of the prime plans and the keyswitch +
// bootstrap call (include/cntt_prime_keyswitch.h) -- the kernel's constants (prime_keyswitch.hpp; launched by prime_keyswitch.hip), what
// the shared host side (keyswitch and keyswitch_bootstrap of lwe_host.hpp) needs to know of these plans, and the C ABI over it.
#include "../../include/cntt_prime_keyswitch.h"
#include "lwe_host.hpp"
#include "prime_keyswitch.hpp"

#pragma GCC visibility push(hidden)

// the constants of prime_keyswitch.hpp: the digit offset of gadget_const, -p^-1 mod R and R^2 mod p for R = 2^(bits of T)
template <class T> static PrimeKsConst<T> prime_ks_const(const PrimePlan<T> *pl, unsigned base_log, unsigned levels) {
    const PrimeGadgetConst<T> G = gadget_const(pl, 1, base_log, levels, CNTT_SRC_PLAIN);
    PrimeKsConst<T> K{};
    K.p = pl->p;
    K.off = G.off;
    K.sh1 = G.sh1;
    K.base_log = base_log;
    K.levels = levels;
    T inv = 1;   // p^-1 mod R by Newton's iteration: the correct bits double in every round
    for (int i = 0; i < 6; ++i) inv = (T)(inv * (T)(2 - (T)(pl->p * inv)));
    K.pinv_neg = (T)(0 - inv);
    const uint64_t r = (uint64_t)((((u128)1) << (sizeof(T) * 8)) % pl->p);
    K.r2 = (T)host::mulmod(r, r, pl->p);
    return K;
}
// the prime plans' bootstrap family with what the keyswitch and the keyswitch + bootstrap call (lwe_host.hpp) need besides
template <class T> struct PrimeKs : PrimePbs<T> {
    static constexpr bool KS_ROWS_GUARD = true;
    static hipError_t launch_keyswitch(const PrimePlan<T> *pl, T *out, const T *in, const T *ksk, size_t lin, size_t lout, size_t row_stride,
                                       unsigned base_log, unsigned levels, size_t batch, hipStream_t st) {
        return launch_prime_keyswitch<T>(out, in, ksk, prime_ks_const(pl, base_log, levels), lin, lout, row_stride, batch, st);
    }
};
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_KS_API(BITS, T, PLAN)                                                                                                     \
    extern "C" int cntt_prime##BITS##_keyswitch_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *ksk, size_t lwe_dim_in,          \
                                                      size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,             \
                                                      size_t batch, cntt_mem_t where, void *stream) {                                        \
        return keyswitch<PrimeKs<T>>(pl, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where,          \
                                     (hipStream_t)stream);                                                                                   \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_keyswitch_bootstrap_batch(                                                                             \
        const PLAN *pl, T *lwe_out, const T *lwe_in, const T *ksk, size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const T *lut, \
        int lut_per_element, const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,            \
        void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                                                           \
        return keyswitch_bootstrap<PrimeKs<T>>(pl, lwe_out, lwe_in, ksk, row_stride, ks_base_log, ks_levels, lut, lut_per_element, bsk_ntt,  \
                                               lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,                \
                                               (hipStream_t)stream);                                                                         \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_ks_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk,        \
                                                                size_t batch) {                                                              \
        return ks_pbs_workspace_bytes<PrimeKs<T>>(pl, lwe_dim, glwe_dim, levels_bsk, batch);                                                 \
    }

CNTT_PRIME_KS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_KS_API(32, uint32_t, cntt_plan32)
