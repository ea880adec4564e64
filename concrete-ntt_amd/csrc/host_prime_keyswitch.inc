// Part of host_prime.hip (included at its end, after host_prime_pbs.inc): the LWE keyswitch of the prime plans and the keyswitch +
// bootstrap call (include/cntt_prime_keyswitch.h) -- argument checks, the kernel's constants and its launch (prime_keyswitch.hpp; launched
// by prime_keyswitch.hip), the host-slice path, and the C ABI.  The combined call is keyswitch_bootstrap of pbs_host.hpp.
#include "../../include/cntt_prime_keyswitch.h"
#include "prime_keyswitch.hpp"

#pragma GCC visibility push(hidden)

// the digit and stride checks the two calls share; `pre` = "" or "ks_": how the combined call names the keyswitch's digit arguments
template <class T>
static int prime_ks_check(const PrimePlan<T> *pl, size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,
                          const char *pre) {
    const unsigned wbits = modulus_bits(pl);
    if (base_log == 0) return fail(CNTT_EINVAL, "%sbase_log is 0", pre);
    if (levels == 0) return fail(CNTT_EINVAL, "%slevels is 0", pre);
    if ((uint64_t)base_log * levels > wbits)
        return fail(CNTT_EINVAL, "%sbase_log * %slevels = %u * %u exceeds the bit length %u of the modulus", pre, pre, base_log, levels, wbits);
    if (base_log > 31) return fail(CNTT_EINVAL, "%sbase_log = %u exceeds 31: the keyswitch keeps a digit in one 32-bit register", pre, base_log);
    if (row_stride < lwe_dim_out + 1)
        return fail(CNTT_EINVAL, "row_stride = %zu is below lwe_dim_out + 1 = %zu words", row_stride, lwe_dim_out + 1);
    if ((u128)lwe_dim_in * levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "lwe_dim_in * %slevels = %zu * %u is not below 2^32 key rows", pre, lwe_dim_in, levels);
    return CNTT_OK;
}
// bytes of a key of `rows` rows: the last row needs its lwe_dim_out + 1 words only
template <class T> static size_t prime_ksk_bytes(const PrimePlan<T> *, size_t rows, size_t lwe_dim_out, size_t row_stride) {
    return rows ? ((rows - 1) * row_stride + lwe_dim_out + 1) * sizeof(T) : 0;
}
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
template <class T>
static int prime_keyswitch_device(const PrimePlan<T> *pl, T *out, const T *in, const T *ksk, size_t lin, size_t lout, size_t row_stride,
                                  unsigned base_log, unsigned levels, size_t batch, hipStream_t st) {
    const hipError_t e = launch_prime_keyswitch<T>(out, in, ksk, prime_ks_const(pl, base_log, levels), lin, lout, row_stride, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_keyswitch_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

template <class T>
static int prime_keyswitch(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *ksk, size_t lwe_dim_in, size_t lwe_dim_out,
                           size_t row_stride, unsigned base_log, unsigned levels, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = prime_ks_check(pl, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, "")) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim_in && !ksk) return fail(CNTT_EINVAL, "ksk is NULL");
    const size_t ob = batch * (lwe_dim_out + 1) * sizeof(T), ib = batch * (lwe_dim_in + 1) * sizeof(T);
    const size_t kb = prime_ksk_bytes(pl, lwe_dim_in * levels, lwe_dim_out, row_stride);
    if (ranges_overlap(lwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "lwe_out overlaps lwe_in");
    if (ranges_overlap(lwe_out, ob, ksk, kb)) return fail(CNTT_EINVAL, "lwe_out overlaps ksk");
    if (where == CNTT_MEM_DEVICE)
        return prime_keyswitch_device(pl, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, st);
    Staging s(st);
    T *dout = (T *)s.out(lwe_out, ob);
    const T *din = (const T *)s.in(lwe_in, ib), *dk = (const T *)s.in(ksk, kb);
    if (int rc = s.status()) return rc;
    if (int rc = prime_keyswitch_device(pl, dout, din, dk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, st)) return rc;
    return s.finish();
}

// the prime plans' bootstrap family with the keyswitch keyswitch_bootstrap (pbs_host.hpp) puts in front of it
template <class T> struct PrimeKsPbs : PrimePbs<T> {
    static constexpr auto ks_check = prime_ks_check<T>;
    static constexpr auto ks_key_bytes = prime_ksk_bytes<T>;
    static constexpr auto ks_device = prime_keyswitch_device<T>;
};
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_KS_API(BITS, T, PLAN)                                                                                                     \
    extern "C" int cntt_prime##BITS##_keyswitch_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *ksk, size_t lwe_dim_in,           \
                                                      size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,             \
                                                      size_t batch, cntt_mem_t where, void *stream) {                                        \
        return prime_keyswitch<T>(pl, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where,              \
                                  (hipStream_t)stream);                                                                                       \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_keyswitch_bootstrap_batch(                                                                             \
        const PLAN *pl, T *lwe_out, const T *lwe_in, const T *ksk, size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const T *lut, \
        int lut_per_element, const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,            \
        void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                                                           \
        return keyswitch_bootstrap<PrimeKsPbs<T>>(pl, lwe_out, lwe_in, ksk, row_stride, ks_base_log, ks_levels, lut, lut_per_element,         \
                                                  bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,    \
                                                  (hipStream_t)stream);                                                                       \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_ks_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk,         \
                                                                size_t batch) {                                                              \
        return ks_pbs_workspace_bytes<PrimeKsPbs<T>>(pl, lwe_dim, glwe_dim, levels_bsk, batch);                                               \
    }

CNTT_PRIME_KS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_KS_API(32, uint32_t, cntt_plan32)
