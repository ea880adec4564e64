// Part of host_prime.hip (included at its end, after host_prime_cmux.inc): the prime plans' side of the circuit bootstrap from LWE bits to
// GGSW selectors (include/cntt_prime_cbs.h), of the many-LUT bootstrap and of the circuit bootstrap with one rotation per input bit
// (include/cntt_prime_manylut.h) -- the members of PrimePbs<T> that need more than a line, over the kernels of prime_cbs.hpp and
// prime_manylut.hpp (launched by prime_cbs.hip and prime_manylut.hip), and the C ABI.  The checks, the workspace and the launch sequences
// are cbs_host.hpp's, shared with the native plans.
#include "../../include/cntt_prime_cbs.h"
#include "../../include/cntt_prime_manylut.h"
#include "prime_cbs.hpp"
#include "prime_manylut.hpp"

#pragma GCC visibility push(hidden)

template <class T> PrimeCbsSetup<T> PrimePbs<T>::cbs_const(const Plan *pl, size_t k, unsigned cbs_base_log, unsigned cbs_levels) {
    PrimeCbsSetup<T> C{};
    C.p = pl->p;
    C.q4 = (T)(((u128)pl->p + 2) / 4);
    C.half_inv = (T)(pl->p / 2 + 1);
    C.logn = (uint32_t)pl->logn;
    C.k = (uint32_t)k;
    C.wbits = modulus_bits(pl);
    C.cbs_base_log = cbs_base_log;
    C.cbs_levels = cbs_levels;
    return C;
}
template <class T>
hipError_t PrimePbs<T>::launch_cbs_setup(const Plan *, uint32_t *rot_t, T *table, const T *lwe, const CbsConst &C, const unsigned *log_lut,
                                         size_t lwe_dim, size_t rotations, unsigned grid, hipStream_t st) {
    if (log_lut) return launch_prime_cbs_manylut_setup<T>(rot_t, table, lwe, C, *log_lut, lwe_dim, rotations, grid, st);
    return launch_prime_cbs_setup<T>(rot_t, table, lwe, C, lwe_dim, rotations, grid, st);
}
template <class T>
hipError_t PrimePbs<T>::launch_cbs_extract(const Plan *pl, int32_t *digits, const T *acc, unsigned ks_base_log, unsigned ks_levels,
                                           const CbsConst &C, bool one_rotation, size_t rotations, unsigned grid, hipStream_t st) {
    return (one_rotation ? launch_prime_cbs_manylut_extract<T> : launch_prime_cbs_extract<T>)(digits, acc, prime_pack_const(pl, ks_base_log, ks_levels),
                                                                                              C, rotations, grid, st);
}
template <class T>
hipError_t PrimePbs<T>::launch_cbs_ks(const Plan *pl, T *part, const int32_t *digits, const T *fpksk, size_t k, size_t rows, size_t elements,
                                      const CbsShape &shape, unsigned ks_base_log, hipStream_t st) {
    // |slab sum| <= rows 2^(ks_base_log - 1) (2^W - 1) < 2^bits
    unsigned rows_bits = 0;
    while ((shape.rows >> rows_bits) != 0) ++rows_bits;
    const unsigned bits = modulus_bits(pl) + ks_base_log - 1 + rows_bits;
    return launch_prime_cbs_ks<T>(part, digits, fpksk, pl->p, pl->logn, k, rows, elements, shape, bits, st);
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_CBS_API(BITS, T, PLAN)                                                                                                    \
    extern "C" int cntt_prime##BITS##_circuit_bootstrap_batch(                                                                               \
        const PLAN *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,             \
        unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels,    \
        size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                                             \
        return circuit_bootstrap<PrimePbs<T>>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels,     \
                                              ks_base_log, ks_levels, cbs_base_log, cbs_levels, nullptr, batch, workspace, workspace_bytes,  \
                                              where, (hipStream_t)stream);                                                                   \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_circuit_bootstrap_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim,                  \
                                                                           unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,    \
                                                                           size_t batch) {                                                   \
        return cbs_workspace_bytes<PrimePbs<T>>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch, false);                     \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_lwe_modswitch_manylut_batch(const PLAN *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim,             \
                                                                  unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream) {   \
        return lwe_modswitch_manylut<PrimePbs<T>>(pl, rot_t, lwe, lwe_dim, log_lut_count, batch, where, (hipStream_t)stream);                \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_sample_extract_many_batch(const PLAN *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t count,    \
                                                                size_t batch, cntt_mem_t where, void *stream) {                              \
        return sample_extract_many<PrimePbs<T>>(pl, lwe_out, glwe, glwe_dim, count, batch, where, (hipStream_t)stream);                      \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_bootstrap_manylut_batch(                                                                               \
        const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element, const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim,   \
        unsigned base_log, unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch, void *workspace, size_t workspace_bytes, \
        cntt_mem_t where, void *stream) {                                                                                                    \
        return bootstrap_manylut<PrimePbs<T>>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels,       \
                                              log_lut_count, lut_count, batch, workspace, workspace_bytes, where, (hipStream_t)stream);      \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_circuit_bootstrap_manylut_batch(                                                                       \
        const PLAN *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,             \
        unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels,    \
        unsigned log_lut_count, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                     \
        return circuit_bootstrap<PrimePbs<T>>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels,     \
                                              ks_base_log, ks_levels, cbs_base_log, cbs_levels, &log_lut_count, batch, workspace,            \
                                              workspace_bytes, where, (hipStream_t)stream);                                                  \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_circuit_bootstrap_manylut_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim,          \
                                                                                   unsigned pbs_levels, unsigned ks_levels,                 \
                                                                                   unsigned cbs_levels, size_t batch) {                      \
        return cbs_workspace_bytes<PrimePbs<T>>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch, true);                      \
    }

CNTT_PRIME_CBS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_CBS_API(32, uint32_t, cntt_plan32)

extern "C" unsigned cntt_prime_cbs_grid(size_t items, int logn, size_t word_bytes) { return prime_cbs_grid(items, logn, word_bytes); }
