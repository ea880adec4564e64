// Part of host_prime.hip (included at its end, after host_prime_keyswitch.inc): the LWE-to-GLWE packing keyswitch of the prime plans
// (include/cntt_prime_pack.h) -- the constants of the two kernels (prime_pack.hpp; launched by prime_pack.hip), what the shared host side
// (pack_keyswitch of lwe_host.hpp: the checks, the loop over external_product_device above, the host-slice path) needs to know of these
// plans, among it the refusals only they have, and the C ABI over it.
#include "../../include/cntt_prime_pack.h"
#include "lwe_host.hpp"
#include "prime_pack.hpp"

#pragma GCC visibility push(hidden)

// the constants of prime_pack.hpp, from those of the stand-alone decomposition
template <class T> static PrimePackConst<T> prime_pack_const(const PrimePlan<T> *pl, unsigned base_log, unsigned levels) {
    const PrimeGadgetConst<T> G = gadget_const(pl, 1, base_log, levels, CNTT_SRC_PLAIN);
    PrimePackConst<T> K{};
    K.p = pl->p;
    K.off = G.off;
    K.mask = G.mask;
    K.half = G.half;
    K.sh1 = G.sh1;
    K.base_log = base_log;
    K.levels = levels;
    return K;
}

// the prime plans' bootstrap family with what the packing keyswitch (pack_keyswitch of lwe_host.hpp) needs besides
template <class T> struct PrimePack : PrimePbs<T> {
    using Plan = PrimePlan<T>;
    static size_t pack_chunk_terms(const Plan *) { return CNTT_PRIME_PACK_TERMS; }
    static int pack_check_levels(const Plan *, unsigned) { return CNTT_OK; }   // the sums are taken mod p: any number of levels
    // what the kernels index in 32 bits, and the byte counts -- ciphertexts, key, output -- which are products of the arguments: they must
    // fit a size_t before they are formed
    static int pack_check_sizes(const Plan *pl, size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned levels, size_t batch) {
        if (glwe_dim + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");   // (wrapped at SIZE_MAX, past the shared bound)
        if ((u128)lwe_dim_in * levels >= ((u128)1 << 32))
            return fail(CNTT_EINVAL, "lwe_dim_in * levels = %zu * %u is not below 2^32 key rows", lwe_dim_in, levels);
        // (lwe_dim_in < 2^32, glwe_dim + 1 < 2^32 and lwe_count <= n keep the 128-bit products themselves from wrapping)
        const u128 lim = (u128)1 << 63, wb = sizeof(T);
        if ((u128)batch * lwe_count * (lwe_dim_in + 1) * wb >= lim || (u128)batch * (glwe_dim + 1) * pl->n * wb >= lim ||
            (u128)lwe_dim_in * levels * (glwe_dim + 1) * pl->n * wb >= lim)
            return fail(CNTT_EINVAL, "lwe_dim_in = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the key or the output pass 2^63 bytes",
                        lwe_dim_in, glwe_dim, batch);
        // what external_product_device would refuse halfway through the call
        const size_t launch = std::max<size_t>(pack_chunk<PrimePack>(pl, lwe_dim_in, levels) * levels, glwe_dim + 1);
        if ((u128)batch * launch >= ((u128)1 << 32))
            return fail(CNTT_EINVAL, "batch * max(C * levels, glwe_dim + 1) = %zu * %zu is not below 2^32: too large for one launch", batch, launch);
        return CNTT_OK;
    }
    static bool pack_key_overlaps(const T *out, size_t ob, const T *key, size_t kb) { return ranges_overlap(out, ob, key, kb); }
    static hipError_t launch_pack_body(const Plan *pl, T *out, const T *in, size_t glwe_dim, size_t lin, size_t m, size_t batch, unsigned grid,
                                       hipStream_t st) {
        return launch_prime_pack_body<T>(out, in, pl->logn, glwe_dim, lin, m, batch, grid, st);
    }
    static hipError_t launch_pack_decompose(const Plan *pl, T *terms, const T *in, unsigned base_log, unsigned levels, size_t lin, size_t m,
                                            size_t i0, size_t nw, size_t batch, hipStream_t st) {
        return launch_prime_pack_decompose<T>(terms, in, prime_pack_const(pl, base_log, levels), pl->logn, lin, m, i0, nw, batch, st);
    }
};
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_PACK_API(BITS, T, PLAN)                                                                                                   \
    extern "C" int cntt_prime##BITS##_pack_keyswitch_batch(const PLAN *pl, T *glwe_out, const T *lwe_in, const T *pksk_ntt, size_t lwe_dim_in, \
                                                           size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels,            \
                                                           size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,          \
                                                           void *stream) {                                                                   \
        return pack_keyswitch<PrimePack<T>>(pl, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch,        \
                                            workspace, workspace_bytes, where, (hipStream_t)stream);                                         \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_pack_workspace_bytes(const PLAN *pl, size_t lwe_dim_in, unsigned levels, size_t batch) {            \
        return pack_workspace_bytes<PrimePack<T>>(pl, lwe_dim_in, levels, batch);                                                            \
    }

CNTT_PRIME_PACK_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_PACK_API(32, uint32_t, cntt_plan32)
