// Part of host_prime.hip (included at its end, after host_prime_keyswitch.inc): the LWE-to-GLWE packing keyswitch of the prime plans
// (include/cntt_prime_pack.h) -- argument checks, the constants and the launches of the two kernels (prime_pack.hpp; launched by
// prime_pack.hip), the loop over external_product_device above (which it calls and does not change), the host-slice path, and the C ABI.
#include "../../include/cntt_prime_pack.h"
#include "prime_pack.hpp"

#pragma GCC visibility push(hidden)

// mask words of one external product: C of the header, capped at lin (levels >= 1)
static size_t prime_pack_chunk(size_t lin, unsigned levels) {
    return std::min(std::max<size_t>(1, CNTT_PRIME_PACK_TERMS / levels), lin);
}
template <class T> static size_t prime_pack_workspace(const PrimePlan<T> *pl, size_t lin, unsigned levels, size_t batch) {
    return pl && levels ? up256(batch * prime_pack_chunk(lin, levels) * levels * pl->n * sizeof(T)) : 0;
}
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

// out = the body polynomial, then per chunk of mask words the negated digit polynomials into `terms` and the external product
// accumulating into out.  In place is sound as in blind_rotate_device (pbs_host.hpp): a chunk's terms are complete before its product starts
// and rewritten only after it (stream order), and the product reads only the terms and the key.
template <class T>
static int prime_pack_device(const PrimePlan<T> *pl, T *out, const T *in, const T *pksk, size_t lin, size_t m, size_t glwe_dim,
                             unsigned base_log, unsigned levels, size_t batch, T *terms, hipStream_t st) {
    const size_t npolys = glwe_dim + 1, n = pl->n, chunk = prime_pack_chunk(lin, levels);
    hipError_t e = launch_prime_pack_body<T>(out, in, pl->logn, glwe_dim, lin, m, batch, ew_grid(batch * npolys * n), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_pack_body_kernel launch failed: %s", hipGetErrorString(e));
    const PrimePackConst<T> K = prime_pack_const(pl, base_log, levels);
    for (size_t i0 = 0; i0 < lin; i0 += chunk) {
        const size_t nw = std::min(chunk, lin - i0);
        e = launch_prime_pack_decompose<T>(terms, in, K, pl->logn, lin, m, i0, nw, batch, st);
        if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_pack_decompose_kernel launch failed: %s", hipGetErrorString(e));
        if (int rc = external_product_device<T>(pl, out, terms, pksk + i0 * levels * npolys * n, nw * levels, npolys, batch, true, st)) return rc;
    }
    return CNTT_OK;
}

template <class T>
static int prime_pack_keyswitch(const PrimePlan<T> *pl, T *glwe_out, const T *lwe_in, const T *pksk_ntt, size_t lwe_dim_in, size_t lwe_count,
                                size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check<PrimePbs<T>>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (lwe_count == 0 || lwe_count > pl->n)
        return fail(CNTT_EINVAL, "lwe_count = %zu is not in 1 .. ntt_size = %zu", lwe_count, pl->n);
    if (glwe_dim >= ((size_t)1 << 32) - 1) return fail(CNTT_EINVAL, "glwe_dim too large");   // (glwe_dim + 1 would wrap at SIZE_MAX)
    if ((u128)lwe_dim_in * levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "lwe_dim_in * levels = %zu * %u is not below 2^32 key rows", lwe_dim_in, levels);
    // the byte counts below -- ciphertexts, key, output -- are products of the arguments: they must fit a size_t before they are formed
    // (lwe_dim_in < 2^32, glwe_dim + 1 < 2^32 and lwe_count <= n keep the 128-bit products themselves from wrapping)
    const u128 lim = (u128)1 << 63, wb = sizeof(T);
    if ((u128)batch * lwe_count * (lwe_dim_in + 1) * wb >= lim || (u128)batch * (glwe_dim + 1) * pl->n * wb >= lim ||
        (u128)lwe_dim_in * levels * (glwe_dim + 1) * pl->n * wb >= lim)
        return fail(CNTT_EINVAL, "lwe_dim_in = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the key or the output pass 2^63 bytes", lwe_dim_in,
                    glwe_dim, batch);
    // what external_product_device would refuse halfway through the call
    const size_t launch = std::max<size_t>(prime_pack_chunk(lwe_dim_in, levels) * levels, glwe_dim + 1);
    if ((u128)batch * launch >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * max(C * levels, glwe_dim + 1) = %zu * %zu is not below 2^32: too large for one launch", batch, launch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim_in && !pksk_ntt) return fail(CNTT_EINVAL, "pksk_ntt is NULL");
    const size_t n = pl->n, w = sizeof(T), ob = batch * (glwe_dim + 1) * n * w, ib = batch * lwe_count * (lwe_dim_in + 1) * w;
    const size_t kb = lwe_dim_in * levels * (glwe_dim + 1) * n * w, need = prime_pack_workspace(pl, lwe_dim_in, levels, batch);
    if (ranges_overlap(glwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "glwe_out overlaps lwe_in");
    if (ranges_overlap(glwe_out, ob, pksk_ntt, kb)) return fail(CNTT_EINVAL, "glwe_out overlaps pksk_ntt");
    if (workspace) {
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
        if (ranges_overlap(glwe_out, ob, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "glwe_out overlaps workspace");
        if (ranges_overlap(lwe_in, ib, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_in overlaps workspace");
    }
    if (where == CNTT_MEM_DEVICE) {
        void *terms = workspace;
        if (!terms && lwe_dim_in) HIP_TRY(hipMallocAsync(&terms, need, st));   // one allocation for the whole call
        const int rc = prime_pack_device<T>(pl, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, (T *)terms, st);
        if (!workspace && terms) (void)hipFreeAsync(terms, st);
        return rc;
    }
    Staging s(st);
    const T *dkey = lwe_dim_in ? (const T *)s.in(pksk_ntt, kb) : nullptr, *din = (const T *)s.in(lwe_in, ib);
    T *dout = (T *)s.out(glwe_out, ob), *dterms = (T *)s.alloc(need);
    if (int rc = s.status()) return rc;
    if (int rc = prime_pack_device<T>(pl, dout, din, dkey, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, dterms, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_PACK_API(BITS, T, PLAN)                                                                                                   \
    extern "C" int cntt_prime##BITS##_pack_keyswitch_batch(const PLAN *pl, T *glwe_out, const T *lwe_in, const T *pksk_ntt, size_t lwe_dim_in, \
                                                           size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels,            \
                                                           size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,          \
                                                           void *stream) {                                                                   \
        return prime_pack_keyswitch<T>(pl, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, workspace,   \
                                       workspace_bytes, where, (hipStream_t)stream);                                                          \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_pack_workspace_bytes(const PLAN *pl, size_t lwe_dim_in, unsigned levels, size_t batch) {             \
        return prime_pack_workspace<T>(pl, lwe_dim_in, levels, batch);                                                                        \
    }

CNTT_PRIME_PACK_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_PACK_API(32, uint32_t, cntt_plan32)
