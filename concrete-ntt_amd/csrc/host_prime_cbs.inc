// Part of host_prime.hip (included at its end, after host_prime_cmux.inc): the circuit bootstrap from LWE bits to GGSW selectors
// (include/cntt_prime_cbs.h) -- the argument checks, the workspace layout, the host-slice path and the C ABI over the kernels of
// prime_cbs.hpp (launched by prime_cbs.hip) and blind_rotate_device<PrimePbs<T>>, which it calls and does not change.
#include "../../include/cntt_prime_cbs.h"
#include "prime_cbs.hpp"

#pragma GCC visibility push(hidden)

// the six parts of the workspace, in bytes and in this order (cntt_prime_cbs.h states the formula)
struct CbsSizes {
    size_t rot, table, pbs_digits, acc, ks_digits, part;
    CbsShape shape;
    size_t total() const { return up256(rot) + up256(table) + up256(pbs_digits) + up256(acc) + up256(ks_digits) + up256(part); }
};
template <class T>
static CbsSizes cbs_sizes(const PrimePlan<T> *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels, size_t batch) {
    const size_t e = batch * cbs_levels, r = (k * pl->n + 1) * ks_levels, ct = (k + 1) * pl->n * sizeof(T);
    CbsSizes Z;
    Z.shape = prime_cbs_shape(pl->n, sizeof(T), k, r, e);
    Z.rot = (lwe_dim + 1) * e * sizeof(uint32_t);
    Z.table = e * ct;
    Z.pbs_digits = e * ct * pbs_levels;
    Z.acc = e * ct;
    Z.ks_digits = e * r * sizeof(int32_t);
    Z.part = Z.shape.slabs * (k + 1) * e * ct;
    return Z;
}
template <class T>
static size_t cbs_workspace_bytes(const PrimePlan<T> *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                                  size_t batch) {
    return pl ? cbs_sizes(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch).total() : 0;
}

// one of the three gadgets: `name` is the prefix of its two arguments
static int cbs_check_gadget(const char *name, unsigned base_log, unsigned levels, unsigned wbits) {
    if (base_log == 0) return fail(CNTT_EINVAL, "%sbase_log is 0", name);
    if (levels == 0) return fail(CNTT_EINVAL, "%slevels is 0", name);
    if ((uint64_t)base_log * levels > wbits)
        return fail(CNTT_EINVAL, "%sbase_log * %slevels = %u * %u exceeds the bit length %u of the modulus", name, name, base_log, levels, wbits);
    return CNTT_OK;
}

// set-up -> one blind rotation over the E = batch * cbs_levels elements -> extraction and signed digits -> the digit x key product in
// slabs -> the sum of the slabs, negated, in the selector layout.  ws holds rot | table | digits of the rotation | acc | int32 digits |
// slab partials (CbsSizes).
template <class T>
static int circuit_bootstrap_device(const PrimePlan<T> *pl, T *out, const T *lwe_in, const T *bsk, const T *fpksk, size_t lwe_dim, size_t k,
                                    unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log,
                                    unsigned cbs_levels, size_t batch, const CbsSizes &Z, char *ws, hipStream_t st) {
    const size_t e = batch * cbs_levels, n = pl->n, r = (k * n + 1) * ks_levels;
    char *at = ws;
    const auto part_of = [&at](size_t bytes) {
        char *here = at;
        at += up256(bytes);
        return static_cast<void *>(here);
    };
    uint32_t *rot_t = static_cast<uint32_t *>(part_of(Z.rot));
    T *table = static_cast<T *>(part_of(Z.table)), *pbs_digits = static_cast<T *>(part_of(Z.pbs_digits)), *acc = static_cast<T *>(part_of(Z.acc));
    int32_t *ks_digits = static_cast<int32_t *>(part_of(Z.ks_digits));
    T *part = static_cast<T *>(part_of(Z.part));

    PrimeCbsSetup<T> C{};
    C.p = pl->p;
    C.q4 = (T)(((u128)pl->p + 2) / 4);
    C.half_inv = (T)(pl->p / 2 + 1);
    C.logn = (uint32_t)pl->logn;
    C.k = (uint32_t)k;
    C.wbits = modulus_bits(pl);
    C.cbs_base_log = cbs_base_log;
    C.cbs_levels = cbs_levels;
    hipError_t err = launch_prime_cbs_setup<T>(rot_t, table, lwe_in, C, lwe_dim, e, ew_grid((lwe_dim + 1) * e + Z.table / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_setup_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = blind_rotate_device<PrimePbs<T>>(pl, acc, table, true, rot_t, bsk, lwe_dim, k, pbs_base_log, pbs_levels, e, pbs_digits, st)) return rc;
    err = launch_prime_cbs_extract<T>(ks_digits, acc, prime_pack_const(pl, ks_base_log, ks_levels), C, e, ew_grid(e * (k * n + 1)), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_extract_kernel launch failed: %s", hipGetErrorString(err));
    // |slab sum| <= rows 2^(ks_base_log - 1) (2^W - 1) < 2^bits
    unsigned rows_bits = 0;
    while ((Z.shape.rows >> rows_bits) != 0) ++rows_bits;
    const unsigned bits = C.wbits + ks_base_log - 1 + rows_bits;
    err = launch_prime_cbs_ks<T>(part, ks_digits, fpksk, pl->p, pl->logn, k, r, e, Z.shape, bits, st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_ks_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_prime_cbs_sum<T>(out, part, pl->p, pl->logn, k, cbs_levels, e, Z.shape.slabs, ew_grid((k + 1) * Z.acc / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_sum_kernel launch failed: %s", hipGetErrorString(err));
    return CNTT_OK;
}

template <class T>
static int circuit_bootstrap(const PrimePlan<T> *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim, size_t k,
                             unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log,
                             unsigned cbs_levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    const unsigned wbits = modulus_bits(pl);
    if (int rc = cbs_check_gadget("pbs_", pbs_base_log, pbs_levels, wbits)) return rc;
    if (int rc = cbs_check_gadget("ks_", ks_base_log, ks_levels, wbits)) return rc;
    if (ks_base_log > 31) return fail(CNTT_EINVAL, "ks_base_log = %u is above 31: a signed digit must fit an int32", ks_base_log);
    if (int rc = cbs_check_gadget("cbs_", cbs_base_log, cbs_levels, wbits)) return rc;
    if (pl->logn > PrimePbs<T>::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t n = pl->n;
    if (((u128)k * n + 1) * ks_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "(glwe_dim * n + 1) * ks_levels = (%zu * %zu + 1) * %u is not below 2^32 key rows", k, n, ks_levels);
    const size_t r = (k * n + 1) * ks_levels;
    // what the widest launch holds: the external product of the rotation over all E = batch * cbs_levels elements
    if ((u128)batch * cbs_levels * (k + 1) * pbs_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * cbs_levels * (glwe_dim + 1) * pbs_levels = %zu * %u * %zu * %u is not below 2^32: too large for one launch", batch,
                    cbs_levels, k + 1, pbs_levels);
    const size_t e = batch * cbs_levels;
    // the byte counts are products of the arguments: they must fit before they are formed (2048 = the most slabs the shape rule gives)
    if (cmux_passes_2_63({batch, lwe_dim + 1, sizeof(T)}) || lwe_dim + 1 == 0 || cmux_passes_2_63({lwe_dim + 1, e, (size_t)4}) ||
        cmux_passes_2_63({lwe_dim, k + 1, (size_t)pbs_levels, k + 1, n, sizeof(T)}) || cmux_passes_2_63({k + 1, r, k + 1, n, sizeof(T)}) ||
        cmux_passes_2_63({e, k + 1, (size_t)pbs_levels, n, sizeof(T)}) || cmux_passes_2_63({e, r, (size_t)4}) ||
        cmux_passes_2_63({(size_t)2048, k + 1, e, k + 1, n, sizeof(T)}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the keys, the selectors or the workspace pass 2^63 bytes",
                    lwe_dim, k, batch);
    if (batch == 0) return CNTT_OK;
    if (!ggsw_ntt_out) return fail(CNTT_EINVAL, "ggsw_ntt_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim && !bsk_ntt) return fail(CNTT_EINVAL, "bsk_ntt is NULL");
    if (!fpksk_ntt) return fail(CNTT_EINVAL, "fpksk_ntt is NULL");
    const CbsSizes Z = cbs_sizes(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const size_t ob = e * (k + 1) * (k + 1) * n * sizeof(T), ib = batch * (lwe_dim + 1) * sizeof(T),
                 bb = lwe_dim * (k + 1) * pbs_levels * (k + 1) * n * sizeof(T), fb = (k + 1) * r * (k + 1) * n * sizeof(T);
    const Operand ops[5] = {{"ggsw_ntt_out", ggsw_ntt_out, ob, sizeof(T), true},
                            {"lwe_in", lwe_in, ib, sizeof(T), false},
                            {"bsk_ntt", lwe_dim ? bsk_ntt : nullptr, bb, sizeof(T), false},
                            {"fpksk_ntt", fpksk_ntt, fb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    Staging s(where, st);
    const T *din = (const T *)s.in(lwe_in, ib), *dbsk = lwe_dim ? (const T *)s.in(bsk_ntt, bb) : nullptr, *dfk = (const T *)s.in(fpksk_ntt, fb);
    T *dout = (T *)s.out(ggsw_ntt_out, ob);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = circuit_bootstrap_device<T>(pl, dout, din, dbsk, dfk, lwe_dim, k, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log,
                                             cbs_levels, batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_CBS_API(BITS, T, PLAN)                                                                                                    \
    extern "C" int cntt_prime##BITS##_circuit_bootstrap_batch(                                                                               \
        const PLAN *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,             \
        unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels,    \
        size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                                             \
        return circuit_bootstrap<T>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,  \
                                    ks_levels, cbs_base_log, cbs_levels, batch, workspace, workspace_bytes, where, (hipStream_t)stream);     \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_circuit_bootstrap_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim,                  \
                                                                           unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,    \
                                                                           size_t batch) {                                                   \
        return cbs_workspace_bytes<T>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch);                                      \
    }

CNTT_PRIME_CBS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_CBS_API(32, uint32_t, cntt_plan32)

extern "C" unsigned cntt_prime_cbs_grid(size_t items, int logn, size_t word_bytes) { return prime_cbs_grid(items, logn, word_bytes); }
