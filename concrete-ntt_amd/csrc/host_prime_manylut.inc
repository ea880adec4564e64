// Part of host_prime.hip (included at its end, after host_prime_cbs.inc): the many-LUT bootstrap and the circuit bootstrap with one
// rotation per input bit (include/cntt_prime_manylut.h) -- the argument checks, the workspace layouts, the host-slice path and the C ABI
// over the kernels of prime_manylut.hpp (launched by prime_manylut.hip), blind_rotate_device<PrimePbs<T>> and the functional keyswitch
// of prime_cbs.hpp, which it calls and does not change.
#include "../../include/cntt_prime_manylut.h"
#include "prime_manylut.hpp"

#pragma GCC visibility push(hidden)

template <class T> static int manylut_check_log(const PrimePlan<T> *pl, unsigned log_lut) {
    if (log_lut > (unsigned)pl->logn)
        return fail(CNTT_EINVAL, "log_lut_count = %u exceeds log2(ntt_size) = %d", log_lut, pl->logn);
    if (pl->logn > PrimePbs<T>::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    return CNTT_OK;
}

template <class T>
static int modswitch_manylut_device(const PrimePlan<T> *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, unsigned log_lut, size_t batch,
                                    hipStream_t st) {
    const size_t tiles = ((lwe_dim + PRIME_PBS_TILE) / PRIME_PBS_TILE) * ((batch + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE);
    const hipError_t e = launch_prime_modswitch_manylut<T>(rot_t, lwe, pl->p, pl->logn, log_lut, lwe_dim, batch, ew_grid(tiles * 256), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_modswitch_manylut_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

template <class T>
static int extract_many_device(const PrimePlan<T> *pl, T *lwe_out, const T *glwe, size_t k, size_t count, size_t batch, hipStream_t st) {
    const size_t n = pl->n, chunks = (count + EXM_ROWS - 1) / EXM_ROWS;
    const size_t items = batch * k * chunks * (n * sizeof(T) / 16) + batch * count;
    // the output against STREAM_BYTES, as the other element-wise kernels decide it
    const hipError_t e = launch_prime_sample_extract_many<T>(lwe_out, glwe, pl->p, pl->logn, k, count, batch,
                                                             batch * count * (k * n + 1) * sizeof(T) > STREAM_BYTES, ew_grid(items), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_sample_extract_many_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

template <class T>
static int lwe_modswitch_manylut(const PrimePlan<T> *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, unsigned log_lut, size_t batch,
                                 cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = manylut_check_log(pl, log_lut)) return rc;
    if (cmux_passes_2_63({batch, lwe_dim + 1, sizeof(T)}) || lwe_dim + 1 == 0)
        return fail(CNTT_EINVAL, "lwe_dim = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", lwe_dim, batch);
    if (batch == 0) return CNTT_OK;
    if (!rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (!lwe) return fail(CNTT_EINVAL, "lwe is NULL");
    const size_t rb = (lwe_dim + 1) * batch * sizeof(uint32_t), lb = (lwe_dim + 1) * batch * sizeof(T);
    const Operand ops[2] = {{"rot_t", rot_t, rb, sizeof(uint32_t), true}, {"lwe", lwe, lb, sizeof(T), false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    uint32_t *dr = (uint32_t *)s.out(rot_t, rb);
    const T *dl = (const T *)s.in(lwe, lb);
    if (int rc = s.status()) return rc;
    if (int rc = modswitch_manylut_device<T>(pl, dr, dl, lwe_dim, log_lut, batch, st)) return rc;
    return s.finish();
}

template <class T>
static int sample_extract_many(const PrimePlan<T> *pl, T *lwe_out, const T *glwe, size_t k, size_t count, size_t batch, cntt_mem_t where,
                               hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (count == 0 || count > pl->n) return fail(CNTT_EINVAL, "count = %zu is not in 1 .. ntt_size = %zu", count, pl->n);
    if (k + 1 == 0 || cmux_passes_2_63({batch, count, k, pl->n, sizeof(T)}) || cmux_passes_2_63({batch, count + k + 1, pl->n, sizeof(T)}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, count = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", k, count, batch);
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!glwe) return fail(CNTT_EINVAL, "glwe is NULL");
    const size_t ob = batch * count * (k * pl->n + 1) * sizeof(T), gb = batch * (k + 1) * pl->n * sizeof(T);
    const Operand ops[2] = {{"lwe_out", lwe_out, ob, sizeof(T), true}, {"glwe", glwe, gb, sizeof(T), false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    T *dout = (T *)s.out(lwe_out, ob);
    const T *dg = (const T *)s.in(glwe, gb);
    if (int rc = s.status()) return rc;
    if (int rc = extract_many_device<T>(pl, dout, dg, k, count, batch, st)) return rc;
    return s.finish();
}

// the coarse modulus switch -> the blind rotation -> the extraction of the indices 0 .. lut_count - 1; ws holds digits | rot_t | acc
// (PbsSizes), as bootstrap_device
template <class T>
static int bootstrap_manylut(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element, const T *bsk, size_t lwe_dim,
                             size_t k, unsigned base_log, unsigned levels, unsigned log_lut, size_t lut_count, size_t batch, void *workspace,
                             size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using F = PrimePbs<T>;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = manylut_check_log(pl, log_lut)) return rc;
    if (lut_count == 0 || lut_count > ((size_t)1 << log_lut))
        return fail(CNTT_EINVAL, "lut_count = %zu is not in 1 .. 2^log_lut_count = %zu", lut_count, (size_t)1 << log_lut);
    if (k + 1 == 0 || lwe_dim + 1 == 0 || cmux_passes_2_63({batch, lwe_dim + 1, sizeof(T)}) ||
        cmux_passes_2_63({batch, k + 1, (size_t)(levels ? levels : 1), pl->n, sizeof(T)}) ||
        cmux_passes_2_63({batch, lut_count, k + 1, pl->n, sizeof(T)}) ||
        cmux_passes_2_63({lwe_dim, k + 1, (size_t)(levels ? levels : 1), k + 1, pl->n, sizeof(T)}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the key or the workspace pass 2^63 bytes", lwe_dim, k,
                    batch);
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, k, levels, batch);
    if (int rc = pbs_check<F>(pl, bsk, lwe_dim, k, base_log, levels, batch, workspace, workspace_bytes, Z.total())) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t n = pl->n, ob = batch * lut_count * (k * n + 1) * sizeof(T), ib = batch * (lwe_dim + 1) * sizeof(T);
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = lwe_dim * (k + 1) * levels * (k + 1) * n * sizeof(T);
    const Operand ops[5] = {{"lwe_out", lwe_out, ob, sizeof(T), true},
                            {"lwe_in", lwe_in, ib, sizeof(T), false},
                            {"lut", lut, lb, sizeof(T), false},
                            {"bsk_ntt", lwe_dim ? bsk : nullptr, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    Staging s(where, st);
    const T *dkey = lwe_dim ? (const T *)s.in(bsk, kb) : nullptr;
    const T *din = (const T *)s.in(lwe_in, ib), *dlut = (const T *)s.in(lut, lb);
    T *dout = (T *)s.out(lwe_out, ob);
    char *ws = (char *)s.workspace(workspace, Z.total());   // one block for the whole call
    if (int rc = s.status()) return rc;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    T *acc = static_cast<T *>(static_cast<void *>(ws + up256(Z.digits) + up256(Z.rot)));
    if (int rc = modswitch_manylut_device<T>(pl, rot_t, din, lwe_dim, log_lut, batch, st)) return rc;
    if (int rc = blind_rotate_device<F>(pl, acc, dlut, lut_per_element != 0, rot_t, dkey, lwe_dim, k, base_log, levels, batch,
                                        static_cast<T *>(static_cast<void *>(ws)), st))
        return rc;
    if (int rc = extract_many_device<T>(pl, dout, acc, k, lut_count, batch, st)) return rc;
    return s.finish();
}

// the six parts of the workspace of the one-rotation circuit bootstrap, in bytes and in this order (cntt_prime_manylut.h states the
// formula): the rotation's parts are per input bit, the keyswitch's per bit and level, with the slab rule of prime_cbs_shape unchanged
template <class T>
static CbsSizes cbs_manylut_sizes(const PrimePlan<T> *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                                  size_t batch) {
    const size_t e = batch * cbs_levels, r = (k * pl->n + 1) * ks_levels, ct = (k + 1) * pl->n * sizeof(T);
    CbsSizes Z;
    Z.shape = prime_cbs_shape(pl->n, sizeof(T), k, r, e);
    Z.rot = (lwe_dim + 1) * batch * sizeof(uint32_t);
    Z.table = ct;
    Z.pbs_digits = batch * ct * pbs_levels;
    Z.acc = batch * ct;
    Z.ks_digits = e * r * sizeof(int32_t);
    Z.part = Z.shape.slabs * (k + 1) * e * ct;
    return Z;
}

// set-up (the coarse switch of lwe + Q4, the shared table) -> one blind rotation over the batch -> extraction at the indices l - 1 and
// signed digits -> the digit x key product in slabs -> the sum of the slabs, negated, in the selector layout
template <class T>
static int circuit_bootstrap_manylut_device(const PrimePlan<T> *pl, T *out, const T *lwe_in, const T *bsk, const T *fpksk, size_t lwe_dim, size_t k,
                                            unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                            unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut, size_t batch, const CbsSizes &Z, char *ws,
                                            hipStream_t st) {
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
    const size_t tiles = ((lwe_dim + PRIME_PBS_TILE) / PRIME_PBS_TILE) * ((batch + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE);
    hipError_t err = launch_prime_cbs_manylut_setup<T>(rot_t, table, lwe_in, C, log_lut, lwe_dim, batch,
                                                       ew_grid((tiles + (Z.table / 16 + 255) / 256) * 256), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_modswitch_manylut_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = blind_rotate_device<PrimePbs<T>>(pl, acc, table, false, rot_t, bsk, lwe_dim, k, pbs_base_log, pbs_levels, batch, pbs_digits, st))
        return rc;
    err = launch_prime_cbs_manylut_extract<T>(ks_digits, acc, prime_pack_const(pl, ks_base_log, ks_levels), C, batch, ew_grid(batch * (k * n + 1)), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_manylut_extract_kernel launch failed: %s", hipGetErrorString(err));
    // |slab sum| <= rows 2^(ks_base_log - 1) (2^W - 1) < 2^bits
    unsigned rows_bits = 0;
    while ((Z.shape.rows >> rows_bits) != 0) ++rows_bits;
    const unsigned bits = C.wbits + ks_base_log - 1 + rows_bits;
    err = launch_prime_cbs_ks<T>(part, ks_digits, fpksk, pl->p, pl->logn, k, r, e, Z.shape, bits, st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_ks_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_prime_cbs_sum<T>(out, part, pl->p, pl->logn, k, cbs_levels, e, Z.shape.slabs, ew_grid((k + 1) * e * (k + 1) * n * sizeof(T) / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "prime_cbs_sum_kernel launch failed: %s", hipGetErrorString(err));
    return CNTT_OK;
}

template <class T>
static int circuit_bootstrap_manylut(const PrimePlan<T> *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim,
                                     size_t k, unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                     unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut, size_t batch, void *workspace,
                                     size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    const unsigned wbits = modulus_bits(pl);
    if (int rc = cbs_check_gadget("pbs_", pbs_base_log, pbs_levels, wbits)) return rc;
    if (int rc = cbs_check_gadget("ks_", ks_base_log, ks_levels, wbits)) return rc;
    if (ks_base_log > 31) return fail(CNTT_EINVAL, "ks_base_log = %u is above 31: a signed digit must fit an int32", ks_base_log);
    if (int rc = cbs_check_gadget("cbs_", cbs_base_log, cbs_levels, wbits)) return rc;
    if (int rc = manylut_check_log(pl, log_lut)) return rc;
    if (log_lut + 1 > (unsigned)pl->logn)
        return fail(CNTT_EINVAL, "2^log_lut_count = 2^%u exceeds ntt_size / 2 = %zu: the bit values n / 2 and 3 n / 2 leave the coarse grid", log_lut,
                    pl->n / 2);
    if (cbs_levels > (1u << log_lut))
        return fail(CNTT_EINVAL, "cbs_levels = %u exceeds 2^log_lut_count = %u", cbs_levels, 1u << log_lut);
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t n = pl->n;
    if (((u128)k * n + 1) * ks_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "(glwe_dim * n + 1) * ks_levels = (%zu * %zu + 1) * %u is not below 2^32 key rows", k, n, ks_levels);
    const size_t r = (k * n + 1) * ks_levels;
    // what the widest launch holds: the external product of the rotation over the batch
    if ((u128)batch * (k + 1) * pbs_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * pbs_levels = %zu * %zu * %u is not below 2^32: too large for one launch", batch, k + 1,
                    pbs_levels);
    // the byte counts are products of the arguments: they must fit before they are formed (2048 = the most slabs the shape rule gives)
    if (cmux_passes_2_63({batch, (size_t)cbs_levels}) || cmux_passes_2_63({batch, lwe_dim + 1, sizeof(T)}) || lwe_dim + 1 == 0 ||
        cmux_passes_2_63({lwe_dim, k + 1, (size_t)pbs_levels, k + 1, n, sizeof(T)}) || cmux_passes_2_63({k + 1, r, k + 1, n, sizeof(T)}) ||
        cmux_passes_2_63({batch, k + 1, (size_t)pbs_levels, n, sizeof(T)}) || cmux_passes_2_63({batch, (size_t)cbs_levels, r, (size_t)4}) ||
        cmux_passes_2_63({(size_t)2048, k + 1, batch, (size_t)cbs_levels, k + 1, n, sizeof(T)}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the keys, the selectors or the workspace pass 2^63 bytes",
                    lwe_dim, k, batch);
    if (batch == 0) return CNTT_OK;
    if (!ggsw_ntt_out) return fail(CNTT_EINVAL, "ggsw_ntt_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim && !bsk_ntt) return fail(CNTT_EINVAL, "bsk_ntt is NULL");
    if (!fpksk_ntt) return fail(CNTT_EINVAL, "fpksk_ntt is NULL");
    const size_t e = batch * cbs_levels;
    const CbsSizes Z = cbs_manylut_sizes(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch);
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
    if (int rc = circuit_bootstrap_manylut_device<T>(pl, dout, din, dbsk, dfk, lwe_dim, k, pbs_base_log, pbs_levels, ks_base_log, ks_levels,
                                                     cbs_base_log, cbs_levels, log_lut, batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_MANYLUT_API(BITS, T, PLAN)                                                                                                \
    extern "C" int cntt_prime##BITS##_lwe_modswitch_manylut_batch(const PLAN *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim,             \
                                                                  unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream) {   \
        return lwe_modswitch_manylut<T>(pl, rot_t, lwe, lwe_dim, log_lut_count, batch, where, (hipStream_t)stream);                          \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_sample_extract_many_batch(const PLAN *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t count,    \
                                                                size_t batch, cntt_mem_t where, void *stream) {                              \
        return sample_extract_many<T>(pl, lwe_out, glwe, glwe_dim, count, batch, where, (hipStream_t)stream);                                \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_bootstrap_manylut_batch(                                                                               \
        const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element, const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim,   \
        unsigned base_log, unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch, void *workspace, size_t workspace_bytes, \
        cntt_mem_t where, void *stream) {                                                                                                    \
        return bootstrap_manylut<T>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, log_lut_count,  \
                                    lut_count, batch, workspace, workspace_bytes, where, (hipStream_t)stream);                               \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_circuit_bootstrap_manylut_batch(                                                                       \
        const PLAN *pl, T *ggsw_ntt_out, const T *lwe_in, const T *bsk_ntt, const T *fpksk_ntt, size_t lwe_dim, size_t glwe_dim,             \
        unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels,    \
        unsigned log_lut_count, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {                     \
        return circuit_bootstrap_manylut<T>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels,       \
                                            ks_base_log, ks_levels, cbs_base_log, cbs_levels, log_lut_count, batch, workspace,              \
                                            workspace_bytes, where, (hipStream_t)stream);                                                    \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_circuit_bootstrap_manylut_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim,          \
                                                                                   unsigned pbs_levels, unsigned ks_levels,                 \
                                                                                   unsigned cbs_levels, size_t batch) {                      \
        return pl ? cbs_manylut_sizes<T>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch).total() : 0;                       \
    }

CNTT_PRIME_MANYLUT_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_MANYLUT_API(32, uint32_t, cntt_plan32)
