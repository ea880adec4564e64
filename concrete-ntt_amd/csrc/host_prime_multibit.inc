// Part of host_prime.hip (included at its end, after host_prime_pack.inc): the multi-bit blind rotation and bootstrap of the prime plans
// (include/cntt_prime_multibit.h) -- the table of monomial powers, the launch of prime_multibit_accumulate_kernel (prime_multibit.hpp;
// launched by prime_multibit.hip), the loop over the groups and the C ABI.  The digits are gadget_device (host_prime_pbs.inc) in the PLAIN
// mode, the transforms ntt_device above, and the two ends of the bootstrap those of pbs_host.hpp; none of them is changed.
#include "../../include/cntt_prime_multibit.h"
#include "prime_multibit.hpp"

#pragma GCC visibility push(hidden)

// tab[m] = psi^m 2^(2B) mod p for m < n, psi = the plan's root: per device, next to the twiddle tables and under their mutex, built by the
// first multi-bit call on the device (a synchronous allocation and copy, like theirs: that call may not sit inside a stream capture --
// include/cntt_prime_multibit.h, "First call").  Later calls: one lock, one look-up.
template <class T> static int multibit_table(const PrimePlan<T> *pl, const T **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lk(pl->cache->mu);
        auto it = pl->cache->per_device.find(dev);
        if (it != pl->cache->per_device.end() && it->second.mono) {
            *out = it->second.mono;
            return CNTT_OK;
        }
    }
    DeviceTables<T> t;
    if (int rc = device_tables(pl, &t)) return rc;   // the replica's entry exists from here
    std::lock_guard<std::mutex> lk(pl->cache->mu);
    DeviceTables<T> &e = pl->cache->per_device[dev];
    if (!e.mono) {
        const uint64_t p64 = (uint64_t)pl->p;
        std::vector<T> tab(pl->n);
        uint64_t x = (uint64_t)pl->mp.r2;
        for (size_t m = 0; m < pl->n; ++m) {
            tab[m] = (T)x;
            x = host::mulmod(x, pl->root, p64);
        }
        T *d = nullptr;
        if (hipMalloc((void **)&d, pl->n * sizeof(T)) != hipSuccess) return fail(CNTT_ENOMEM, "hipMalloc of the monomial table failed");
        const hipError_t c = hipMemcpy(d, tab.data(), pl->n * sizeof(T), hipMemcpyHostToDevice);
        if (c != hipSuccess) {
            (void)hipFree(d);
            return fail(CNTT_EDEVICE, "upload of the monomial table failed: %s", hipGetErrorString(c));
        }
        e.mono = d;
    }
    *out = e.mono;
    return CNTT_OK;
}

template <class T>
static int multibit_accumulate_device(const PrimePlan<T> *pl, T *out, const T *terms, const uint32_t *rot_rows, const T *key, size_t nterms,
                                      size_t nout, unsigned grouping, size_t batch, hipStream_t st) {
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (nterms == 0) {   // empty sums
        HIP_TRY(hipMemsetAsync(out, 0, batch * nout * pl->n * sizeof(T), st));
        return CNTT_OK;
    }
    const T *tab = nullptr;
    if (int rc = multibit_table(pl, &tab)) return rc;
    const hipError_t e = launch_prime_multibit_accumulate<T>(out, terms, rot_rows, key, tab, pl->p, pl->mp.pinv_neg, pl->logn, nterms, nout,
                                                             grouping, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_multibit_accumulate_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

// acc = X^(body row of rot_t) lut, then per group: digits of acc (PLAIN) -> fwd in place -> the bundle's pointwise step into acc -> inv.
// Writing acc in the third step is sound in stream order: its old words are dead once the digits exist.
template <class T>
static int multibit_rotate_device(const PrimePlan<T> *pl, T *acc, const T *lut, bool lut_per_element, const uint32_t *rot_t, const T *bsk,
                                  size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                  T *digits, hipStream_t st) {
    using F = PrimePbs<T>;
    const size_t npolys = glwe_dim + 1, nterms = npolys * levels, n = pl->n;
    const size_t group_polys = ((size_t)nterms * npolys) << grouping;   // one group's key
    const hipError_t e = F::launch_pbs_init(pl, acc, lut, rot_t + lwe_dim * batch, (uint32_t)npolys, lut_per_element, batch,
                                            batch * npolys * n * sizeof(T) > STREAM_BYTES, ew_grid(batch * npolys * n * sizeof(T) / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_pbs_init_kernel launch failed: %s", hipGetErrorString(e));
    for (size_t r = 0; r < lwe_dim / grouping; ++r) {
        if (int rc = gadget_device<T>(pl, digits, acc, nullptr, npolys, base_log, levels, CNTT_SRC_PLAIN, batch, st)) return rc;
        if (int rc = ntt_device<T>(pl, digits, batch * nterms, false, st)) return rc;
        if (int rc = multibit_accumulate_device<T>(pl, acc, digits, rot_t + r * grouping * batch, bsk + r * group_polys * n, nterms, npolys,
                                                   grouping, batch, st))
            return rc;
        if (int rc = ntt_device<T>(pl, acc, batch * npolys, true, st)) return rc;
    }
    return CNTT_OK;
}

template <class T>
static int multibit_accumulate(const PrimePlan<T> *pl, T *out, const T *terms, const uint32_t *rot_rows, const T *key, size_t nterms,
                               size_t nout, unsigned grouping, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (grouping == 0 || grouping > PRIME_MULTIBIT_MAX_GROUPING) return fail(CNTT_EINVAL, "grouping = %u is not in 1 ... 4", grouping);
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (!out) return fail(CNTT_EINVAL, "out_ntt is NULL");
    if (!rot_rows) return fail(CNTT_EINVAL, "rot_rows is NULL");
    if (nterms && !terms) return fail(CNTT_EINVAL, "terms_ntt is NULL");
    if (nterms && !key) return fail(CNTT_EINVAL, "key_group is NULL");
    if (nterms >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "nterms or nout too large");
    const size_t pb = pl->n * sizeof(T), ob = batch * nout * pb, tb = batch * nterms * pb, kb = ((nterms * nout) << grouping) * pb,
                 rb = grouping * batch * sizeof(uint32_t);
    const Operand ops[4] = {{"out_ntt", out, ob, sizeof(T), true},
                            {"terms_ntt", terms, tb, sizeof(T), false},
                            {"rot_rows", rot_rows, rb, sizeof(uint32_t), false},
                            {"key_group", key, kb, sizeof(T), false}};
    if (int rc = check_operands(ops, 4)) return rc;
    if (where == CNTT_MEM_DEVICE) return multibit_accumulate_device<T>(pl, out, terms, rot_rows, key, nterms, nout, grouping, batch, st);
    if (int rc = check_rot_host(pl->n, rot_rows, grouping * batch, "rot_rows")) return rc;
    Staging s(st);
    T *dout = (T *)s.out(out, ob);
    const T *dt = (const T *)s.in(terms, tb), *dk = (const T *)s.in(key, kb);
    const uint32_t *dr = (const uint32_t *)s.in(rot_rows, rb);
    if (int rc = s.status()) return rc;
    if (int rc = multibit_accumulate_device<T>(pl, dout, dt, dr, dk, nterms, nout, grouping, batch, st)) return rc;
    return s.finish();
}

// the argument checks the blind rotation and the bootstrap share
template <class T>
static int multibit_check(const PrimePlan<T> *pl, const T *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                          unsigned grouping, size_t batch, const void *workspace, size_t workspace_bytes, size_t need) {
    if (int rc = gadget_check<PrimePbs<T>>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (grouping == 0 || grouping > PRIME_MULTIBIT_MAX_GROUPING) return fail(CNTT_EINVAL, "grouping = %u is not in 1 ... 4", grouping);
    if (lwe_dim % grouping) return fail(CNTT_EINVAL, "lwe_dim = %zu is not a multiple of grouping = %u", lwe_dim, grouping);
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (batch == 0) return CNTT_OK;
    // what ntt_device would refuse halfway through the call
    const int depth = pl->logn > MaxLdsLogN<T>::value ? pl->logn - MaxLdsLogN<T>::value : 0;
    if ((u128)batch * (glwe_dim + 1) * levels >= ((u128)1 << (32 - depth)))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * levels is too large for one transform launch");
    if (lwe_dim && !bsk) return fail(CNTT_EINVAL, "bsk_mb is NULL");
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    return CNTT_OK;
}
template <class T> static size_t multibit_key_bytes(const PrimePlan<T> *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, unsigned grouping) {
    return (((lwe_dim / grouping) * (glwe_dim + 1) * levels * (glwe_dim + 1)) << grouping) * pl->n * sizeof(T);
}

template <class T>
static int multibit_blind_rotate(const PrimePlan<T> *pl, T *acc, const T *lut, int lut_per_element, const uint32_t *rot_t, const T *bsk,
                                 size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                 void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using F = PrimePbs<T>;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch && !rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = multibit_check<T>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.digits)) return rc;
    if (batch == 0) return CNTT_OK;
    if (!acc) return fail(CNTT_EINVAL, "acc is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = multibit_key_bytes(pl, lwe_dim, glwe_dim, levels, grouping);
    const Operand ops[5] = {{"acc", acc, Z.acc, sizeof(T), true},
                            {"lut", lut, lb, sizeof(T), false},
                            {"rot_t", rot_t, Z.rot, sizeof(uint32_t), false},
                            {"bsk_mb", bsk, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    if (where == CNTT_MEM_DEVICE) {
        void *digits = workspace;
        if (!digits && lwe_dim) HIP_TRY(hipMallocAsync(&digits, Z.digits, st));   // one allocation for the whole loop
        const int rc = multibit_rotate_device<T>(pl, acc, lut, lut_per_element != 0, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, grouping,
                                                 batch, (T *)digits, st);
        if (!workspace && digits) (void)hipFreeAsync(digits, st);
        return rc;
    }
    if (int rc = check_rot_host(pl->n, rot_t, (lwe_dim + 1) * batch, "rot_t")) return rc;
    Staging s(st);
    const T *dkey = lwe_dim ? (const T *)s.in(bsk, kb) : nullptr;
    const T *dlut = (const T *)s.in(lut, lb);
    const uint32_t *drot = (const uint32_t *)s.in(rot_t, Z.rot);
    T *dacc = (T *)s.out(acc, Z.acc), *ddig = (T *)s.alloc(Z.digits);
    if (int rc = s.status()) return rc;
    if (int rc = multibit_rotate_device<T>(pl, dacc, dlut, lut_per_element != 0, drot, dkey, lwe_dim, glwe_dim, base_log, levels, grouping,
                                           batch, ddig, st))
        return rc;
    return s.finish();
}

// modulus switch -> multi-bit blind rotation -> extraction of coefficient 0 on device buffers; ws holds digits | rot_t | acc (PbsSizes)
template <class T>
static int multibit_bootstrap_device(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *lut, bool lut_per_element, const T *bsk,
                                     size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                     const PbsSizes &Z, char *ws, hipStream_t st) {
    using F = PrimePbs<T>;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    T *acc = static_cast<T *>(static_cast<void *>(ws + up256(Z.digits) + up256(Z.rot)));
    if (int rc = modswitch_device<F>(pl, rot_t, lwe_in, lwe_dim, batch, st)) return rc;
    if (int rc = multibit_rotate_device<T>(pl, acc, lut, lut_per_element, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                           static_cast<T *>(static_cast<void *>(ws)), st))
        return rc;
    return extract_device<F>(pl, lwe_out, acc, glwe_dim, 0, batch, st);
}

template <class T>
static int multibit_bootstrap(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element, const T *bsk,
                              size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                              void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using F = PrimePbs<T>;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = multibit_check<T>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.total())) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t ob = batch * (glwe_dim * pl->n + 1) * sizeof(T), ib = batch * (lwe_dim + 1) * sizeof(T);
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = multibit_key_bytes(pl, lwe_dim, glwe_dim, levels, grouping);
    const Operand ops[5] = {{"lwe_out", lwe_out, ob, sizeof(T), true},
                            {"lwe_in", lwe_in, ib, sizeof(T), false},
                            {"lut", lut, lb, sizeof(T), false},
                            {"bsk_mb", bsk, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    if (where == CNTT_MEM_DEVICE) {
        void *ws = workspace;
        if (!ws) HIP_TRY(hipMallocAsync(&ws, Z.total(), st));   // one allocation for the whole call
        const int rc = multibit_bootstrap_device<T>(pl, lwe_out, lwe_in, lut, lut_per_element != 0, bsk, lwe_dim, glwe_dim, base_log, levels,
                                                    grouping, batch, Z, static_cast<char *>(ws), st);
        if (!workspace) (void)hipFreeAsync(ws, st);
        return rc;
    }
    Staging s(st);
    const T *dkey = lwe_dim ? (const T *)s.in(bsk, kb) : nullptr;
    const T *din = (const T *)s.in(lwe_in, ib), *dlut = (const T *)s.in(lut, lb);
    T *dout = (T *)s.out(lwe_out, ob);
    char *dws = (char *)s.alloc(Z.total());
    if (int rc = s.status()) return rc;
    if (int rc = multibit_bootstrap_device<T>(pl, dout, din, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels, grouping,
                                              batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" unsigned cntt_prime_multibit_grid(size_t vectors) { return prime_multibit_grid(vectors); }

#define CNTT_PRIME_MULTIBIT_API(BITS, T, PLAN)                                                                                               \
    extern "C" int cntt_prime##BITS##_multibit_accumulate_batch(const PLAN *pl, T *out_ntt, const T *terms_ntt, const uint32_t *rot_rows,     \
                                                                const T *key_group, size_t nterms, size_t nout, unsigned grouping,           \
                                                                size_t batch, cntt_mem_t where, void *stream) {                              \
        return multibit_accumulate<T>(pl, out_ntt, terms_ntt, rot_rows, key_group, nterms, nout, grouping, batch, where,                      \
                                      (hipStream_t)stream);                                                                                   \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_multibit_blind_rotate_batch(const PLAN *pl, T *acc, const T *lut, int lut_per_element,                  \
                                                                  const uint32_t *rot_t, const T *bsk_mb, size_t lwe_dim, size_t glwe_dim,   \
                                                                  unsigned base_log, unsigned levels, unsigned grouping, size_t batch,       \
                                                                  void *workspace, size_t workspace_bytes, cntt_mem_t where,                 \
                                                                  void *stream) {                                                            \
        return multibit_blind_rotate<T>(pl, acc, lut, lut_per_element, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, batch,   \
                                        workspace, workspace_bytes, where, (hipStream_t)stream);                                              \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_multibit_bootstrap_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut,                     \
                                                               int lut_per_element, const T *bsk_mb, size_t lwe_dim, size_t glwe_dim,        \
                                                               unsigned base_log, unsigned levels, unsigned grouping, size_t batch,          \
                                                               void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {    \
        return multibit_bootstrap<T>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping,        \
                                     batch, workspace, workspace_bytes, where, (hipStream_t)stream);                                          \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_multibit_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,       \
                                                                      unsigned, size_t batch) {                                              \
        return pbs_workspace_bytes<PrimePbs<T>>(pl, lwe_dim, glwe_dim, levels, batch);                                                        \
    }

CNTT_PRIME_MULTIBIT_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_MULTIBIT_API(32, uint32_t, cntt_plan32)
