// Part of host_prime.hip (included at its end, after host_prime_pack.inc): the multi-bit blind rotation and bootstrap of the prime plans
// (include/cntt_prime_multibit.h) -- the table of monomial powers, the launch of prime_multibit_accumulate_kernel (prime_multibit.hpp;
// launched by prime_multibit.hip), the stand-alone accumulate call, the step of PrimePbs<T> that multibit_host.hpp runs per group, and
// the C ABI.  The checks, the workspace and the loop over the groups are multibit_host.hpp's, shared with the native plans.  The digits
// are gadget_device (host_prime_pbs.inc) in the PLAIN mode, the transforms ntt_device above, and the two ends of the bootstrap those of
// pbs_host.hpp; none of them is changed.
#include "../../include/cntt_prime_multibit.h"
#include "prime_multibit.hpp"

#pragma GCC visibility push(hidden)
static_assert(PRIME_MULTIBIT_MAX_GROUPING == MULTIBIT_MAX_GROUPING, "the grouping check of multibit_host.hpp is not the kernel's bound");

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

// one group of the loop of multibit_host.hpp: fwd of the digits in place -> the bundle's pointwise step into acc -> inv
template <class T>
int PrimePbs<T>::multibit_step(const Plan *pl, T *acc, T *digits, char *, const MultibitSizes &, const uint32_t *rot_rows, Key key,
                               size_t nterms, size_t npolys, unsigned grouping, size_t batch, hipStream_t st) {
    if (int rc = ntt_device<T>(pl, digits, batch * nterms, false, st)) return rc;
    if (int rc = multibit_accumulate_device<T>(pl, acc, digits, rot_rows, key, nterms, npolys, grouping, batch, st)) return rc;
    return ntt_device<T>(pl, acc, batch * npolys, true, st);
}

template <class T>
static int multibit_accumulate(const PrimePlan<T> *pl, T *out, const T *terms, const uint32_t *rot_rows, const T *key, size_t nterms,
                               size_t nout, unsigned grouping, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = multibit_grouping_check(grouping)) return rc;
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
    Staging s(where, st);
    if (s.host())
        if (int rc = check_rot_host(pl->n, rot_rows, grouping * batch, "rot_rows")) return rc;
    T *dout = (T *)s.out(out, ob);
    const T *dt = (const T *)s.in(terms, tb), *dk = (const T *)s.in(key, kb);
    const uint32_t *dr = (const uint32_t *)s.in(rot_rows, rb);
    if (int rc = s.status()) return rc;
    if (int rc = multibit_accumulate_device<T>(pl, dout, dt, dr, dk, nterms, nout, grouping, batch, st)) return rc;
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
        return multibit_blind_rotate<PrimePbs<T>>(pl, acc, lut, lut_per_element, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels,          \
                                                  grouping, batch, workspace, workspace_bytes, where, (hipStream_t)stream);                   \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_multibit_bootstrap_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut,                     \
                                                               int lut_per_element, const T *bsk_mb, size_t lwe_dim, size_t glwe_dim,        \
                                                               unsigned base_log, unsigned levels, unsigned grouping, size_t batch,          \
                                                               void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {    \
        return multibit_bootstrap<PrimePbs<T>>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_mb, lwe_dim, glwe_dim, base_log, levels,        \
                                               grouping, batch, workspace, workspace_bytes, where, (hipStream_t)stream);                      \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_multibit_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,       \
                                                                      unsigned, size_t batch) {                                              \
        return multibit_pbs_workspace_bytes<PrimePbs<T>>(pl, lwe_dim, glwe_dim, levels, batch);                                               \
    }

CNTT_PRIME_MULTIBIT_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_MULTIBIT_API(32, uint32_t, cntt_plan32)
