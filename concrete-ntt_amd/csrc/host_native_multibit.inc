// Part of host_native_ext.hip (included at its end): the multi-bit blind rotation and bootstrap of the native plans
// (include/cntt_multibit.h) -- the launch of native_multibit_accumulate_kernel (native_multibit.hpp; launched by native_multibit.hip), the
// stand-alone accumulate call, the multibit_* members of NativePbs that multibit_host.hpp asks for, and the C ABI.  The checks, the
// workspace and the loop over the groups are multibit_host.hpp's, shared with the prime plans.  Per group: native_gadget_device (PLAIN)
// -> native_split_device -> the sub-plans' forward transforms -> the new kernel -> the sub-plans' inverse transforms -> native_crt_device;
// the two ends of the bootstrap are those of pbs_host.hpp.  None of them is changed.  The monomial tables live in the native cache
// (host_native.hip, native_multibit_tables).
#include "../../include/cntt_multibit.h"
#include "native_multibit.hpp"

#pragma GCC visibility push(hidden)
static_assert(NATIVE_MULTIBIT_MAX_GROUPING == MULTIBIT_MAX_GROUPING, "the grouping check of multibit_host.hpp is not the kernel's bound");

// the lazy inner sum of the kernel is derived from P < 2^30 (native_multibit.hpp): every prime a Plan32 kind can hold
static constexpr bool multibit_primes_in_range() {
    for (int i = 0; i < 10; ++i)
        if (PRIMES32[i] >= NATIVE_MULTIBIT_PRIME_BOUND) return false;
    return true;
}
static_assert(multibit_primes_in_range(), "a prime of PRIMES32 is not below 2^30: the four-product lazy sum would leave the range of one reduction");

int NativePbs::multibit_plan_check(const cntt_native *pl) {
    if (multibit_supported(pl)) return CNTT_OK;
    return fail(CNTT_EINVAL, "plan kind %d is a Plan52 kind: the multi-bit calls exist for the Plan32 kinds only (50-bit key residues)",
                (int)pl->kind);
}

static int native_multibit_accumulate_device(const cntt_native *pl, void *const *out, const void *const *terms, const uint32_t *rot_rows,
                                             const void *const *key, size_t nterms, size_t nout, unsigned grouping, size_t batch,
                                             hipStream_t st) {
    if (batch == 0 || nout == 0) return CNTT_OK;
    const int k = pl->info.nprimes;
    if (nterms == 0) {   // empty sums
        for (int i = 0; i < k; ++i) HIP_TRY(hipMemsetAsync(out[i], 0, batch * nout * pl->n * sizeof(uint32_t), st));
        return CNTT_OK;
    }
    const uint32_t *tab[10];
    if (int rc = native_multibit_tables(pl, tab)) return rc;
    MultibitPlanes A{};
    for (int i = 0; i < k; ++i) {
        const cntt_plan32 *sub = pl->p32[(size_t)i].get();
        A.out[i] = static_cast<uint32_t *>(out[i]);
        A.terms[i] = static_cast<const uint32_t *>(terms[i]);
        A.key[i] = static_cast<const uint32_t *>(key[i]);
        A.tab[i] = tab[i];
        A.p[i] = sub->p;
        A.pinv_neg[i] = sub->mp.pinv_neg;
    }
    const hipError_t e = launch_native_multibit_accumulate(A, (unsigned)k, rot_rows, native_logn(pl), nterms, nout, grouping, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_multibit_accumulate_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

// false when a part of the workspace, or the rot_t of lwe_dim rows, does not fit 2^62 bytes: multibit_sizes would wrap.  Every factor
// is below 2^64 and the running product is held below 2^62, so the u128 products cannot wrap themselves.
bool NativePbs::multibit_sizes_fit(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const u128 cap = (u128)1 << 62;
    u128 x = (u128)batch;
    for (const u128 f : {(u128)glwe_dim + 1, (u128)pl->n, (u128)levels, (u128)pl->info.nprimes * 16}) {
        x *= f;
        if (x >= cap) return false;
    }
    return batch == 0 || (u128)lwe_dim + 1 < cap / sizeof(uint32_t) / batch;
}
int NativePbs::multibit_check_terms(const cntt_native *pl, size_t glwe_dim, unsigned levels, unsigned grouping) {
    const u128 products = ((u128)(glwe_dim + 1) * levels) << grouping;
    if (products > (u128)pl->max_terms)
        return fail(CNTT_EINVAL,
                    "2^grouping * (glwe_dim + 1) * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range",
                    (size_t)products, pl->max_terms);
    return CNTT_OK;
}
// the scratch of the workspace: the residue planes of the terms, then those of the outputs (cntt_multibit.h states the formula)
void NativePbs::multibit_scratch(const cntt_native *pl, size_t polys, unsigned levels, size_t *bytes) {
    const size_t planes = (size_t)pl->info.nprimes * polys * pl->n * sizeof(uint32_t);
    bytes[0] = planes * levels;
    bytes[1] = planes;
}

// one group of the loop of multibit_host.hpp: the digits into residue planes -> fwd in place -> the bundle's pointwise step into the
// output planes -> inv in place -> CRT into acc
int NativePbs::multibit_step(const cntt_native *pl, void *acc, void *digits, char *scratch, const MultibitSizes &Z, const uint32_t *rot_rows,
                             Key key, size_t nterms, size_t npolys, unsigned grouping, size_t batch, hipStream_t st) {
    const size_t k = (size_t)pl->info.nprimes, n = pl->n;
    void *T[10], *O[10];
    for (size_t i = 0; i < k; ++i) {
        T[i] = scratch + i * (Z.scratch[0] / k);
        O[i] = scratch + up256(Z.scratch[0]) + i * (Z.scratch[1] / k);
    }
    if (int rc = native_split_device(pl, digits, T, batch * nterms * n, false, st)) return rc;
    if (int rc = native_ntt_device(pl, T, batch * nterms, false, st)) return rc;
    if (int rc = native_multibit_accumulate_device(pl, O, T, rot_rows, key, nterms, npolys, grouping, batch, st)) return rc;
    if (int rc = native_ntt_device(pl, O, batch * npolys, true, st)) return rc;
    return native_crt_device(pl, acc, O, batch * npolys * n, st);
}

#define MB_PLANES(s) {s "[0]", s "[1]", s "[2]", s "[3]", s "[4]", s "[5]", s "[6]", s "[7]", s "[8]", s "[9]"}
static const char *const MB_OUT[10] = MB_PLANES("out_ntt");
static const char *const MB_TERMS[10] = MB_PLANES("terms_ntt");
static const char *const MB_KEY[10] = MB_PLANES("key_group");
static const char *const MB_BSK[10] = MB_PLANES("bsk_mb");
#undef MB_PLANES
// how the key appears among the operands of the two calls: one plane per prime
int NativePbs::multibit_key_operands(const cntt_native *pl, Operand *ops, int cnt, Key bsk, size_t kb) {
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {MB_BSK[i], bsk[i], kb, sizeof(uint32_t), false};
    return cnt;
}

static int native_multibit_accumulate(const cntt_native *pl, void *const *out, const void *const *terms, const uint32_t *rot_rows,
                                      const void *const *key, size_t nterms, size_t nout, unsigned grouping, size_t batch, cntt_mem_t where,
                                      hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = NativePbs::multibit_plan_check(pl)) return rc;
    if (int rc = multibit_grouping_check(grouping)) return rc;
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (!out) return fail(CNTT_EINVAL, "out_ntt is NULL");
    if (!rot_rows) return fail(CNTT_EINVAL, "rot_rows is NULL");
    if (nterms && !terms) return fail(CNTT_EINVAL, "terms_ntt is NULL");
    if (nterms && !key) return fail(CNTT_EINVAL, "key_group is NULL");
    if (nterms >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "nterms or nout too large");
    const int k = pl->info.nprimes;
    for (int i = 0; i < k; ++i) {
        if (!out[i]) return fail(CNTT_EINVAL, "NULL residue plane (out_ntt[%d])", i);
        if (nterms && !terms[i]) return fail(CNTT_EINVAL, "NULL residue plane (terms_ntt[%d])", i);
        if (nterms && !key[i]) return fail(CNTT_EINVAL, "NULL residue plane (key_group[%d])", i);
    }
    const size_t pb = pl->n * sizeof(uint32_t), ob = batch * nout * pb, tb = batch * nterms * pb, kb = ((nterms * nout) << grouping) * pb,
                 rb = grouping * batch * sizeof(uint32_t);
    Operand ops[31];
    int cnt = 0;
    for (int i = 0; i < k; ++i) ops[cnt++] = {MB_OUT[i], out[i], ob, sizeof(uint32_t), true};
    for (int i = 0; i < k && nterms; ++i) ops[cnt++] = {MB_TERMS[i], terms[i], tb, sizeof(uint32_t), false};
    for (int i = 0; i < k && nterms; ++i) ops[cnt++] = {MB_KEY[i], key[i], kb, sizeof(uint32_t), false};
    ops[cnt++] = {"rot_rows", rot_rows, rb, sizeof(uint32_t), false};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    if (s.host())
        if (int rc = check_rot_host(pl->n, rot_rows, grouping * batch, "rot_rows")) return rc;
    void *dout[10];
    const void *dt[10], *dk[10];
    for (int i = 0; i < k; ++i) {
        dout[i] = s.out(out[i], ob);
        dt[i] = s.in(nterms ? terms[i] : nullptr, tb);
        dk[i] = s.in(nterms ? key[i] : nullptr, kb);
    }
    const uint32_t *dr = (const uint32_t *)s.in(rot_rows, rb);
    if (int rc = s.status()) return rc;
    if (int rc = native_multibit_accumulate_device(pl, dout, dt, dr, dk, nterms, nout, grouping, batch, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" unsigned cntt_native_multibit_grid(size_t vectors) { return native_multibit_grid(vectors); }

extern "C" int cntt_native_multibit_accumulate_batch(const cntt_native_t *pl, void *const *out_ntt, const void *const *terms_ntt,
                                                     const uint32_t *rot_rows, const void *const *key_group, size_t nterms, size_t nout,
                                                     unsigned grouping, size_t batch, cntt_mem_t where, void *stream) {
    return native_multibit_accumulate(pl, out_ntt, terms_ntt, rot_rows, key_group, nterms, nout, grouping, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_multibit_blind_rotate_batch(const cntt_native_t *pl, void *acc, const void *lut, int lut_per_element,
                                                       const uint32_t *rot_t, const void *const *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                                       unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                                       size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return multibit_blind_rotate<NativePbs>(pl, acc, lut, lut_per_element, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                            workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" int cntt_native_multibit_bootstrap_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *lut,
                                                    int lut_per_element, const void *const *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                                    unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                                    size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return multibit_bootstrap<NativePbs>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                         workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_multibit_pbs_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,
                                                           unsigned, size_t batch) {
    return multibit_pbs_workspace_bytes<NativePbs>(pl, lwe_dim, glwe_dim, levels, batch);
}
