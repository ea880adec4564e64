// Part of host_native_ext.hip (included at its end): the multi-bit blind rotation and bootstrap of the native plans
// (include/cntt_multibit.h) -- the launch of native_multibit_accumulate_kernel (native_multibit.hpp; launched by native_multibit.hip), the
// loop over the groups and the C ABI.  Per group: native_gadget_device (PLAIN) -> native_split_device -> the sub-plans' forward transforms
// -> the new kernel -> the sub-plans' inverse transforms -> native_crt_device; the two ends of the bootstrap are those of pbs_host.hpp
// through NativePbs.  None of them is changed.  The monomial tables live in the native cache (host_native.hip, native_multibit_tables).
#include "../../include/cntt_multibit.h"
#include "native_multibit.hpp"

#pragma GCC visibility push(hidden)

// the lazy inner sum of the kernel is derived from P < 2^30 (native_multibit.hpp): every prime a Plan32 kind can hold
static constexpr bool multibit_primes_in_range() {
    for (int i = 0; i < 10; ++i)
        if (PRIMES32[i] >= NATIVE_MULTIBIT_PRIME_BOUND) return false;
    return true;
}
static_assert(multibit_primes_in_range(), "a prime of PRIMES32 is not below 2^30: the four-product lazy sum would leave the range of one reduction");

static int multibit_plan_check(const cntt_native *pl) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (pl->info.is52)
        return fail(CNTT_EINVAL, "plan kind %d is a Plan52 kind: the multi-bit calls exist for the Plan32 kinds only (50-bit key residues)",
                    (int)pl->kind);
    return CNTT_OK;
}
static int multibit_grouping_check(unsigned grouping) {
    if (grouping == 0 || grouping > NATIVE_MULTIBIT_MAX_GROUPING) return fail(CNTT_EINVAL, "grouping = %u is not in 1 ... 4", grouping);
    return CNTT_OK;
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

// the parts of the workspace, in bytes and in this order (cntt_multibit.h states the formula); the blind rotation takes the first three
struct MultibitSizes {
    size_t digits, terms, outs, rot, acc;
    size_t rotate() const { return up256(digits) + up256(terms) + up256(outs); }
    size_t total() const { return rotate() + up256(rot) + up256(acc); }
};
// false when a part of the workspace, or the rot_t of lwe_dim rows, does not fit 2^62 bytes: multibit_sizes would wrap.  Every factor
// is below 2^64 and the running product is held below 2^62, so the u128 products cannot wrap themselves.
static bool multibit_sizes_fit(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const u128 cap = (u128)1 << 62;
    u128 x = (u128)batch;
    for (const u128 f : {(u128)glwe_dim + 1, (u128)pl->n, (u128)levels, (u128)pl->info.nprimes * 16}) {
        x *= f;
        if (x >= cap) return false;
    }
    return batch == 0 || (u128)lwe_dim + 1 < cap / sizeof(uint32_t) / batch;
}
static int multibit_sizes_check(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    if (!multibit_sizes_fit(pl, lwe_dim, glwe_dim, levels, batch))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * levels * ntt_size or (lwe_dim + 1) * batch is too large: the workspace would not fit 2^62 bytes");
    return CNTT_OK;
}
static MultibitSizes multibit_sizes(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const size_t polys = batch * (glwe_dim + 1), pb = polys * pl->n * (size_t)pl->info.word, rp = polys * pl->n * sizeof(uint32_t);
    const size_t k = (size_t)pl->info.nprimes;
    return MultibitSizes{pb * levels, k * rp * levels, k * rp, (lwe_dim + 1) * batch * sizeof(uint32_t), pb};
}

// acc = X^(body row of rot_t) lut, then per group: digits of acc (PLAIN) -> residue planes -> fwd in place -> the bundle's pointwise step
// into the output planes -> inv in place -> CRT into acc.  Writing acc in the last step is sound in stream order: its old words are dead
// once the digits exist.  ws: digits | term planes | output planes.
static int native_multibit_rotate_device(const cntt_native *pl, void *acc, const void *lut, bool lut_per_element, const uint32_t *rot_t,
                                         const void *const *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                         unsigned grouping, size_t batch, const MultibitSizes &Z, char *ws, hipStream_t st) {
    using F = NativePbs;
    const size_t npolys = glwe_dim + 1, nterms = npolys * levels, n = pl->n, w = F::word(pl);
    const int k = pl->info.nprimes;
    const size_t group_bytes = F::key_bytes(pl, (nterms * npolys) << grouping);   // one group's key, per plane
    const hipError_t e = F::launch_pbs_init(pl, acc, lut, rot_t + lwe_dim * batch, (uint32_t)npolys, lut_per_element, batch,
                                            batch * npolys * n * w > STREAM_BYTES, ew_grid(batch * npolys * n * w / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_pbs_init_kernel launch failed: %s", hipGetErrorString(e));
    if (lwe_dim == 0) return CNTT_OK;
    void *digits = ws, *T[10], *O[10];
    for (int i = 0; i < k; ++i) {
        T[i] = ws + up256(Z.digits) + (size_t)i * (Z.terms / (size_t)k);
        O[i] = ws + up256(Z.digits) + up256(Z.terms) + (size_t)i * (Z.outs / (size_t)k);
    }
    F::KeyStore ks;
    for (size_t r = 0; r < lwe_dim / grouping; ++r) {
        if (int rc = native_gadget_device(pl, digits, acc, nullptr, npolys, base_log, levels, CNTT_SRC_PLAIN, batch, st)) return rc;
        if (int rc = native_split_device(pl, digits, T, batch * nterms * n, false, st)) return rc;
        if (int rc = native_ntt_device(pl, T, batch * nterms, false, st)) return rc;
        if (int rc = native_multibit_accumulate_device(pl, O, T, rot_t + r * grouping * batch, F::key_at(pl, bsk, r * group_bytes, ks), nterms,
                                                       npolys, grouping, batch, st))
            return rc;
        if (int rc = native_ntt_device(pl, O, batch * npolys, true, st)) return rc;
        if (int rc = native_crt_device(pl, acc, O, batch * npolys * n, st)) return rc;
    }
    return CNTT_OK;
}

static const char *const MB_OUT[10] = {"out_ntt[0]", "out_ntt[1]", "out_ntt[2]", "out_ntt[3]", "out_ntt[4]",
                                       "out_ntt[5]", "out_ntt[6]", "out_ntt[7]", "out_ntt[8]", "out_ntt[9]"};
static const char *const MB_TERMS[10] = {"terms_ntt[0]", "terms_ntt[1]", "terms_ntt[2]", "terms_ntt[3]", "terms_ntt[4]",
                                         "terms_ntt[5]", "terms_ntt[6]", "terms_ntt[7]", "terms_ntt[8]", "terms_ntt[9]"};
static const char *const MB_KEY[10] = {"key_group[0]", "key_group[1]", "key_group[2]", "key_group[3]", "key_group[4]",
                                       "key_group[5]", "key_group[6]", "key_group[7]", "key_group[8]", "key_group[9]"};
static const char *const MB_BSK[10] = {"bsk_mb[0]", "bsk_mb[1]", "bsk_mb[2]", "bsk_mb[3]", "bsk_mb[4]",
                                       "bsk_mb[5]", "bsk_mb[6]", "bsk_mb[7]", "bsk_mb[8]", "bsk_mb[9]"};

static int native_multibit_accumulate(const cntt_native *pl, void *const *out, const void *const *terms, const uint32_t *rot_rows,
                                      const void *const *key, size_t nterms, size_t nout, unsigned grouping, size_t batch, cntt_mem_t where,
                                      hipStream_t st) {
    if (int rc = multibit_plan_check(pl)) return rc;
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
    if (where == CNTT_MEM_DEVICE) return native_multibit_accumulate_device(pl, out, terms, rot_rows, key, nterms, nout, grouping, batch, st);
    if (int rc = check_rot_host(pl->n, rot_rows, grouping * batch, "rot_rows")) return rc;
    Staging s(st);
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

// the argument checks the blind rotation and the bootstrap share: everything a step of the loop would refuse is refused here
static int native_multibit_check(const cntt_native *pl, const void *const *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log,
                                 unsigned levels, unsigned grouping, size_t batch, const void *workspace, size_t workspace_bytes, size_t need) {
    if (int rc = gadget_check<NativePbs>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (int rc = multibit_grouping_check(grouping)) return rc;
    if (lwe_dim % grouping) return fail(CNTT_EINVAL, "lwe_dim = %zu is not a multiple of grouping = %u", lwe_dim, grouping);
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    const u128 products = ((u128)(glwe_dim + 1) * levels) << grouping;
    if (products > (u128)pl->max_terms)
        return fail(CNTT_EINVAL,
                    "2^grouping * (glwe_dim + 1) * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range",
                    (size_t)products, pl->max_terms);
    if (batch == 0) return CNTT_OK;
    // what the sub-plans' transforms would refuse halfway through the call (the split and the CRT walk any count)
    const int logn = native_logn(pl), depth = logn > MaxLdsLogN<uint32_t>::value ? logn - MaxLdsLogN<uint32_t>::value : 0;
    if ((u128)batch * (glwe_dim + 1) * levels >= ((u128)1 << (32 - depth)))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * levels is too large for one transform launch");
    if (lwe_dim)
        if (int rc = NativePbs::key_check(pl, bsk, "bsk_mb")) return rc;
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    return CNTT_OK;
}
static size_t native_multibit_key_bytes(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, unsigned grouping) {
    return NativePbs::key_bytes(pl, ((lwe_dim / grouping) * (glwe_dim + 1) * levels * (glwe_dim + 1)) << grouping);
}
// the operands of both calls after `fixed` entries: the key planes and the workspace
static int multibit_operands(const cntt_native *pl, Operand *ops, int fixed, const void *const *bsk, size_t kb, const void *workspace,
                             size_t workspace_bytes) {
    int cnt = fixed;
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {MB_BSK[i], bsk[i], kb, sizeof(uint32_t), false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    return check_operands(ops, cnt);
}

static int native_multibit_blind_rotate(const cntt_native *pl, void *acc, const void *lut, int lut_per_element, const uint32_t *rot_t,
                                        const void *const *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                        unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                        hipStream_t st) {
    if (int rc = multibit_plan_check(pl)) return rc;
    if (batch && !rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (int rc = multibit_sizes_check(pl, lwe_dim, glwe_dim, levels, batch)) return rc;
    const MultibitSizes Z = multibit_sizes(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = native_multibit_check(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.rotate()))
        return rc;
    if (batch == 0) return CNTT_OK;
    if (!acc) return fail(CNTT_EINVAL, "acc is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t w = (size_t)pl->info.word, lb = lut_per_element ? Z.acc : Z.acc / batch;
    const size_t kb = native_multibit_key_bytes(pl, lwe_dim, glwe_dim, levels, grouping);
    Operand ops[14] = {{"acc", acc, Z.acc, w, true}, {"lut", lut, lb, w, false}, {"rot_t", rot_t, Z.rot, sizeof(uint32_t), false}};
    if (int rc = multibit_operands(pl, ops, 3, bsk, kb, workspace, workspace_bytes)) return rc;
    if (where == CNTT_MEM_DEVICE) {
        void *ws = workspace;
        if (!ws && lwe_dim) HIP_TRY(hipMallocAsync(&ws, Z.rotate(), st));   // one allocation for the whole loop
        const int rc = native_multibit_rotate_device(pl, acc, lut, lut_per_element != 0, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels,
                                                     grouping, batch, Z, static_cast<char *>(ws), st);
        if (!workspace && ws) (void)hipFreeAsync(ws, st);
        return rc;
    }
    if (int rc = check_rot_host(pl->n, rot_t, (lwe_dim + 1) * batch, "rot_t")) return rc;
    Staging s(st);
    NativePbs::KeyStore ks;
    const void *const *dkey = lwe_dim ? NativePbs::key_in(pl, s, bsk, kb, ks) : nullptr;
    const void *dlut = s.in(lut, lb);
    const uint32_t *drot = (const uint32_t *)s.in(rot_t, Z.rot);
    void *dacc = s.out(acc, Z.acc);
    char *dws = (char *)s.alloc(Z.rotate());
    if (int rc = s.status()) return rc;
    if (int rc = native_multibit_rotate_device(pl, dacc, dlut, lut_per_element != 0, drot, dkey, lwe_dim, glwe_dim, base_log, levels, grouping,
                                               batch, Z, dws, st))
        return rc;
    return s.finish();
}

// modulus switch -> multi-bit blind rotation -> extraction of coefficient 0 on device buffers; ws: digits | terms | outputs | rot_t | acc
static int native_multibit_bootstrap_device(const cntt_native *pl, void *lwe_out, const void *lwe_in, const void *lut, bool lut_per_element,
                                            const void *const *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                            unsigned grouping, size_t batch, const MultibitSizes &Z, char *ws, hipStream_t st) {
    using F = NativePbs;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + Z.rotate());
    void *acc = ws + Z.rotate() + up256(Z.rot);
    if (int rc = modswitch_device<F>(pl, rot_t, lwe_in, lwe_dim, batch, st)) return rc;
    if (int rc = native_multibit_rotate_device(pl, acc, lut, lut_per_element, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                               Z, ws, st))
        return rc;
    return extract_device<F>(pl, lwe_out, acc, glwe_dim, 0, batch, st);
}

static int native_multibit_bootstrap(const cntt_native *pl, void *lwe_out, const void *lwe_in, const void *lut, int lut_per_element,
                                     const void *const *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                     unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                     hipStream_t st) {
    using F = NativePbs;
    if (int rc = multibit_plan_check(pl)) return rc;
    if (int rc = multibit_sizes_check(pl, lwe_dim, glwe_dim, levels, batch)) return rc;
    const MultibitSizes Z = multibit_sizes(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = native_multibit_check(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.total()))
        return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t w = F::word(pl), ob = batch * (glwe_dim * pl->n + 1) * w, ib = batch * (lwe_dim + 1) * w;
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = native_multibit_key_bytes(pl, lwe_dim, glwe_dim, levels, grouping);
    Operand ops[14] = {{"lwe_out", lwe_out, ob, w, true}, {"lwe_in", lwe_in, ib, w, false}, {"lut", lut, lb, w, false}};
    if (int rc = multibit_operands(pl, ops, 3, bsk, kb, workspace, workspace_bytes)) return rc;
    if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    if (where == CNTT_MEM_DEVICE) {
        void *ws = workspace;
        if (!ws) HIP_TRY(hipMallocAsync(&ws, Z.total(), st));   // one allocation for the whole call
        const int rc = native_multibit_bootstrap_device(pl, lwe_out, lwe_in, lut, lut_per_element != 0, bsk, lwe_dim, glwe_dim, base_log,
                                                        levels, grouping, batch, Z, static_cast<char *>(ws), st);
        if (!workspace) (void)hipFreeAsync(ws, st);
        return rc;
    }
    Staging s(st);
    F::KeyStore ks;
    const void *const *dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : nullptr;
    const void *din = s.in(lwe_in, ib), *dlut = s.in(lut, lb);
    void *dout = s.out(lwe_out, ob);
    char *dws = (char *)s.alloc(Z.total());
    if (int rc = s.status()) return rc;
    if (int rc = native_multibit_bootstrap_device(pl, dout, din, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels,
                                                  grouping, batch, Z, dws, st))
        return rc;
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
    return native_multibit_blind_rotate(pl, acc, lut, lut_per_element, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                        workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" int cntt_native_multibit_bootstrap_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *lut,
                                                    int lut_per_element, const void *const *bsk_mb, size_t lwe_dim, size_t glwe_dim,
                                                    unsigned base_log, unsigned levels, unsigned grouping, size_t batch, void *workspace,
                                                    size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return native_multibit_bootstrap(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, batch,
                                     workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_multibit_pbs_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,
                                                           unsigned, size_t batch) {
    if (!pl || pl->info.is52 || !multibit_sizes_fit(pl, lwe_dim, glwe_dim, levels, batch)) return 0;
    return multibit_sizes(pl, lwe_dim, glwe_dim, levels, batch).total();
}
