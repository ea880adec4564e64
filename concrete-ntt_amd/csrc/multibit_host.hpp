// The host side of the multi-bit blind rotation and bootstrap, once for the native plans (include/cntt_multibit.h, host_native_ext.hip
// through host_native_multibit.inc) and the prime plans (include/cntt_prime_multibit.h, host_prime.hip through host_prime_multibit.inc):
// argument checks, the workspace layout and the loop over the groups, each call on one path for device pointers and host slices
// through Staging (host_common.hpp).  Internal, never installed.  Templates over
// a family F as in pbs_host.hpp, which this file builds on: the bootstrap family plus the multibit_* members NativePbs
// (host_native_ext.hip) and PrimePbs<T> (host_prime_pbs.inc) show.  The stand-alone *_multibit_accumulate_batch calls stay with their
// families (residue planes on one side, plain buffers on the other) and share the grouping check only.
#pragma once
#include "pbs_host.hpp"

#pragma GCC visibility push(hidden)

// what both kernels take (each .inc holds it against its kernel header's constant)
constexpr unsigned MULTIBIT_MAX_GROUPING = 4;
inline int multibit_grouping_check(unsigned grouping) {
    if (grouping == 0 || grouping > MULTIBIT_MAX_GROUPING)
        return fail(CNTT_EINVAL, "grouping = %u is not in 1 ... %u", grouping, MULTIBIT_MAX_GROUPING);
    return CNTT_OK;
}

// The parts of the workspace, in bytes and in this order (cntt_multibit.h and cntt_prime_multibit.h state the formulas): the digits, the
// family's scratch (F::multibit_scratch -- native: term planes and output planes, prime: none), rot_t, the accumulator.  The blind
// rotation takes what lies before rot_t.  Without scratch that is the digits alone and nothing follows them to align, so their size
// stays unrounded; the layout and the total are then those of PbsSizes, up256(0) being 0.
struct MultibitSizes {
    size_t digits, scratch[2], rot, acc;
    size_t rot_offset() const { return up256(digits) + up256(scratch[0]) + up256(scratch[1]); }
    size_t rotate() const { return scratch[0] || scratch[1] ? rot_offset() : digits; }
    size_t total() const { return rot_offset() + up256(rot) + up256(acc); }
};
template <class F> MultibitSizes multibit_sizes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const PbsSizes P = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    MultibitSizes Z{P.digits, {0, 0}, P.rot, P.acc};
    F::multibit_scratch(pl, batch * (glwe_dim + 1), levels, Z.scratch);
    return Z;
}
// F::multibit_supported: the plan has the calls at all; F::multibit_sizes_fit: no part of the workspace wraps
template <class F>
size_t multibit_pbs_workspace_bytes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    if (!pl || !F::multibit_supported(pl) || !F::multibit_sizes_fit(pl, lwe_dim, glwe_dim, levels, batch)) return 0;
    return multibit_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch).total();
}
// the refusals that come before any size is formed; the caller has checked pl
template <class F> int multibit_sizes_check(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    if (!F::multibit_sizes_fit(pl, lwe_dim, glwe_dim, levels, batch))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * levels * ntt_size or (lwe_dim + 1) * batch is too large: the workspace would not fit 2^62 bytes");
    return CNTT_OK;
}

// acc = X^(body row of rot_t) lut, then per group: digits of acc (PLAIN), and the family's step from the digits to the new acc
// (F::multibit_step -- prime: fwd in place -> the bundle's pointwise step into acc -> inv; native: residue planes -> fwd -> the
// pointwise step into the output planes -> inv -> CRT into acc).  Writing acc at the end of the step is sound in stream order: its old
// words are dead once the digits exist.  ws: digits | scratch.
template <class F>
int multibit_rotate_device(const typename F::Plan *pl, typename F::Word *acc, const typename F::Word *lut, bool lut_per_element,
                           const uint32_t *rot_t, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                           unsigned grouping, size_t batch, const MultibitSizes &Z, char *ws, hipStream_t st) {
    using W = typename F::Word;
    const size_t npolys = glwe_dim + 1, nterms = npolys * levels, n = pl->n, w = F::word(pl);
    const size_t group_bytes = F::key_bytes(pl, (nterms * npolys) << grouping);   // one group's key
    const hipError_t e = F::launch_pbs_init(pl, acc, lut, rot_t + lwe_dim * batch, (uint32_t)npolys, lut_per_element, batch,
                                            batch * npolys * n * w > STREAM_BYTES, ew_grid(batch * npolys * n * w / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_pbs_init_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    typename F::KeyStore ks;
    for (size_t r = 0; r < lwe_dim / grouping; ++r) {   // (no groups: ws may be NULL)
        W *digits = static_cast<W *>(static_cast<void *>(ws));
        if (int rc = F::gadget(pl, digits, acc, nullptr, npolys, base_log, levels, CNTT_SRC_PLAIN, batch, st)) return rc;
        if (int rc = F::multibit_step(pl, acc, digits, ws + up256(Z.digits), Z, rot_t + r * grouping * batch,
                                      F::key_at(pl, bsk, r * group_bytes, ks), nterms, npolys, grouping, batch, st))
            return rc;
    }
    return CNTT_OK;
}

// the argument checks the blind rotation and the bootstrap share: everything a step of the loop would refuse is refused here
template <class F>
int multibit_check(const typename F::Plan *pl, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                   unsigned grouping, size_t batch, const void *workspace, size_t workspace_bytes, size_t need) {
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (int rc = multibit_grouping_check(grouping)) return rc;
    if (lwe_dim % grouping) return fail(CNTT_EINVAL, "lwe_dim = %zu is not a multiple of grouping = %u", lwe_dim, grouping);
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = F::multibit_check_terms(pl, glwe_dim, levels, grouping)) return rc;
    if (batch == 0) return CNTT_OK;
    // what the transforms would refuse halfway through the call (the native split and CRT walk any count)
    const int depth = F::logn(pl) > F::MAX_LDS_LOGN ? F::logn(pl) - F::MAX_LDS_LOGN : 0;
    if ((u128)batch * (glwe_dim + 1) * levels >= ((u128)1 << (32 - depth)))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * levels is too large for one transform launch");
    if (lwe_dim)
        if (int rc = F::key_check(pl, bsk, "bsk_mb")) return rc;
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    return CNTT_OK;
}
template <class F> size_t multibit_key_bytes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, unsigned grouping) {
    return F::key_bytes(pl, ((lwe_dim / grouping) * (glwe_dim + 1) * levels * (glwe_dim + 1)) << grouping);
}
// the operands of both calls after the 3 entries of their own: the key as the family lists it (F::multibit_key_operands, which returns
// the new count) and the workspace
constexpr int MULTIBIT_MAX_OPERANDS = 3 + 10 + 1;
template <class F>
int multibit_operands(const typename F::Plan *pl, Operand *ops, typename F::Key bsk, size_t kb, const void *workspace, size_t workspace_bytes) {
    int cnt = F::multibit_key_operands(pl, ops, 3, bsk, kb);
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    return check_operands(ops, cnt);
}

template <class F>
int multibit_blind_rotate(const typename F::Plan *pl, typename F::Word *acc, const typename F::Word *lut, int lut_per_element,
                          const uint32_t *rot_t, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                          unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = F::multibit_plan_check(pl)) return rc;
    if (batch && !rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (int rc = multibit_sizes_check<F>(pl, lwe_dim, glwe_dim, levels, batch)) return rc;
    const MultibitSizes Z = multibit_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = multibit_check<F>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.rotate()))
        return rc;
    if (batch == 0) return CNTT_OK;
    if (!acc) return fail(CNTT_EINVAL, "acc is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t w = F::word(pl), lb = lut_per_element ? Z.acc : Z.acc / batch;
    const size_t kb = multibit_key_bytes<F>(pl, lwe_dim, glwe_dim, levels, grouping);
    Operand ops[MULTIBIT_MAX_OPERANDS] = {{"acc", acc, Z.acc, w, true}, {"lut", lut, lb, w, false}, {"rot_t", rot_t, Z.rot, sizeof(uint32_t), false}};
    if (int rc = multibit_operands<F>(pl, ops, bsk, kb, workspace, workspace_bytes)) return rc;
    Staging s(where, st);
    if (s.host())
        if (int rc = check_rot_host(pl->n, rot_t, (lwe_dim + 1) * batch, "rot_t")) return rc;
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : typename F::Key{};
    const W *dlut = (const W *)s.in(lut, lb);
    const uint32_t *drot = (const uint32_t *)s.in(rot_t, Z.rot);
    W *dacc = (W *)s.out(acc, Z.acc);
    char *dws = (char *)s.workspace(workspace, Z.rotate(), lwe_dim != 0);   // one block for the whole loop
    if (int rc = s.status()) return rc;
    if (int rc = multibit_rotate_device<F>(pl, dacc, dlut, lut_per_element != 0, drot, dkey, lwe_dim, glwe_dim, base_log, levels, grouping,
                                           batch, Z, dws, st))
        return rc;
    return s.finish();
}

// modulus switch -> multi-bit blind rotation -> extraction of coefficient 0 on device buffers; ws: digits | scratch | rot_t | acc
template <class F>
int multibit_bootstrap_device(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *lut,
                              bool lut_per_element, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                              unsigned grouping, size_t batch, const MultibitSizes &Z, char *ws, hipStream_t st) {
    using W = typename F::Word;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + Z.rot_offset());
    W *acc = static_cast<W *>(static_cast<void *>(ws + Z.rot_offset() + up256(Z.rot)));
    if (int rc = modswitch_device<F>(pl, rot_t, lwe_in, lwe_dim, batch, st)) return rc;
    if (int rc = multibit_rotate_device<F>(pl, acc, lut, lut_per_element, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, Z,
                                           ws, st))
        return rc;
    return extract_device<F>(pl, lwe_out, acc, glwe_dim, 0, batch, st);
}

template <class F>
int multibit_bootstrap(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *lut,
                       int lut_per_element, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                       unsigned grouping, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = F::multibit_plan_check(pl)) return rc;
    if (int rc = multibit_sizes_check<F>(pl, lwe_dim, glwe_dim, levels, batch)) return rc;
    const MultibitSizes Z = multibit_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = multibit_check<F>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, grouping, batch, workspace, workspace_bytes, Z.total()))
        return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t w = F::word(pl), ob = batch * (glwe_dim * pl->n + 1) * w, ib = batch * (lwe_dim + 1) * w;
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = multibit_key_bytes<F>(pl, lwe_dim, glwe_dim, levels, grouping);
    Operand ops[MULTIBIT_MAX_OPERANDS] = {{"lwe_out", lwe_out, ob, w, true}, {"lwe_in", lwe_in, ib, w, false}, {"lut", lut, lb, w, false}};
    if (int rc = multibit_operands<F>(pl, ops, bsk, kb, workspace, workspace_bytes)) return rc;
    if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    Staging s(where, st);
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : typename F::Key{};
    const W *din = (const W *)s.in(lwe_in, ib), *dlut = (const W *)s.in(lut, lb);
    W *dout = (W *)s.out(lwe_out, ob);
    char *dws = (char *)s.workspace(workspace, Z.total());   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = multibit_bootstrap_device<F>(pl, dout, din, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels, grouping,
                                              batch, Z, dws, st))
        return rc;
    return s.finish();
}

#pragma GCC visibility pop
