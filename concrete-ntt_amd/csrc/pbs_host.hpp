// The host side of the programmable bootstrap, once for the native plans (include/cntt_pbs.h, host_native_ext.hip) and the prime plans
// (include/cntt_prime_pbs.h, host_prime.hip): argument checks, the workspace layout and the blind rotation loop.  Every call is one
// path for device pointers and host slices: after its checks it takes its operands and its workspace from a Staging(where, stream)
// (host_common.hpp) and runs its _device function on them; only check_rot_host asks which of the two it is.
// Internal, never installed.  Every function here is a template over a family F, one struct of static members per plan family that supplies
// what the two differ in and nothing else: NativePbs (host_native_ext.hip) and PrimePbs<T> (host_prime_pbs.inc) show the members.
// lwe_host.hpp, on top of this file, does the same for the keyswitch, the keyswitch + bootstrap call and the packing keyswitch, and
// multibit_host.hpp for the multi-bit blind rotation and bootstrap, and cbs_host.hpp for the circuit bootstrap and the many-LUT calls.
#pragma once
#include "host_common.hpp"

#pragma GCC visibility push(hidden)

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// one gadget: `pre` is the prefix of its two arguments' names ("", or "ks_", "pbs_", "cbs_" where a call has several)
template <class F> int digits_check(const typename F::Plan *pl, const char *pre, unsigned base_log, unsigned levels) {
    const unsigned wbits = F::digit_bits(pl);
    if (base_log == 0) return fail(CNTT_EINVAL, "%sbase_log is 0", pre);
    if (levels == 0) return fail(CNTT_EINVAL, "%slevels is 0", pre);
    if ((uint64_t)base_log * levels > wbits) return fail(CNTT_EINVAL, F::DIGIT_BUDGET_MSG, pre, pre, base_log, levels, wbits);
    return CNTT_OK;
}
// the checks every call with digits and a source mode shares
template <class F> int gadget_check(const typename F::Plan *pl, unsigned base_log, unsigned levels, int mode, const uint32_t *rot) {
    if (int rc = digits_check<F>(pl, "", base_log, levels)) return rc;
    if (mode != CNTT_SRC_PLAIN && mode != CNTT_SRC_ROTATE && mode != CNTT_SRC_CMUX) return fail(CNTT_EINVAL, "src_mode %d is not a cntt_src_mode_t", mode);
    if (mode != CNTT_SRC_PLAIN && !rot) return fail(CNTT_EINVAL, "rot is NULL and src_mode reads it");
    return CNTT_OK;
}
// host path: the rotation exponents are in reach, so one that is not below 2n is an error there (`name`: the argument in the message)
inline int check_rot_host(size_t n, const uint32_t *rot, size_t count, const char *name) {
    for (size_t i = 0; i < count; ++i)
        if ((size_t)rot[i] >= 2 * n) return fail(CNTT_EINVAL, "%s[%zu] = %u is not below 2n = %zu", name, i, rot[i], 2 * n);
    return CNTT_OK;
}
// a workspace the caller brought: aligned, and `need` bytes at least
inline int check_workspace(const void *workspace, size_t workspace_bytes, size_t need) {
    if ((uintptr_t)workspace % 16) return fail(CNTT_EINVAL, "workspace is not 16-byte aligned");
    if (workspace_bytes < need) return fail(CNTT_EINVAL, "workspace_bytes = %zu is below the %zu bytes this call needs", workspace_bytes, need);
    return CNTT_OK;
}

template <class F>
int gadget_decompose(const typename F::Plan *pl, typename F::Word *terms, const typename F::Word *polys, const uint32_t *rot, size_t npolys,
                     unsigned base_log, unsigned levels, int mode, size_t batch, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check<F>(pl, base_log, levels, mode, rot)) return rc;
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (!terms || !polys) return fail(CNTT_EINVAL, "NULL argument");
    const size_t pb = batch * npolys * pl->n * F::word(pl), tb = pb * levels;
    if (ranges_overlap(terms, tb, polys, pb)) return fail(CNTT_EINVAL, "terms overlaps polys");
    const bool rotated = mode != CNTT_SRC_PLAIN;
    Staging s(where, st);
    if (s.host() && rotated)
        if (int rc = check_rot_host(pl->n, rot, batch, "rot")) return rc;
    W *dt = (W *)s.out(terms, tb);
    const W *dp = (const W *)s.in(polys, pb);
    const uint32_t *dr = rotated ? (const uint32_t *)s.in(rot, batch * sizeof(uint32_t)) : nullptr;
    if (int rc = s.status()) return rc;
    if (int rc = F::gadget(pl, dt, dp, dr, npolys, base_log, levels, mode, batch, st)) return rc;
    return s.finish();
}

// the three parts of the workspace, in bytes and in this order (cntt_pbs.h and cntt_prime_pbs.h state the formula)
struct PbsSizes {
    size_t digits, rot, acc;
    size_t total() const { return up256(digits) + up256(rot) + up256(acc); }
};
template <class F> PbsSizes pbs_sizes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const size_t pb = batch * (glwe_dim + 1) * pl->n * F::word(pl);
    return PbsSizes{pb * levels, (lwe_dim + 1) * batch * sizeof(uint32_t), pb};
}
template <class F> size_t pbs_workspace_bytes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    return pl ? pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch).total() : 0;
}

template <class F>
int modswitch_device(const typename F::Plan *pl, uint32_t *rot_t, const typename F::Word *lwe, size_t lwe_dim, size_t batch, hipStream_t st) {
    if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    const size_t tiles = ((lwe_dim + F::TILE) / F::TILE) * ((batch + F::TILE - 1) / F::TILE);
    const hipError_t e = F::launch_modswitch(pl, rot_t, lwe, lwe_dim, batch, ew_grid(tiles * 256), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_lwe_modswitch_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}
template <class F>
int extract_device(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *glwe, size_t glwe_dim, size_t index,
                   size_t batch, hipStream_t st) {
    const hipError_t e = F::launch_sample_extract(pl, lwe_out, glwe, glwe_dim, (uint32_t)index, batch, ew_grid(batch * (glwe_dim * pl->n + 1)), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_sample_extract_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}
// acc = X^(body row of rot_t) lut, then lwe_dim times decomposition (CMux difference) into `digits` and the external product accumulating
// into acc.  In place is sound: the digits are complete before the product starts (stream order), the product reads only the digits and
// the key besides the output words it adds to, and each of its launches reads and writes only its own outputs.
template <class F>
int blind_rotate_device(const typename F::Plan *pl, typename F::Word *acc, const typename F::Word *lut, bool lut_per_element,
                        const uint32_t *rot_t, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                        size_t batch, typename F::Word *digits, hipStream_t st) {
    const size_t npolys = glwe_dim + 1, nterms = npolys * levels, n = pl->n, w = F::word(pl);
    const size_t slice = F::key_bytes(pl, nterms * npolys);   // one iteration's key
    const hipError_t e = F::launch_pbs_init(pl, acc, lut, rot_t + lwe_dim * batch, (uint32_t)npolys, lut_per_element, batch,
                                            batch * npolys * n * w > STREAM_BYTES, ew_grid(batch * npolys * n * w / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_pbs_init_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    typename F::KeyStore ks;
    for (size_t i = 0; i < lwe_dim; ++i) {
        if (int rc = F::gadget(pl, digits, acc, rot_t + i * batch, npolys, base_log, levels, CNTT_SRC_CMUX, batch, st)) return rc;
        if (int rc = F::ext_product(pl, acc, digits, F::key_at(pl, bsk, i * slice, ks), nterms, npolys, batch, true, st)) return rc;
    }
    return CNTT_OK;
}

template <class F>
int lwe_modswitch(const typename F::Plan *pl, uint32_t *rot_t, const typename F::Word *lwe, size_t lwe_dim, size_t batch, cntt_mem_t where,
                  hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch == 0) return CNTT_OK;
    if (!rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (!lwe) return fail(CNTT_EINVAL, "lwe is NULL");
    const size_t rb = (lwe_dim + 1) * batch * sizeof(uint32_t), lb = (lwe_dim + 1) * batch * F::word(pl);
    if (ranges_overlap(rot_t, rb, lwe, lb)) return fail(CNTT_EINVAL, "rot_t overlaps lwe");
    Staging s(where, st);
    uint32_t *dr = (uint32_t *)s.out(rot_t, rb);
    const typename F::Word *dl = (const typename F::Word *)s.in(lwe, lb);
    if (int rc = s.status()) return rc;
    if (int rc = modswitch_device<F>(pl, dr, dl, lwe_dim, batch, st)) return rc;
    return s.finish();
}

template <class F>
int sample_extract(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *glwe, size_t glwe_dim, size_t index,
                   size_t batch, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (index >= pl->n) return fail(CNTT_EINVAL, "index = %zu is not below ntt_size = %zu", index, pl->n);
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!glwe) return fail(CNTT_EINVAL, "glwe is NULL");
    const size_t w = F::word(pl), ob = batch * (glwe_dim * pl->n + 1) * w, gb = batch * (glwe_dim + 1) * pl->n * w;
    if (ranges_overlap(lwe_out, ob, glwe, gb)) return fail(CNTT_EINVAL, "lwe_out overlaps glwe");
    Staging s(where, st);
    W *dout = (W *)s.out(lwe_out, ob);
    const W *dg = (const W *)s.in(glwe, gb);
    if (int rc = s.status()) return rc;
    if (int rc = extract_device<F>(pl, dout, dg, glwe_dim, index, batch, st)) return rc;
    return s.finish();
}

// the argument checks blind_rotate and bootstrap share; `need` = what the workspace must hold
template <class F>
int pbs_check(const typename F::Plan *pl, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
              const void *workspace, size_t workspace_bytes, size_t need) {
    const uint32_t some_rot = 0;
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_CMUX, &some_rot)) return rc;
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = F::check_terms(pl, glwe_dim, levels)) return rc;
    if (batch == 0) return CNTT_OK;
    if (lwe_dim)
        if (int rc = F::key_check(pl, bsk, "bsk_ntt")) return rc;
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    return CNTT_OK;
}

template <class F>
int blind_rotate(const typename F::Plan *pl, typename F::Word *acc, const typename F::Word *lut, int lut_per_element, const uint32_t *rot_t,
                 typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                 size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch && !rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = pbs_check<F>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, Z.digits)) return rc;
    if (batch == 0) return CNTT_OK;
    if (!acc) return fail(CNTT_EINVAL, "acc is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch;
    if (ranges_overlap(acc, Z.acc, lut, lb)) return fail(CNTT_EINVAL, "acc overlaps lut");
    if (ranges_overlap(acc, Z.acc, rot_t, Z.rot)) return fail(CNTT_EINVAL, "acc overlaps rot_t");
    if (workspace && ranges_overlap(acc, Z.acc, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "acc overlaps workspace");
    Staging s(where, st);
    if (s.host())
        if (int rc = check_rot_host(pl->n, rot_t, (lwe_dim + 1) * batch, "rot_t")) return rc;
    const size_t kb = F::key_bytes(pl, lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1));
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : typename F::Key{};
    const W *dlut = (const W *)s.in(lut, lb);
    const uint32_t *drot = (const uint32_t *)s.in(rot_t, Z.rot);
    W *dacc = (W *)s.out(acc, Z.acc), *ddig = (W *)s.workspace(workspace, Z.digits, lwe_dim != 0);   // one block for the whole loop
    if (int rc = s.status()) return rc;
    if (int rc = blind_rotate_device<F>(pl, dacc, dlut, lut_per_element != 0, drot, dkey, lwe_dim, glwe_dim, base_log, levels, batch, ddig, st))
        return rc;
    return s.finish();
}

// modulus switch -> blind rotation -> extraction of coefficient 0 on device buffers; ws holds digits | rot_t | acc (PbsSizes)
template <class F>
int bootstrap_device(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *lut,
                     bool lut_per_element, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
                     const PbsSizes &Z, char *ws, hipStream_t st) {
    using W = typename F::Word;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    W *acc = static_cast<W *>(static_cast<void *>(ws + up256(Z.digits) + up256(Z.rot)));
    if (int rc = modswitch_device<F>(pl, rot_t, lwe_in, lwe_dim, batch, st)) return rc;
    if (int rc = blind_rotate_device<F>(pl, acc, lut, lut_per_element, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, batch,
                                        static_cast<W *>(static_cast<void *>(ws)), st))
        return rc;
    return extract_device<F>(pl, lwe_out, acc, glwe_dim, 0, batch, st);
}

template <class F>
int bootstrap(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *lut,
              int lut_per_element, typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
              void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = pbs_check<F>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, Z.total())) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t w = F::word(pl), ob = batch * (glwe_dim * pl->n + 1) * w, ib = batch * (lwe_dim + 1) * w;
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch;
    if (ranges_overlap(lwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "lwe_out overlaps lwe_in");
    if (ranges_overlap(lwe_out, ob, lut, lb)) return fail(CNTT_EINVAL, "lwe_out overlaps lut");
    if (workspace) {
        if (ranges_overlap(lwe_out, ob, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_out overlaps workspace");
        if (ranges_overlap(lwe_in, ib, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_in overlaps workspace");
        if (ranges_overlap(lut, lb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lut overlaps workspace");
    }
    const size_t kb = F::key_bytes(pl, lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1));
    Staging s(where, st);
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : typename F::Key{};
    const W *din = (const W *)s.in(lwe_in, ib), *dlut = (const W *)s.in(lut, lb);
    W *dout = (W *)s.out(lwe_out, ob);
    char *dws = (char *)s.workspace(workspace, Z.total());   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = bootstrap_device<F>(pl, dout, din, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels, batch, Z, dws, st))
        return rc;
    return s.finish();
}

#pragma GCC visibility pop
