// The host side of the circuit bootstrap from LWE bits to GGSW selectors and of the many-LUT calls, once for the native plans
// (include/cntt_cbs.h, cntt_manylut.h; host_native_ext.hip through host_native_cbs.inc) and the prime plans (include/cntt_prime_cbs.h,
// cntt_prime_manylut.h; host_prime.hip through host_prime_cbs.inc): argument checks, the workspace layout and the launch sequences, each
// call on one path for device pointers and host slices through Staging (host_common.hpp).  Internal, never installed.  Templates over a
// family F as in pbs_host.hpp, which this file builds on: the bootstrap family plus the members the last part of NativePbs
// (host_native_ext.hip) and of PrimePbs<T> (host_prime_pbs.inc) show.  The circuit bootstrap exists in two variants that share every
// function here: one rotation per input bit and level (log_lut == nullptr), and one rotation per input bit whose table holds
// 2^*log_lut values, one per level (the one-rotation form of the many-LUT headers).
#pragma once
#include "pbs_host.hpp"

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------------------------------------
// the many-LUT bootstrap and its two ends
// ---------------------------------------------------------------------------------------------
template <class F> int manylut_check_log(const typename F::Plan *pl, unsigned log_lut) {
    if (log_lut > (unsigned)F::logn(pl)) return fail(CNTT_EINVAL, "log_lut_count = %u exceeds log2(ntt_size) = %d", log_lut, F::logn(pl));
    if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    return CNTT_OK;
}
// 32 x 32 tiles of the transposing modulus switches
template <class F> size_t modswitch_tiles(size_t lwe_dim, size_t batch) { return ((lwe_dim + F::TILE) / F::TILE) * ((batch + F::TILE - 1) / F::TILE); }

template <class F>
int modswitch_manylut_device(const typename F::Plan *pl, uint32_t *rot_t, const typename F::Word *lwe, size_t lwe_dim, unsigned log_lut,
                             size_t batch, hipStream_t st) {
    const hipError_t e = F::launch_modswitch_manylut(pl, rot_t, lwe, log_lut, lwe_dim, batch, ew_grid(modswitch_tiles<F>(lwe_dim, batch) * 256), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_modswitch_manylut_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}
template <class F>
int extract_many_device(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *glwe, size_t k, size_t count, size_t batch,
                        hipStream_t st) {
    const size_t n = pl->n, w = F::word(pl), chunks = (count + F::EXTRACT_MANY_ROWS - 1) / F::EXTRACT_MANY_ROWS;
    const size_t items = batch * k * chunks * (n * w / 16) + batch * count;
    // the output against STREAM_BYTES, as the other element-wise kernels decide it
    const hipError_t e = F::launch_extract_many(pl, lwe_out, glwe, k, count, batch, batch * count * (k * n + 1) * w > STREAM_BYTES, ew_grid(items), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_sample_extract_many_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}

template <class F>
int lwe_modswitch_manylut(const typename F::Plan *pl, uint32_t *rot_t, const typename F::Word *lwe, size_t lwe_dim, unsigned log_lut, size_t batch,
                          cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = manylut_check_log<F>(pl, log_lut)) return rc;
    const size_t w = F::word(pl);
    if (product_passes_2_63({batch, lwe_dim + 1, w}) || lwe_dim + 1 == 0)
        return fail(CNTT_EINVAL, "lwe_dim = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", lwe_dim, batch);
    if (batch == 0) return CNTT_OK;
    if (!rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (!lwe) return fail(CNTT_EINVAL, "lwe is NULL");
    const size_t rb = (lwe_dim + 1) * batch * sizeof(uint32_t), lb = (lwe_dim + 1) * batch * w;
    const Operand ops[2] = {{"rot_t", rot_t, rb, sizeof(uint32_t), true}, {"lwe", lwe, lb, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    uint32_t *dr = (uint32_t *)s.out(rot_t, rb);
    const typename F::Word *dl = (const typename F::Word *)s.in(lwe, lb);
    if (int rc = s.status()) return rc;
    if (int rc = modswitch_manylut_device<F>(pl, dr, dl, lwe_dim, log_lut, batch, st)) return rc;
    return s.finish();
}

// F::extract_many_check: what the family's extraction kernel asks of the plan
template <class F>
int sample_extract_many(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *glwe, size_t k, size_t count, size_t batch,
                        cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (count == 0 || count > pl->n) return fail(CNTT_EINVAL, "count = %zu is not in 1 .. ntt_size = %zu", count, pl->n);
    if (int rc = F::extract_many_check(pl)) return rc;
    const size_t n = pl->n, w = F::word(pl);
    if (k + 1 == 0 || product_passes_2_63({batch, count, k, n, w}) || product_passes_2_63({batch, count + k + 1, n, w}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, count = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", k, count, batch);
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!glwe) return fail(CNTT_EINVAL, "glwe is NULL");
    const size_t ob = batch * count * (k * n + 1) * w, gb = batch * (k + 1) * n * w;
    const Operand ops[2] = {{"lwe_out", lwe_out, ob, w, true}, {"glwe", glwe, gb, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    W *dout = (W *)s.out(lwe_out, ob);
    const W *dg = (const W *)s.in(glwe, gb);
    if (int rc = s.status()) return rc;
    if (int rc = extract_many_device<F>(pl, dout, dg, k, count, batch, st)) return rc;
    return s.finish();
}

// the operands of a call after `cnt` entries of its own: the bootstrapping key as the family lists it (F::bsk_operands, which returns the
// new count), what `last` names (nullptr: nothing) and the workspace
constexpr int CBS_MAX_OPERANDS = 10 + 1 + 10 + 1 + 1;
template <class F>
int key_and_workspace_operands(const typename F::Plan *pl, Operand *ops, int cnt, typename F::Key bsk, size_t kb, const Operand *last,
                               const void *workspace, size_t workspace_bytes) {
    cnt = F::bsk_operands(pl, ops, cnt, bsk, kb);
    if (last) ops[cnt++] = *last;
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    return check_operands(ops, cnt);
}

// the coarse modulus switch -> the blind rotation -> the extraction of the indices 0 .. lut_count - 1; ws holds digits | rot_t | acc
// (PbsSizes), as bootstrap_device
template <class F>
int bootstrap_manylut(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *lut,
                      int lut_per_element, typename F::Key bsk, size_t lwe_dim, size_t k, unsigned base_log, unsigned levels, unsigned log_lut,
                      size_t lut_count, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = manylut_check_log<F>(pl, log_lut)) return rc;
    if (lut_count == 0 || lut_count > ((size_t)1 << log_lut))
        return fail(CNTT_EINVAL, "lut_count = %zu is not in 1 .. 2^log_lut_count = %zu", lut_count, (size_t)1 << log_lut);
    if (int rc = F::extract_many_check(pl)) return rc;
    const size_t n = pl->n, w = F::word(pl), lv = levels ? levels : 1;
    if (k + 1 == 0 || lwe_dim + 1 == 0 || product_passes_2_63({batch, lwe_dim + 1, w}) || product_passes_2_63({batch, k + 1, lv, n, w}) ||
        product_passes_2_63({batch, lut_count, k + 1, n, w}) || product_passes_2_63({lwe_dim, k + 1, lv, k + 1, n, F::key_word(pl)}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the key or the workspace pass 2^63 bytes", lwe_dim, k,
                    batch);
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, k, levels, batch);
    if (int rc = pbs_check<F>(pl, bsk, lwe_dim, k, base_log, levels, batch, workspace, workspace_bytes, Z.total())) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t ob = batch * lut_count * (k * n + 1) * w, ib = batch * (lwe_dim + 1) * w;
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch, kb = F::key_bytes(pl, lwe_dim * (k + 1) * levels * (k + 1));
    Operand ops[CBS_MAX_OPERANDS] = {{"lwe_out", lwe_out, ob, w, true}, {"lwe_in", lwe_in, ib, w, false}, {"lut", lut, lb, w, false}};
    if (int rc = key_and_workspace_operands<F>(pl, ops, 3, bsk, kb, nullptr, workspace, workspace_bytes)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : typename F::Key{};
    const W *din = (const W *)s.in(lwe_in, ib), *dlut = (const W *)s.in(lut, lb);
    W *dout = (W *)s.out(lwe_out, ob);
    char *ws = (char *)s.workspace(workspace, Z.total());   // one block for the whole call
    if (int rc = s.status()) return rc;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    W *acc = static_cast<W *>(static_cast<void *>(ws + up256(Z.digits) + up256(Z.rot)));
    if (int rc = modswitch_manylut_device<F>(pl, rot_t, din, lwe_dim, log_lut, batch, st)) return rc;
    if (int rc = blind_rotate_device<F>(pl, acc, dlut, lut_per_element != 0, rot_t, dkey, lwe_dim, k, base_log, levels, batch,
                                        static_cast<W *>(static_cast<void *>(ws)), st))
        return rc;
    if (int rc = extract_many_device<F>(pl, dout, acc, k, lut_count, batch, st)) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------
// the circuit bootstrap from LWE bits to GGSW selectors, per bit and level or with one rotation per bit
// ---------------------------------------------------------------------------------------------
// The parts of the workspace, in bytes and in this order (the four headers state the formulas): rot_t, the table, the digits of the
// rotation, the accumulators, the int32 digits of the keyswitch, the slab partials, and the selector words where the family sums into
// words before it makes the output (F::CBS_SEL: native; prime sums into the output and has no such part, up256(0) being 0).  The first
// four are per rotation: E = batch * cbs_levels of them, or -- one_rotation -- batch of them over one shared table.
template <class F> struct CbsSizes {
    size_t rot, table, pbs_digits, acc, ks_digits, part, sel;
    typename F::CbsShape shape;
    size_t total() const { return up256(rot) + up256(table) + up256(pbs_digits) + up256(acc) + up256(ks_digits) + up256(part) + up256(sel); }
};
template <class F>
CbsSizes<F> cbs_sizes(const typename F::Plan *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                      size_t batch, bool one_rotation) {
    const size_t w = F::word(pl), e = batch * cbs_levels, rotations = one_rotation ? batch : e, r = (k * pl->n + 1) * ks_levels,
                 ct = (k + 1) * pl->n * w;
    CbsSizes<F> Z;
    Z.shape = F::cbs_shape(pl->n, w, k, r, e);
    Z.rot = (lwe_dim + 1) * rotations * sizeof(uint32_t);
    Z.table = (one_rotation ? 1 : e) * ct;
    Z.pbs_digits = rotations * ct * pbs_levels;
    Z.acc = rotations * ct;
    Z.ks_digits = e * r * sizeof(int32_t);
    Z.part = Z.shape.slabs * (k + 1) * e * ct;
    Z.sel = F::CBS_SEL ? (k + 1) * e * ct : 0;
    return Z;
}
template <class F>
size_t cbs_workspace_bytes(const typename F::Plan *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                           size_t batch, bool one_rotation) {
    return pl ? cbs_sizes<F>(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch, one_rotation).total() : 0;
}

// set-up (the modulus switch of lwe + a quarter and the table or tables) -> one blind rotation over all the rotations -> extraction and
// signed digits -> the digit x key product in slabs -> the sum of the slabs, negated, in the selector layout -> F::cbs_finish (native:
// the split into residues and the forward transforms into the caller's planes; prime: nothing).  out: the planes of F::cbs_out_planes.
template <class F>
int circuit_bootstrap_device(const typename F::Plan *pl, void *const *out, const typename F::Word *lwe_in, typename F::Key bsk,
                             const typename F::Word *fpksk, size_t lwe_dim, size_t k, unsigned pbs_base_log, unsigned pbs_levels,
                             unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, const unsigned *log_lut,
                             size_t batch, const CbsSizes<F> &Z, char *ws, hipStream_t st) {
    using W = typename F::Word;
    const size_t e = batch * cbs_levels, rotations = log_lut ? batch : e, n = pl->n, r = (k * n + 1) * ks_levels;
    char *at = ws;
    const auto part_of = [&at](size_t bytes) {
        char *here = at;
        at += up256(bytes);
        return static_cast<void *>(here);
    };
    uint32_t *rot_t = static_cast<uint32_t *>(part_of(Z.rot));
    W *table = static_cast<W *>(part_of(Z.table)), *pbs_digits = static_cast<W *>(part_of(Z.pbs_digits)), *acc = static_cast<W *>(part_of(Z.acc));
    int32_t *ks_digits = static_cast<int32_t *>(part_of(Z.ks_digits));
    W *part = static_cast<W *>(part_of(Z.part)), *sel = F::CBS_SEL ? static_cast<W *>(part_of(Z.sel)) : static_cast<W *>(out[0]);

    const typename F::CbsConst C = F::cbs_const(pl, k, cbs_base_log, cbs_levels);
    const unsigned grid = log_lut ? ew_grid((modswitch_tiles<F>(lwe_dim, batch) + (Z.table / 16 + 255) / 256) * 256)
                                  : ew_grid((lwe_dim + 1) * e + Z.table / 16);
    hipError_t err = F::launch_cbs_setup(pl, rot_t, table, lwe_in, C, log_lut, lwe_dim, rotations, grid, st);
    if (err != hipSuccess)
        return fail(CNTT_EDEVICE, "%s_%s_kernel launch failed: %s", F::NAME, log_lut ? "modswitch_manylut" : "cbs_setup", hipGetErrorString(err));
    if (int rc = blind_rotate_device<F>(pl, acc, table, !log_lut, rot_t, bsk, lwe_dim, k, pbs_base_log, pbs_levels, rotations, pbs_digits, st))
        return rc;
    err = F::launch_cbs_extract(pl, ks_digits, acc, ks_base_log, ks_levels, C, log_lut != nullptr, rotations, ew_grid(rotations * (k * n + 1)), st);
    if (err != hipSuccess)
        return fail(CNTT_EDEVICE, "%s_%s_kernel launch failed: %s", F::NAME, log_lut ? "cbs_manylut_extract" : "cbs_extract", hipGetErrorString(err));
    err = F::launch_cbs_ks(pl, part, ks_digits, fpksk, k, r, e, Z.shape, ks_base_log, st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "%s_cbs_ks_kernel launch failed: %s", F::NAME, hipGetErrorString(err));
    err = F::launch_cbs_sum(pl, sel, part, k, cbs_levels, e, Z.shape.slabs, ew_grid((k + 1) * e * (k + 1) * n * F::word(pl) / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "%s_cbs_sum_kernel launch failed: %s", F::NAME, hipGetErrorString(err));
    return F::cbs_finish(pl, out, sel, e * (k + 1) * (k + 1), st);
}

// The family's refusals keep the places they have in each header's list: F::cbs_plan_check first, F::cbs_budget_check after the three
// gadgets, F::extract_many_check after the one-rotation form's own, F::check_terms after the bound on glwe_dim.
template <class F>
int circuit_bootstrap(const typename F::Plan *pl, typename F::CbsOut ggsw_ntt_out, const typename F::Word *lwe_in, typename F::Key bsk_ntt,
                      const typename F::Word *fpksk, size_t lwe_dim, size_t k, unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log,
                      unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, const unsigned *log_lut, size_t batch, void *workspace,
                      size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = F::cbs_plan_check(pl)) return rc;
    if (int rc = digits_check<F>(pl, "pbs_", pbs_base_log, pbs_levels)) return rc;
    if (int rc = digits_check<F>(pl, "ks_", ks_base_log, ks_levels)) return rc;
    if (ks_base_log > 31) return fail(CNTT_EINVAL, "ks_base_log = %u is above 31: a signed digit must fit an int32", ks_base_log);
    if (int rc = digits_check<F>(pl, "cbs_", cbs_base_log, cbs_levels)) return rc;
    if (int rc = F::cbs_budget_check(pl, cbs_base_log, cbs_levels)) return rc;
    if (log_lut) {
        if (int rc = manylut_check_log<F>(pl, *log_lut)) return rc;
        if (*log_lut + 1 > (unsigned)F::logn(pl))
            return fail(CNTT_EINVAL, "2^log_lut_count = 2^%u exceeds ntt_size / 2 = %zu: the bit values n / 2 and 3 n / 2 leave the coarse grid",
                        *log_lut, pl->n / 2);
        if (cbs_levels > (1u << *log_lut))
            return fail(CNTT_EINVAL, "cbs_levels = %u exceeds 2^log_lut_count = %u", cbs_levels, 1u << *log_lut);
        if (int rc = F::extract_many_check(pl)) return rc;
    } else if (F::logn(pl) > F::MODSWITCH_MAX_LOGN) {
        return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    }
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = F::check_terms(pl, k, pbs_levels)) return rc;
    const size_t n = pl->n, w = F::word(pl), kw = F::key_word(pl), lv = cbs_levels, per_bit = log_lut ? 1 : lv;   // rotations per input bit
    if (((u128)k * n + 1) * ks_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "(glwe_dim * n + 1) * ks_levels = (%zu * %zu + 1) * %u is not below 2^32 key rows", k, n, ks_levels);
    const size_t r = (k * n + 1) * ks_levels;
    // what the widest launches hold: the external product of the rotation over all its elements and, where the family transforms the
    // selectors (F::CBS_SEL), their polynomials
    if ((u128)batch * per_bit * (k + 1) * pbs_levels >= ((u128)1 << 32) || (F::CBS_SEL && (u128)batch * lv * (k + 1) * (k + 1) * n >= ((u128)1 << 46))) {
        const char *also = F::CBS_SEL ? ", or the selectors' words are not below 2^46" : "";
        if (log_lut)
            return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * pbs_levels = %zu * %zu * %u is not below 2^32%s: too large for one launch", batch,
                        k + 1, pbs_levels, also);
        return fail(CNTT_EINVAL, "batch * cbs_levels * (glwe_dim + 1) * pbs_levels = %zu * %u * %zu * %u is not below 2^32%s: too large for one launch",
                    batch, cbs_levels, k + 1, pbs_levels, also);
    }
    // the byte counts are products of the arguments: they must fit before they are formed (2048 = the most slabs the shape rule gives).
    // One list for both forms and both families: it is the union of theirs, and every entry one of them lacked is implied there by one it
    // had with the same zero factors ({batch, lv}: e < 2^32 after the launch check; {lwe_dim + 1, batch, 1, 4}: by {batch, lwe_dim + 1, w},
    // w >= 4; the last one where kw == w: by the 2048-slab entry), so no entry is a new refusal -- and none may be dropped as redundant.
    if (product_passes_2_63({batch, lv}) || product_passes_2_63({batch, lwe_dim + 1, w}) || lwe_dim + 1 == 0 ||
        product_passes_2_63({lwe_dim + 1, batch, per_bit, (size_t)4}) || product_passes_2_63({lwe_dim, k + 1, (size_t)pbs_levels, k + 1, n, kw}) ||
        product_passes_2_63({k + 1, r, k + 1, n, w}) || product_passes_2_63({batch, per_bit, k + 1, (size_t)pbs_levels, n, w}) ||
        product_passes_2_63({batch, lv, r, (size_t)4}) || product_passes_2_63({(size_t)2048, k + 1, batch, lv, k + 1, n, w}) ||
        product_passes_2_63({k + 1, batch, lv, k + 1, n, kw}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the keys, the selectors or the workspace pass 2^63 bytes",
                    lwe_dim, k, batch);
    if (batch == 0) return CNTT_OK;
    if (!ggsw_ntt_out) return fail(CNTT_EINVAL, "ggsw_ntt_out is NULL");
    void *out[10], *dout[10];
    const char *out_name[10];
    const int np = F::cbs_out_planes(pl, ggsw_ntt_out, out, out_name);
    for (int i = 0; i < np; ++i)
        if (!out[i]) return fail(CNTT_EINVAL, "NULL output residue plane (%s)", out_name[i]);
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim)
        if (int rc = F::key_check(pl, bsk_ntt, "bsk_ntt")) return rc;
    const size_t e = batch * cbs_levels, fb = (k + 1) * r * (k + 1) * n * w;
    const Operand fk = F::fpksk_operand(pl, fpksk, fb);
    if (!fpksk) return fail(CNTT_EINVAL, "%s is NULL", fk.name);
    const CbsSizes<F> Z = cbs_sizes<F>(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch, log_lut != nullptr);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const size_t ob = e * (k + 1) * (k + 1) * n * kw, ib = batch * (lwe_dim + 1) * w, bb = F::key_bytes(pl, lwe_dim * (k + 1) * pbs_levels * (k + 1));
    Operand ops[CBS_MAX_OPERANDS];
    int cnt = 0;
    for (int i = 0; i < np; ++i) ops[cnt++] = {out_name[i], out[i], ob, kw, true};
    ops[cnt++] = {"lwe_in", lwe_in, ib, w, false};
    if (int rc = key_and_workspace_operands<F>(pl, ops, cnt, bsk_ntt, bb, &fk, workspace, workspace_bytes)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *din = (const W *)s.in(lwe_in, ib);
    const typename F::Key dbsk = lwe_dim ? F::key_in(pl, s, bsk_ntt, bb, ks) : typename F::Key{};
    const W *dfk = (const W *)s.in(fpksk, fb);
    for (int i = 0; i < np; ++i) dout[i] = s.out(out[i], ob);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = circuit_bootstrap_device<F>(pl, dout, din, dbsk, dfk, lwe_dim, k, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log,
                                             cbs_levels, log_lut, batch, Z, dws, st))
        return rc;
    return s.finish();
}

#pragma GCC visibility pop
