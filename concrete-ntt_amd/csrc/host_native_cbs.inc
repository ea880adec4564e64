// Part of host_native_ext.hip (included at its end, after host_native_cmux.inc): the circuit bootstrap from LWE bits to GGSW selectors
// (include/cntt_cbs.h) -- the argument checks, the workspace layout, the host-slice path and the C ABI over the kernels of native_cbs.hpp
// (launched by native_cbs.hip), blind_rotate_device<NativePbs>, native_split_device and native_ntt_device, which it calls and does not
// change.
#include "../../include/cntt_cbs.h"
#include "native_cbs.hpp"

#pragma GCC visibility push(hidden)

// the seven parts of the workspace, in bytes and in this order (cntt_cbs.h states the formula)
struct NativeCbsSizes {
    size_t rot, table, pbs_digits, acc, ks_digits, part, sel;
    NativeCbsShape shape;
    size_t total() const {
        return up256(rot) + up256(table) + up256(pbs_digits) + up256(acc) + up256(ks_digits) + up256(part) + up256(sel);
    }
};
static NativeCbsSizes native_cbs_sizes(const cntt_native *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels,
                                       unsigned cbs_levels, size_t batch) {
    const size_t w = (size_t)pl->info.word, e = batch * cbs_levels, r = (k * pl->n + 1) * ks_levels, ct = (k + 1) * pl->n * w;
    NativeCbsSizes Z;
    Z.shape = native_cbs_shape(pl->n, w, k, r, e);
    Z.rot = (lwe_dim + 1) * e * sizeof(uint32_t);
    Z.table = e * ct;
    Z.pbs_digits = e * ct * pbs_levels;
    Z.acc = e * ct;
    Z.ks_digits = e * r * sizeof(int32_t);
    Z.part = Z.shape.slabs * (k + 1) * e * ct;
    Z.sel = (k + 1) * e * ct;
    return Z;
}

// one of the three gadgets: `name` is the prefix of its two arguments; budget: the bits base_log * levels may fill
static int native_cbs_check_gadget(const char *name, unsigned base_log, unsigned levels, unsigned wbits) {
    if (base_log == 0) return fail(CNTT_EINVAL, "%sbase_log is 0", name);
    if (levels == 0) return fail(CNTT_EINVAL, "%slevels is 0", name);
    if ((uint64_t)base_log * levels > wbits) return fail(CNTT_EINVAL, NativePbs::DIGIT_BUDGET_MSG, name, name, base_log, levels, wbits);
    return CNTT_OK;
}

// set-up -> one blind rotation over the E = batch * cbs_levels elements -> extraction and signed digits -> the digit x key product in
// slabs -> the sum of the slabs, negated, in the selector layout -> the split into residues and the forward transforms, the two steps of
// cntt_native_fwd_batch, into the caller's planes.  ws holds rot | table | digits of the rotation | acc | int32 digits | slab partials |
// selector words (NativeCbsSizes).
static int native_cbs_device(const cntt_native *pl, void *const *out, const void *lwe_in, NativePbs::Key bsk, const void *fpksk, size_t lwe_dim,
                             size_t k, unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                             unsigned cbs_base_log, unsigned cbs_levels, size_t batch, const NativeCbsSizes &Z, char *ws, hipStream_t st) {
    const size_t e = batch * cbs_levels, n = pl->n, r = (k * n + 1) * ks_levels, polys = e * (k + 1) * (k + 1);
    const int word = pl->info.word, logn = native_logn(pl);
    char *at = ws;
    const auto part_of = [&at](size_t bytes) {
        char *here = at;
        at += up256(bytes);
        return static_cast<void *>(here);
    };
    uint32_t *rot_t = static_cast<uint32_t *>(part_of(Z.rot));
    void *table = part_of(Z.table), *pbs_digits = part_of(Z.pbs_digits), *acc = part_of(Z.acc);
    int32_t *ks_digits = static_cast<int32_t *>(part_of(Z.ks_digits));
    void *part = part_of(Z.part), *sel = part_of(Z.sel);

    const NativeCbsConst C{(uint32_t)logn, (uint32_t)k, cbs_base_log, cbs_levels};
    hipError_t err = launch_native_cbs_setup(word, rot_t, table, lwe_in, C, lwe_dim, e, ew_grid((lwe_dim + 1) * e + Z.table / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_setup_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = blind_rotate_device<NativePbs>(pl, acc, table, true, rot_t, bsk, lwe_dim, k, pbs_base_log, pbs_levels, e, pbs_digits, st)) return rc;
    const u128 off = gadget_offset(NativePbs::digit_bits(pl), ks_base_log, ks_levels);
    err = launch_native_cbs_extract(word, ks_digits, acc, (uint64_t)off, (uint64_t)(off >> 64), ks_base_log, ks_levels, C, e,
                                    ew_grid(e * (k * n + 1)), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_extract_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_native_cbs_ks(word, part, ks_digits, fpksk, logn, k, r, e, Z.shape, st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_ks_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_native_cbs_sum(word, sel, part, logn, k, cbs_levels, e, Z.shape.slabs, ew_grid(Z.sel / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_sum_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = native_split_device(pl, sel, out, polys * n, false, st)) return rc;
    return native_ntt_device(pl, out, polys, false, st);
}

static const char *const CBS_OUT[10] = {"ggsw_ntt_out[0]", "ggsw_ntt_out[1]", "ggsw_ntt_out[2]", "ggsw_ntt_out[3]", "ggsw_ntt_out[4]",
                                        "ggsw_ntt_out[5]", "ggsw_ntt_out[6]", "ggsw_ntt_out[7]", "ggsw_ntt_out[8]", "ggsw_ntt_out[9]"};
static const char *const CBS_BSK[10] = {"bsk_ntt[0]", "bsk_ntt[1]", "bsk_ntt[2]", "bsk_ntt[3]", "bsk_ntt[4]",
                                        "bsk_ntt[5]", "bsk_ntt[6]", "bsk_ntt[7]", "bsk_ntt[8]", "bsk_ntt[9]"};

static int native_circuit_bootstrap(const cntt_native *pl, void *const *ggsw_ntt_out, const void *lwe_in, NativePbs::Key bsk_ntt, const void *fpksk,
                                    size_t lwe_dim, size_t k, unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                    unsigned cbs_base_log, unsigned cbs_levels, size_t batch, void *workspace, size_t workspace_bytes,
                                    cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (pl->info.binary)
        return fail(CNTT_EINVAL, "plan is of a native_binary kind: a produced selector has full-width words, and the exactness of these kinds rests on "
                                 "0/1 key words");
    const unsigned wbits = NativePbs::digit_bits(pl);
    if (int rc = native_cbs_check_gadget("pbs_", pbs_base_log, pbs_levels, wbits)) return rc;
    if (int rc = native_cbs_check_gadget("ks_", ks_base_log, ks_levels, wbits)) return rc;
    if (ks_base_log > 31) return fail(CNTT_EINVAL, "ks_base_log = %u is above 31: a signed digit must fit an int32", ks_base_log);
    if (int rc = native_cbs_check_gadget("cbs_", cbs_base_log, cbs_levels, wbits)) return rc;
    if ((uint64_t)cbs_base_log * cbs_levels > wbits - 1)
        return fail(CNTT_EINVAL, "cbs_base_log * cbs_levels = %u * %u exceeds w - 1 = %u: H = 2^(w - cbs_base_log * cbs_levels) / 2 must be a word, "
                                 "and 2 has no inverse mod 2^w", cbs_base_log, cbs_levels, wbits - 1);
    if (native_logn(pl) > NativePbs::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = NativePbs::check_terms(pl, k, pbs_levels)) return rc;
    const size_t n = pl->n, w = (size_t)pl->info.word, rb = pl->rbytes();
    if (((u128)k * n + 1) * ks_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "(glwe_dim * n + 1) * ks_levels = (%zu * %zu + 1) * %u is not below 2^32 key rows", k, n, ks_levels);
    const size_t r = (k * n + 1) * ks_levels;
    // what the widest launches hold: the external product of the rotation over all E = batch * cbs_levels elements, and the transforms of
    // the selectors' polynomials
    if ((u128)batch * cbs_levels * (k + 1) * pbs_levels >= ((u128)1 << 32) || (u128)batch * cbs_levels * (k + 1) * (k + 1) * n >= ((u128)1 << 46))
        return fail(CNTT_EINVAL, "batch * cbs_levels * (glwe_dim + 1) * pbs_levels = %zu * %u * %zu * %u is not below 2^32, or the selectors' words "
                                 "are not below 2^46: too large for one launch", batch, cbs_levels, k + 1, pbs_levels);
    const size_t e = batch * cbs_levels;
    // the byte counts are products of the arguments: they must fit before they are formed (2048 = the most slabs the shape rule gives)
    if (cmux_passes_2_63({batch, lwe_dim + 1, w}) || lwe_dim + 1 == 0 || cmux_passes_2_63({lwe_dim + 1, e, (size_t)4}) ||
        cmux_passes_2_63({lwe_dim, k + 1, (size_t)pbs_levels, k + 1, n, rb}) || cmux_passes_2_63({k + 1, r, k + 1, n, w}) ||
        cmux_passes_2_63({e, k + 1, (size_t)pbs_levels, n, w}) || cmux_passes_2_63({e, r, (size_t)4}) ||
        cmux_passes_2_63({(size_t)2048, k + 1, e, k + 1, n, w}) || cmux_passes_2_63({k + 1, e, k + 1, n, rb}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the keys, the selectors or the workspace pass 2^63 bytes",
                    lwe_dim, k, batch);
    if (batch == 0) return CNTT_OK;
    const int np = pl->info.nprimes;
    if (!ggsw_ntt_out) return fail(CNTT_EINVAL, "ggsw_ntt_out is NULL");
    for (int i = 0; i < np; ++i)
        if (!ggsw_ntt_out[i]) return fail(CNTT_EINVAL, "NULL output residue plane (%s)", CBS_OUT[i]);
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim)
        if (int rc = NativePbs::key_check(pl, bsk_ntt, "bsk_ntt")) return rc;
    if (!fpksk) return fail(CNTT_EINVAL, "fpksk is NULL");
    const NativeCbsSizes Z = native_cbs_sizes(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const size_t ob = e * (k + 1) * (k + 1) * n * rb, ib = batch * (lwe_dim + 1) * w, bb = NativePbs::key_bytes(pl, lwe_dim * (k + 1) * pbs_levels * (k + 1)),
                 fb = (k + 1) * r * (k + 1) * n * w;
    Operand ops[23];
    int cnt = 0;
    for (int i = 0; i < np; ++i) ops[cnt++] = {CBS_OUT[i], ggsw_ntt_out[i], ob, rb, true};
    ops[cnt++] = {"lwe_in", lwe_in, ib, w, false};
    for (int i = 0; i < np && bb; ++i) ops[cnt++] = {CBS_BSK[i], bsk_ntt[i], bb, rb, false};
    ops[cnt++] = {"fpksk", fpksk, fb, 16, false};   // read in 16-byte vectors
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    NativePbs::KeyStore ks;
    const void *din = s.in(lwe_in, ib);
    const NativePbs::Key dbsk = lwe_dim ? NativePbs::key_in(pl, s, bsk_ntt, bb, ks) : NativePbs::Key{};
    const void *dfk = s.in(fpksk, fb);
    void *dout[10];
    for (int i = 0; i < np; ++i) dout[i] = s.out(ggsw_ntt_out[i], ob);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = native_cbs_device(pl, dout, din, dbsk, dfk, lwe_dim, k, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels,
                                   batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_circuit_bootstrap_batch(const cntt_native_t *pl, void *const *ggsw_ntt_out, const void *lwe_in,
                                                   const void *const *bsk_ntt, const void *fpksk, size_t lwe_dim, size_t glwe_dim,
                                                   unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                   unsigned cbs_base_log, unsigned cbs_levels, size_t batch, void *workspace,
                                                   size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return native_circuit_bootstrap(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels,
                                    cbs_base_log, cbs_levels, batch, workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_circuit_bootstrap_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                                unsigned ks_levels, unsigned cbs_levels, size_t batch) {
    return pl ? native_cbs_sizes(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch).total() : 0;
}
extern "C" unsigned cntt_native_cbs_grid(size_t items, int logn, size_t word_bytes) { return native_cbs_grid(items, logn, word_bytes); }
