// Part of host_native_ext.hip (included at its end, after host_native_cbs.inc): the many-LUT bootstrap and the circuit bootstrap with one
// rotation per input bit (include/cntt_manylut.h) -- the argument checks, the workspace layouts, the host-slice path and the C ABI over
// the kernels of native_manylut.hpp (launched by native_manylut.hip), blind_rotate_device<NativePbs>, the functional keyswitch of
// native_cbs.hpp, native_split_device and native_ntt_device, which it calls and does not change.
#include "../../include/cntt_manylut.h"
#include "native_manylut.hpp"

#pragma GCC visibility push(hidden)

static int native_manylut_check_log(const cntt_native *pl, unsigned log_lut) {
    if (log_lut > (unsigned)native_logn(pl))
        return fail(CNTT_EINVAL, "log_lut_count = %u exceeds log2(ntt_size) = %d", log_lut, native_logn(pl));
    if (native_logn(pl) > NativePbs::MODSWITCH_MAX_LOGN) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");
    return CNTT_OK;
}
// the extraction owns 16 bytes of a row per thread
static int native_manylut_check_vector(const cntt_native *pl) {
    if (pl->n * (size_t)pl->info.word < 16)
        return fail(CNTT_EINVAL, "ntt_size = %zu words of %d bytes are below the 16 bytes one thread of the extraction owns", pl->n, pl->info.word);
    return CNTT_OK;
}

static int native_modswitch_manylut_device(const cntt_native *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim, unsigned log_lut, size_t batch,
                                           hipStream_t st) {
    const size_t tiles = ((lwe_dim + PBS_TILE) / PBS_TILE) * ((batch + PBS_TILE - 1) / PBS_TILE);
    const hipError_t e = launch_native_modswitch_manylut(pl->info.word, rot_t, lwe, native_logn(pl), log_lut, lwe_dim, batch, ew_grid(tiles * 256), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_modswitch_manylut_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

static int native_extract_many_device(const cntt_native *pl, void *lwe_out, const void *glwe, size_t k, size_t count, size_t batch, hipStream_t st) {
    const size_t n = pl->n, w = (size_t)pl->info.word, chunks = (count + NEXM_ROWS - 1) / NEXM_ROWS;
    const size_t items = batch * k * chunks * (n * w / 16) + batch * count;
    // the output against STREAM_BYTES, as the other element-wise kernels decide it
    const hipError_t e = launch_native_sample_extract_many(pl->info.word, lwe_out, glwe, native_logn(pl), k, count, batch,
                                                           batch * count * (k * n + 1) * w > STREAM_BYTES, ew_grid(items), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_sample_extract_many_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

static int native_lwe_modswitch_manylut(const cntt_native *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim, unsigned log_lut, size_t batch,
                                        cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = native_manylut_check_log(pl, log_lut)) return rc;
    const size_t w = (size_t)pl->info.word;
    if (cmux_passes_2_63({batch, lwe_dim + 1, w}) || lwe_dim + 1 == 0)
        return fail(CNTT_EINVAL, "lwe_dim = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", lwe_dim, batch);
    if (batch == 0) return CNTT_OK;
    if (!rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (!lwe) return fail(CNTT_EINVAL, "lwe is NULL");
    const size_t rb = (lwe_dim + 1) * batch * sizeof(uint32_t), lb = (lwe_dim + 1) * batch * w;
    const Operand ops[2] = {{"rot_t", rot_t, rb, sizeof(uint32_t), true}, {"lwe", lwe, lb, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    uint32_t *dr = (uint32_t *)s.out(rot_t, rb);
    const void *dl = s.in(lwe, lb);
    if (int rc = s.status()) return rc;
    if (int rc = native_modswitch_manylut_device(pl, dr, dl, lwe_dim, log_lut, batch, st)) return rc;
    return s.finish();
}

static int native_sample_extract_many(const cntt_native *pl, void *lwe_out, const void *glwe, size_t k, size_t count, size_t batch,
                                      cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (count == 0 || count > pl->n) return fail(CNTT_EINVAL, "count = %zu is not in 1 .. ntt_size = %zu", count, pl->n);
    if (int rc = native_manylut_check_vector(pl)) return rc;
    const size_t w = (size_t)pl->info.word;
    if (k + 1 == 0 || cmux_passes_2_63({batch, count, k, pl->n, w}) || cmux_passes_2_63({batch, count + k + 1, pl->n, w}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, count = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", k, count, batch);
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!glwe) return fail(CNTT_EINVAL, "glwe is NULL");
    const size_t ob = batch * count * (k * pl->n + 1) * w, gb = batch * (k + 1) * pl->n * w;
    const Operand ops[2] = {{"lwe_out", lwe_out, ob, w, true}, {"glwe", glwe, gb, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    void *dout = s.out(lwe_out, ob);
    const void *dg = s.in(glwe, gb);
    if (int rc = s.status()) return rc;
    if (int rc = native_extract_many_device(pl, dout, dg, k, count, batch, st)) return rc;
    return s.finish();
}

static const char *const MANYLUT_OUT[10] = {"ggsw_ntt_out[0]", "ggsw_ntt_out[1]", "ggsw_ntt_out[2]", "ggsw_ntt_out[3]", "ggsw_ntt_out[4]",
                                            "ggsw_ntt_out[5]", "ggsw_ntt_out[6]", "ggsw_ntt_out[7]", "ggsw_ntt_out[8]", "ggsw_ntt_out[9]"};
static const char *const MANYLUT_BSK[10] = {"bsk_ntt[0]", "bsk_ntt[1]", "bsk_ntt[2]", "bsk_ntt[3]", "bsk_ntt[4]",
                                            "bsk_ntt[5]", "bsk_ntt[6]", "bsk_ntt[7]", "bsk_ntt[8]", "bsk_ntt[9]"};

// the coarse modulus switch -> the blind rotation -> the extraction of the indices 0 .. lut_count - 1; ws holds digits | rot_t | acc
// (PbsSizes), as bootstrap_device
static int native_bootstrap_manylut(const cntt_native *pl, void *lwe_out, const void *lwe_in, const void *lut, int lut_per_element,
                                    NativePbs::Key bsk, size_t lwe_dim, size_t k, unsigned base_log, unsigned levels, unsigned log_lut,
                                    size_t lut_count, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using F = NativePbs;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = native_manylut_check_log(pl, log_lut)) return rc;
    if (lut_count == 0 || lut_count > ((size_t)1 << log_lut))
        return fail(CNTT_EINVAL, "lut_count = %zu is not in 1 .. 2^log_lut_count = %zu", lut_count, (size_t)1 << log_lut);
    if (int rc = native_manylut_check_vector(pl)) return rc;
    const size_t n = pl->n, w = (size_t)pl->info.word, rb = pl->rbytes(), lv = levels ? levels : 1;
    if (k + 1 == 0 || lwe_dim + 1 == 0 || cmux_passes_2_63({batch, lwe_dim + 1, w}) || cmux_passes_2_63({batch, k + 1, lv, n, w}) ||
        cmux_passes_2_63({batch, lut_count, k + 1, n, w}) || cmux_passes_2_63({lwe_dim, k + 1, lv, k + 1, n, rb}))
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
    const int np = pl->info.nprimes;
    Operand ops[14];
    int cnt = 0;
    ops[cnt++] = {"lwe_out", lwe_out, ob, w, true};
    ops[cnt++] = {"lwe_in", lwe_in, ib, w, false};
    ops[cnt++] = {"lut", lut, lb, w, false};
    for (int i = 0; i < np && kb; ++i) ops[cnt++] = {MANYLUT_BSK[i], bsk[i], kb, rb, false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    F::KeyStore ks;
    const F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, kb, ks) : F::Key{};
    const void *din = s.in(lwe_in, ib), *dlut = s.in(lut, lb);
    void *dout = s.out(lwe_out, ob);
    char *ws = (char *)s.workspace(workspace, Z.total());   // one block for the whole call
    if (int rc = s.status()) return rc;
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    void *acc = ws + up256(Z.digits) + up256(Z.rot);
    if (int rc = native_modswitch_manylut_device(pl, rot_t, din, lwe_dim, log_lut, batch, st)) return rc;
    if (int rc = blind_rotate_device<F>(pl, acc, dlut, lut_per_element != 0, rot_t, dkey, lwe_dim, k, base_log, levels, batch, ws, st)) return rc;
    if (int rc = native_extract_many_device(pl, dout, acc, k, lut_count, batch, st)) return rc;
    return s.finish();
}

// the seven parts of the workspace of the one-rotation circuit bootstrap, in bytes and in this order (cntt_manylut.h states the formula):
// the rotation's parts are per input bit, the keyswitch's per bit and level, with the slab rule of native_cbs_shape unchanged
static NativeCbsSizes native_cbs_manylut_sizes(const cntt_native *pl, size_t lwe_dim, size_t k, unsigned pbs_levels, unsigned ks_levels,
                                               unsigned cbs_levels, size_t batch) {
    const size_t w = (size_t)pl->info.word, e = batch * cbs_levels, r = (k * pl->n + 1) * ks_levels, ct = (k + 1) * pl->n * w;
    NativeCbsSizes Z;
    Z.shape = native_cbs_shape(pl->n, w, k, r, e);
    Z.rot = (lwe_dim + 1) * batch * sizeof(uint32_t);
    Z.table = ct;
    Z.pbs_digits = batch * ct * pbs_levels;
    Z.acc = batch * ct;
    Z.ks_digits = e * r * sizeof(int32_t);
    Z.part = Z.shape.slabs * (k + 1) * e * ct;
    Z.sel = (k + 1) * e * ct;
    return Z;
}

// set-up (the coarse switch of lwe + 2^(w - 2), the shared table) -> one blind rotation over the batch -> extraction at the indices l - 1
// and signed digits -> the digit x key product in slabs -> the sum of the slabs, negated, in the selector layout -> the split into
// residues and the forward transforms into the caller's planes
static int native_cbs_manylut_device(const cntt_native *pl, void *const *out, const void *lwe_in, NativePbs::Key bsk, const void *fpksk,
                                     size_t lwe_dim, size_t k, unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log,
                                     unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut, size_t batch,
                                     const NativeCbsSizes &Z, char *ws, hipStream_t st) {
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
    const size_t tiles = ((lwe_dim + PBS_TILE) / PBS_TILE) * ((batch + PBS_TILE - 1) / PBS_TILE);
    hipError_t err = launch_native_cbs_manylut_setup(word, rot_t, table, lwe_in, C, log_lut, lwe_dim, batch,
                                                     ew_grid((tiles + (Z.table / 16 + 255) / 256) * 256), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_modswitch_manylut_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = blind_rotate_device<NativePbs>(pl, acc, table, false, rot_t, bsk, lwe_dim, k, pbs_base_log, pbs_levels, batch, pbs_digits, st))
        return rc;
    const u128 off = gadget_offset(NativePbs::digit_bits(pl), ks_base_log, ks_levels);
    err = launch_native_cbs_manylut_extract(word, ks_digits, acc, (uint64_t)off, (uint64_t)(off >> 64), ks_base_log, ks_levels, C, batch,
                                            ew_grid(batch * (k * n + 1)), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_manylut_extract_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_native_cbs_ks(word, part, ks_digits, fpksk, logn, k, r, e, Z.shape, st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_ks_kernel launch failed: %s", hipGetErrorString(err));
    err = launch_native_cbs_sum(word, sel, part, logn, k, cbs_levels, e, Z.shape.slabs, ew_grid(Z.sel / 16), st);
    if (err != hipSuccess) return fail(CNTT_EDEVICE, "native_cbs_sum_kernel launch failed: %s", hipGetErrorString(err));
    if (int rc = native_split_device(pl, sel, out, polys * n, false, st)) return rc;
    return native_ntt_device(pl, out, polys, false, st);
}

static int native_circuit_bootstrap_manylut(const cntt_native *pl, void *const *ggsw_ntt_out, const void *lwe_in, NativePbs::Key bsk_ntt,
                                            const void *fpksk, size_t lwe_dim, size_t k, unsigned pbs_base_log, unsigned pbs_levels,
                                            unsigned ks_base_log, unsigned ks_levels, unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut,
                                            size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
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
    if (int rc = native_manylut_check_log(pl, log_lut)) return rc;
    if (log_lut + 1 > (unsigned)native_logn(pl))
        return fail(CNTT_EINVAL, "2^log_lut_count = 2^%u exceeds ntt_size / 2 = %zu: the bit values n / 2 and 3 n / 2 leave the coarse grid", log_lut,
                    pl->n / 2);
    if (cbs_levels > (1u << log_lut))
        return fail(CNTT_EINVAL, "cbs_levels = %u exceeds 2^log_lut_count = %u", cbs_levels, 1u << log_lut);
    if (int rc = native_manylut_check_vector(pl)) return rc;
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = NativePbs::check_terms(pl, k, pbs_levels)) return rc;
    const size_t n = pl->n, w = (size_t)pl->info.word, rb = pl->rbytes();
    if (((u128)k * n + 1) * ks_levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "(glwe_dim * n + 1) * ks_levels = (%zu * %zu + 1) * %u is not below 2^32 key rows", k, n, ks_levels);
    const size_t r = (k * n + 1) * ks_levels;
    // what the widest launches hold: the external product of the rotation over the batch, and the transforms of the selectors' polynomials
    if ((u128)batch * (k + 1) * pbs_levels >= ((u128)1 << 32) || (u128)batch * cbs_levels * (k + 1) * (k + 1) * n >= ((u128)1 << 46))
        return fail(CNTT_EINVAL, "batch * (glwe_dim + 1) * pbs_levels = %zu * %zu * %u is not below 2^32, or the selectors' words are not below "
                                 "2^46: too large for one launch", batch, k + 1, pbs_levels);
    // the byte counts are products of the arguments: they must fit before they are formed (2048 = the most slabs the shape rule gives)
    if (cmux_passes_2_63({batch, (size_t)cbs_levels}) || cmux_passes_2_63({batch, lwe_dim + 1, w}) || lwe_dim + 1 == 0 ||
        cmux_passes_2_63({lwe_dim, k + 1, (size_t)pbs_levels, k + 1, n, rb}) || cmux_passes_2_63({k + 1, r, k + 1, n, w}) ||
        cmux_passes_2_63({batch, k + 1, (size_t)pbs_levels, n, w}) || cmux_passes_2_63({batch, (size_t)cbs_levels, r, (size_t)4}) ||
        cmux_passes_2_63({(size_t)2048, k + 1, batch, (size_t)cbs_levels, k + 1, n, w}) ||
        cmux_passes_2_63({k + 1, batch, (size_t)cbs_levels, k + 1, n, rb}))
        return fail(CNTT_EINVAL, "lwe_dim = %zu, glwe_dim = %zu, batch = %zu: the ciphertexts, the keys, the selectors or the workspace pass 2^63 bytes",
                    lwe_dim, k, batch);
    if (batch == 0) return CNTT_OK;
    const int np = pl->info.nprimes;
    if (!ggsw_ntt_out) return fail(CNTT_EINVAL, "ggsw_ntt_out is NULL");
    for (int i = 0; i < np; ++i)
        if (!ggsw_ntt_out[i]) return fail(CNTT_EINVAL, "NULL output residue plane (%s)", MANYLUT_OUT[i]);
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim)
        if (int rc = NativePbs::key_check(pl, bsk_ntt, "bsk_ntt")) return rc;
    if (!fpksk) return fail(CNTT_EINVAL, "fpksk is NULL");
    const size_t e = batch * cbs_levels;
    const NativeCbsSizes Z = native_cbs_manylut_sizes(pl, lwe_dim, k, pbs_levels, ks_levels, cbs_levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const size_t ob = e * (k + 1) * (k + 1) * n * rb, ib = batch * (lwe_dim + 1) * w,
                 bb = NativePbs::key_bytes(pl, lwe_dim * (k + 1) * pbs_levels * (k + 1)), fb = (k + 1) * r * (k + 1) * n * w;
    Operand ops[23];
    int cnt = 0;
    for (int i = 0; i < np; ++i) ops[cnt++] = {MANYLUT_OUT[i], ggsw_ntt_out[i], ob, rb, true};
    ops[cnt++] = {"lwe_in", lwe_in, ib, w, false};
    for (int i = 0; i < np && bb; ++i) ops[cnt++] = {MANYLUT_BSK[i], bsk_ntt[i], bb, rb, false};
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
    if (int rc = native_cbs_manylut_device(pl, dout, din, dbsk, dfk, lwe_dim, k, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log,
                                           cbs_levels, log_lut, batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_lwe_modswitch_manylut_batch(const cntt_native_t *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim,
                                                       unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream) {
    return native_lwe_modswitch_manylut(pl, rot_t, lwe, lwe_dim, log_lut_count, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_sample_extract_many_batch(const cntt_native_t *pl, void *lwe_out, const void *glwe, size_t glwe_dim, size_t count,
                                                     size_t batch, cntt_mem_t where, void *stream) {
    return native_sample_extract_many(pl, lwe_out, glwe, glwe_dim, count, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_bootstrap_manylut_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *lut,
                                                   int lut_per_element, const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                                   unsigned base_log, unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch,
                                                   void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return native_bootstrap_manylut(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, log_lut_count,
                                    lut_count, batch, workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" int cntt_native_circuit_bootstrap_manylut_batch(const cntt_native_t *pl, void *const *ggsw_ntt_out, const void *lwe_in,
                                                           const void *const *bsk_ntt, const void *fpksk, size_t lwe_dim, size_t glwe_dim,
                                                           unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                           unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut_count, size_t batch,
                                                           void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return native_circuit_bootstrap_manylut(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                            ks_levels, cbs_base_log, cbs_levels, log_lut_count, batch, workspace, workspace_bytes, where,
                                            (hipStream_t)stream);
}
extern "C" size_t cntt_native_circuit_bootstrap_manylut_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim,
                                                                        unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                                                                        size_t batch) {
    return pl ? native_cbs_manylut_sizes(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch).total() : 0;
}
