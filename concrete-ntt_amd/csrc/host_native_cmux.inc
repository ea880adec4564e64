// Part of host_native_ext.hip (included at its end, after host_native_multibit.inc): the CMux and the CMux tree against GGSW selectors
// (include/cntt_cmux.h) -- the argument checks, the workspace layout, the host-slice path and the C ABI over the kernel of
// native_cmux.hpp (launched by native_cmux.hip), gadget_check and the family's external product (native_ext_device), which it calls and
// does not change.  Written as templates over a plan family F in the style of pbs_host.hpp: F is NativePbs plus the one launcher below,
// so that the prime path (host_prime_cmux.inc, as it is) can be folded in later.
#include "../../include/cntt_cmux.h"
#include "native_cmux.hpp"

#pragma GCC visibility push(hidden)

struct NativeCmux : NativePbs {
    static hipError_t launch_cmux_diff(const cntt_native *pl, void *terms, void *out, const void *c0, const void *c1, bool leaf,
                                       unsigned base_log, unsigned levels, size_t glwe_dim, size_t h, size_t gs, size_t nct, bool stream,
                                       hipStream_t st) {
        const u128 off = gadget_offset(digit_bits(pl), base_log, levels);
        return launch_native_cmux_diff(pl->info.word, terms, out, c0, c1, leaf, (uint64_t)off, (uint64_t)(off >> 64), base_log, levels,
                                       native_logn(pl), glwe_dim, h, gs, nct, stream, st);
    }
};

// a word pointer moved on by `bytes` (F::Word is void for the native plans)
template <class P> static const P *cmux_at(const P *p, size_t bytes) {
    return static_cast<const P *>(static_cast<const void *>(static_cast<const char *>(static_cast<const void *>(p)) + bytes));
}

// the three parts of the tree's workspace: the digits of the widest stage, and the two ciphertext buffers the stages alternate between
struct CmuxSizes {
    size_t digits, buf_a, buf_b;
    size_t total() const { return up256(digits) + up256(buf_a) + up256(buf_b); }
};
template <class F> static CmuxSizes cmux_tree_sizes(const typename F::Plan *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    const size_t h = m / 2, q = m / 4, pb = pl->n * F::word(pl), ct = (k + 1) * pb;
    return CmuxSizes{std::max(batch * h * levels, batch * q * (k + 1) * levels) * pb, batch * h * ct, batch * q * ct};
}
template <class F> static size_t cmux_digit_bytes(const typename F::Plan *pl, size_t terms_per, unsigned levels, size_t nct) {
    return nct * terms_per * levels * pl->n * F::word(pl);
}
template <class F> static size_t cmux_workspace_bytes(const typename F::Plan *pl, size_t k, unsigned levels, size_t batch) {
    return pl ? up256(cmux_digit_bytes<F>(pl, k + 1, levels, batch)) : 0;
}
template <class F> static size_t cmux_tree_workspace_bytes(const typename F::Plan *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    return pl ? cmux_tree_sizes<F>(pl, m, k, levels, batch).total() : 0;
}

// the checks the two calls share; the widest launch holds cts ciphertexts per batch element; sums: whether the call runs an external
// product at all (a tree of one entry does not)
template <class F>
static int cmux_check_sizes(const typename F::Plan *pl, size_t k, unsigned base_log, unsigned levels, size_t batch, size_t cts, bool sums) {
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (sums)
        if (int rc = F::check_terms(pl, k, levels)) return rc;
    if ((u128)batch * cts >= ((u128)1 << 64) || (u128)batch * cts * (k + 1) * levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * ciphertexts per element * (glwe_dim + 1) * levels = %zu * %zu * %zu * %u is not below 2^32: too large for one launch",
                    batch, cts, k + 1, levels);
    return CNTT_OK;
}

// One stage for nct output ciphertexts: one launch writes the prefilled output and the digits, the external product accumulates.  leaf:
// the sources are plain polynomials standing for trivial ciphertexts, only their bodies have digits, and these meet the selector's body
// rows only.  no selector (leaf): the trivial ciphertexts and nothing else.
template <class F>
static int cmux_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *c0, const typename F::Word *c1, bool leaf,
                       typename F::Key sel, size_t k, unsigned base_log, unsigned levels, size_t h, size_t gs, size_t nct,
                       typename F::Word *terms, hipStream_t st) {
    const bool digits = !leaf || sel;
    const bool stream = digits && cmux_digit_bytes<F>(pl, leaf ? 1 : k + 1, levels, nct) > STREAM_BYTES;
    const hipError_t e = F::launch_cmux_diff(pl, digits ? terms : nullptr, out, c0, c1, leaf, base_log, levels, k, h, gs, nct, stream, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_cmux_diff_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    if (!digits) return CNTT_OK;
    if (!leaf) return F::ext_product(pl, out, terms, sel, (k + 1) * levels, k + 1, nct, true, st);
    typename F::KeyStore body;   // the rows q = k of the selector
    return F::ext_product(pl, out, terms, F::key_at(pl, sel, F::key_bytes(pl, k * levels * (k + 1)), body), levels, k + 1, nct, true, st);
}

// the operands both calls have: the key planes and the workspace behind the `cnt` the call stated itself
static const char *const CMUX_SEL[10] = {"ggsw_ntt[0]", "ggsw_ntt[1]", "ggsw_ntt[2]", "ggsw_ntt[3]", "ggsw_ntt[4]",
                                         "ggsw_ntt[5]", "ggsw_ntt[6]", "ggsw_ntt[7]", "ggsw_ntt[8]", "ggsw_ntt[9]"};
constexpr int CMUX_MAX_OPERANDS = 14;
static int cmux_check_operands(const cntt_native *pl, Operand *ops, int cnt, const void *const *sel, size_t kb, const void *workspace,
                               size_t workspace_bytes) {
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {CMUX_SEL[i], sel[i], kb, pl->rbytes(), false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    return check_operands(ops, cnt);
}

// call 1 of the header
template <class F>
static int glwe_cmux(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *glwe0, const typename F::Word *glwe1,
                     typename F::Key ggsw_ntt, size_t k, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                     size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = cmux_check_sizes<F>(pl, k, base_log, levels, batch, 1, true)) return rc;
    const size_t n = pl->n, w = F::word(pl);
    if (product_passes_2_63({batch, k + 1, levels, n, w}) || product_passes_2_63({k + 1, levels, k + 1, n, w}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the selector pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!glwe0) return fail(CNTT_EINVAL, "glwe0 is NULL");
    if (!glwe1) return fail(CNTT_EINVAL, "glwe1 is NULL");
    if (int rc = F::key_check(pl, ggsw_ntt, "ggsw_ntt")) return rc;
    const size_t cb = batch * (k + 1) * n * w, kb = F::key_bytes(pl, (k + 1) * levels * (k + 1));
    const size_t need = cmux_workspace_bytes<F>(pl, k, levels, batch);
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    Operand ops[CMUX_MAX_OPERANDS] = {{"glwe_out", glwe_out, cb, w, true}, {"glwe0", glwe0, cb, w, false}, {"glwe1", glwe1, cb, w, false}};
    if (int rc = cmux_check_operands(pl, ops, 3, ggsw_ntt, kb, workspace, workspace_bytes)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *d0 = (const W *)s.in(glwe0, cb), *d1 = (const W *)s.in(glwe1, cb);
    const typename F::Key dsel = F::key_in(pl, s, ggsw_ntt, kb, ks);
    W *dout = (W *)s.out(glwe_out, cb);
    W *dterms = (W *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = cmux_device<F>(pl, dout, d0, d1, false, dsel, k, base_log, levels, 1, 1, batch, dterms, st)) return rc;
    return s.finish();
}

// The tree.  Stage s = 1 .. depth (h = m / 2^s) selects between entries j and j + h of the previous stage with selector depth - s;
// stage 1 reads the table polynomials as leaves.  Stage outputs alternate between buf_a (odd s) and buf_b (even s); the last stage
// writes `out`.  m == 1: the trivial ciphertext.
template <class F>
static int cmux_tree_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *lut, typename F::Key sel, size_t m, size_t k,
                            unsigned base_log, unsigned levels, size_t batch, typename F::Word *terms, typename F::Word *buf_a,
                            typename F::Word *buf_b, hipStream_t st) {
    using W = typename F::Word;
    const size_t pb = pl->n * F::word(pl), slice = F::key_bytes(pl, (k + 1) * levels * (k + 1));   // one polynomial; one selector
    unsigned depth = 0;
    while (((size_t)1 << depth) < m) ++depth;
    if (depth == 0) return cmux_device<F>(pl, out, lut, lut, true, typename F::Key{}, k, base_log, levels, 1, 1, batch, nullptr, st);
    const W *cur = lut;
    typename F::KeyStore ks;
    for (unsigned s = 1; s <= depth; ++s) {
        const size_t h = m >> s;
        W *dst = s == depth ? out : s % 2 ? buf_a : buf_b;
        const W *c1 = cmux_at(cur, h * (s == 1 ? pb : (k + 1) * pb));
        if (int rc = cmux_device<F>(pl, dst, cur, c1, s == 1, F::key_at(pl, sel, (size_t)(depth - s) * slice, ks), k, base_log, levels, h, 2 * h,
                                    batch * h, terms, st))
            return rc;
        cur = dst;
    }
    return CNTT_OK;
}

// call 2 of the header
template <class F>
static int cmux_tree(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *lut_in, typename F::Key ggsw_ntt, size_t m,
                     size_t k, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                     hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (m == 0 || (m & (m - 1))) return fail(CNTT_EINVAL, "lut_count = %zu is not a power of two >= 1", m);
    const size_t h = std::max<size_t>(m / 2, 1);
    if (int rc = cmux_check_sizes<F>(pl, k, base_log, levels, batch, h, m > 1)) return rc;
    unsigned depth = 0;
    while (((size_t)1 << depth) < m) ++depth;
    const size_t n = pl->n, w = F::word(pl);
    // the byte counts are products of the arguments: they must fit before they are formed
    if (product_passes_2_63({batch, m, n, w}) || product_passes_2_63({batch, h, k + 1, levels, n, w}) ||
        product_passes_2_63({(size_t)depth, k + 1, levels, k + 1, n, w}) || product_passes_2_63({k + 1, levels, k + 1, n, w}))
        return fail(CNTT_EINVAL, "lut_count = %zu, glwe_dim = %zu, levels = %u, batch = %zu: the table, the ciphertexts, the digits or the selectors pass 2^63 bytes",
                    m, k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lut_in) return fail(CNTT_EINVAL, "lut_in is NULL");
    if (depth > 0)
        if (int rc = F::key_check(pl, ggsw_ntt, "ggsw_ntt")) return rc;
    const size_t ob = batch * (k + 1) * n * w, ib = batch * m * n * w, kb = F::key_bytes(pl, (size_t)depth * (k + 1) * levels * (k + 1));
    const CmuxSizes Z = cmux_tree_sizes<F>(pl, m, k, levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    Operand ops[CMUX_MAX_OPERANDS] = {{"glwe_out", glwe_out, ob, w, true}, {"lut_in", lut_in, ib, w, false}};
    if (int rc = cmux_check_operands(pl, ops, 2, ggsw_ntt, kb, workspace, workspace_bytes)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *din = (const W *)s.in(lut_in, ib);
    const typename F::Key dsel = depth > 0 ? F::key_in(pl, s, ggsw_ntt, kb, ks) : typename F::Key{};
    W *dout = (W *)s.out(glwe_out, ob);
    char *dws = (char *)s.workspace(workspace, need, depth > 0);   // one block for the whole call
    if (int rc = s.status()) return rc;
    W *terms = static_cast<W *>(static_cast<void *>(dws));
    W *buf_a = static_cast<W *>(static_cast<void *>(dws + up256(Z.digits)));
    W *buf_b = static_cast<W *>(static_cast<void *>(dws + up256(Z.digits) + up256(Z.buf_a)));
    if (int rc = cmux_tree_device<F>(pl, dout, din, dsel, m, k, base_log, levels, batch, terms, buf_a, buf_b, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_glwe_cmux_batch(const cntt_native_t *pl, void *glwe_out, const void *glwe0, const void *glwe1,
                                           const void *const *ggsw_ntt, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
                                           void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return glwe_cmux<NativeCmux>(pl, glwe_out, glwe0, glwe1, ggsw_ntt, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,
                                 (hipStream_t)stream);
}
extern "C" size_t cntt_native_glwe_cmux_workspace_bytes(const cntt_native_t *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return cmux_workspace_bytes<NativeCmux>(pl, glwe_dim, levels, batch);
}
extern "C" int cntt_native_cmux_tree_batch(const cntt_native_t *pl, void *glwe_out, const void *lut_in, const void *const *ggsw_ntt,
                                           size_t lut_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                           size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return cmux_tree<NativeCmux>(pl, glwe_out, lut_in, ggsw_ntt, lut_count, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,
                                 (hipStream_t)stream);
}
extern "C" size_t cntt_native_cmux_tree_workspace_bytes(const cntt_native_t *pl, size_t lut_count, size_t glwe_dim, unsigned levels, size_t batch) {
    return cmux_tree_workspace_bytes<NativeCmux>(pl, lut_count, glwe_dim, levels, batch);
}
extern "C" unsigned cntt_native_cmux_grid(size_t polys, int logn, size_t word_bytes) { return native_cmux_grid(polys, logn, word_bytes); }
