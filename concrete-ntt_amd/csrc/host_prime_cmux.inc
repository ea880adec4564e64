// Part of host_prime.hip (included at its end, after host_prime_ring_pack.inc): the CMux and the CMux tree against GGSW selectors
// (include/cntt_prime_cmux.h) -- the argument checks, the workspace layout, the host-slice path and the C ABI over the kernel of
// prime_cmux.hpp (launched by prime_cmux.hip), gadget_check and external_product_device, which it calls and does not change.
#include "../../include/cntt_prime_cmux.h"
#include "prime_cmux.hpp"

#pragma GCC visibility push(hidden)

// the three parts of the tree's workspace: the digits of the widest stage, and the two ciphertext buffers the stages alternate between
struct CmuxTreeSizes {
    size_t digits, buf_a, buf_b;
    size_t total() const { return up256(digits) + up256(buf_a) + up256(buf_b); }
};
template <class T> static CmuxTreeSizes cmux_tree_sizes(const PrimePlan<T> *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    const size_t h = m / 2, q = m / 4, ct = (k + 1) * pl->n * sizeof(T);
    return CmuxTreeSizes{std::max(batch * h * levels, batch * q * (k + 1) * levels) * pl->n * sizeof(T), batch * h * ct, batch * q * ct};
}
template <class T> static size_t cmux_digit_bytes(const PrimePlan<T> *pl, size_t terms_per, unsigned levels, size_t nct) {
    return nct * terms_per * levels * pl->n * sizeof(T);
}
template <class T> static size_t cmux_workspace_bytes(const PrimePlan<T> *pl, size_t k, unsigned levels, size_t batch) {
    return pl ? up256(cmux_digit_bytes(pl, k + 1, levels, batch)) : 0;
}
template <class T> static size_t cmux_tree_workspace_bytes(const PrimePlan<T> *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    return pl ? cmux_tree_sizes(pl, m, k, levels, batch).total() : 0;
}

// the checks the two calls share; the widest launch holds cts ciphertexts per batch element
template <class T> static int cmux_check_sizes(const PrimePlan<T> *pl, size_t k, unsigned base_log, unsigned levels, size_t batch, size_t cts) {
    if (int rc = gadget_check<PrimePbs<T>>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if ((u128)batch * cts >= ((u128)1 << 64) || (u128)batch * cts * (k + 1) * levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * ciphertexts per element * (glwe_dim + 1) * levels = %zu * %zu * %zu * %u is not below 2^32: too large for one launch",
                    batch, cts, k + 1, levels);
    return CNTT_OK;
}

// One stage for nct output ciphertexts: one launch writes the prefilled output and the digits, the external product accumulates.  leaf:
// the sources are plain polynomials standing for trivial ciphertexts, only their bodies have digits, and these meet the selector's body
// rows only.  sel == nullptr (leaf): the trivial ciphertexts and nothing else.
template <class T>
static int cmux_device(const PrimePlan<T> *pl, T *out, const T *c0, const T *c1, bool leaf, const T *sel, size_t k, unsigned base_log, unsigned levels,
                       size_t h, size_t gs, size_t nct, T *terms, hipStream_t st) {
    const bool digits = !leaf || sel;
    const bool stream = digits && cmux_digit_bytes(pl, leaf ? 1 : k + 1, levels, nct) > STREAM_BYTES;
    const hipError_t e = launch_prime_cmux_diff<T>(digits ? terms : nullptr, out, c0, c1, leaf, prime_pack_const(pl, base_log, levels), pl->logn, k, h, gs,
                                                   nct, stream, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_cmux_diff_kernel launch failed: %s", hipGetErrorString(e));
    if (!digits) return CNTT_OK;
    if (leaf) return external_product_device<T>(pl, out, terms, sel + k * levels * (k + 1) * pl->n, levels, k + 1, nct, true, st);
    return external_product_device<T>(pl, out, terms, sel, (k + 1) * levels, k + 1, nct, true, st);
}

// call 1 of the header
template <class T>
static int glwe_cmux(const PrimePlan<T> *pl, T *glwe_out, const T *glwe0, const T *glwe1, const T *ggsw_ntt, size_t k, unsigned base_log,
                     unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = cmux_check_sizes(pl, k, base_log, levels, batch, 1)) return rc;
    if (product_passes_2_63({batch, k + 1, levels, pl->n, sizeof(T)}) || product_passes_2_63({k + 1, levels, k + 1, pl->n, sizeof(T)}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the selector pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!glwe0) return fail(CNTT_EINVAL, "glwe0 is NULL");
    if (!glwe1) return fail(CNTT_EINVAL, "glwe1 is NULL");
    if (!ggsw_ntt) return fail(CNTT_EINVAL, "ggsw_ntt is NULL");
    const size_t n = pl->n, cb = batch * (k + 1) * n * sizeof(T), kb = (k + 1) * levels * (k + 1) * n * sizeof(T);
    const size_t need = cmux_workspace_bytes(pl, k, levels, batch);
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const Operand ops[5] = {{"glwe_out", glwe_out, cb, sizeof(T), true},
                            {"glwe0", glwe0, cb, sizeof(T), false},
                            {"glwe1", glwe1, cb, sizeof(T), false},
                            {"ggsw_ntt", ggsw_ntt, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    Staging s(where, st);
    const T *d0 = (const T *)s.in(glwe0, cb), *d1 = (const T *)s.in(glwe1, cb), *dsel = (const T *)s.in(ggsw_ntt, kb);
    T *dout = (T *)s.out(glwe_out, cb);
    T *dterms = (T *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = cmux_device<T>(pl, dout, d0, d1, false, dsel, k, base_log, levels, 1, 1, batch, dterms, st)) return rc;
    return s.finish();
}

// The tree.  Stage s = 1 .. depth (h = m / 2^s) selects between entries j and j + h of the previous stage with selector depth - s;
// stage 1 reads the table polynomials as leaves.  Stage outputs alternate between buf_a (odd s) and buf_b (even s); the last stage
// writes `out`.  m == 1: the trivial ciphertext.
template <class T>
static int cmux_tree_device(const PrimePlan<T> *pl, T *out, const T *lut, const T *sel, size_t m, size_t k, unsigned base_log, unsigned levels,
                            size_t batch, T *terms, T *buf_a, T *buf_b, hipStream_t st) {
    const size_t n = pl->n, sel_polys = (k + 1) * levels * (k + 1);
    unsigned depth = 0;
    while (((size_t)1 << depth) < m) ++depth;
    if (depth == 0) return cmux_device<T>(pl, out, lut, lut, true, nullptr, k, base_log, levels, 1, 1, batch, nullptr, st);
    const T *cur = lut;
    for (unsigned s = 1; s <= depth; ++s) {
        const size_t h = m >> s;
        T *dst = s == depth ? out : s % 2 ? buf_a : buf_b;
        const T *c1 = cur + h * (s == 1 ? n : (k + 1) * n);
        if (int rc = cmux_device<T>(pl, dst, cur, c1, s == 1, sel + (size_t)(depth - s) * sel_polys * n, k, base_log, levels, h, 2 * h, batch * h, terms, st))
            return rc;
        cur = dst;
    }
    return CNTT_OK;
}

// call 2 of the header
template <class T>
static int cmux_tree(const PrimePlan<T> *pl, T *glwe_out, const T *lut_in, const T *ggsw_ntt, size_t m, size_t k, unsigned base_log, unsigned levels,
                     size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (m == 0 || (m & (m - 1))) return fail(CNTT_EINVAL, "lut_count = %zu is not a power of two >= 1", m);
    const size_t h = std::max<size_t>(m / 2, 1);
    if (int rc = cmux_check_sizes(pl, k, base_log, levels, batch, h)) return rc;
    unsigned depth = 0;
    while (((size_t)1 << depth) < m) ++depth;
    // the byte counts are products of the arguments: they must fit before they are formed
    if (product_passes_2_63({batch, m, pl->n, sizeof(T)}) || product_passes_2_63({batch, h, k + 1, levels, pl->n, sizeof(T)}) ||
        product_passes_2_63({(size_t)depth, k + 1, levels, k + 1, pl->n, sizeof(T)}) || product_passes_2_63({k + 1, levels, k + 1, pl->n, sizeof(T)}))
        return fail(CNTT_EINVAL, "lut_count = %zu, glwe_dim = %zu, levels = %u, batch = %zu: the table, the ciphertexts, the digits or the selectors pass 2^63 bytes",
                    m, k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lut_in) return fail(CNTT_EINVAL, "lut_in is NULL");
    if (depth > 0 && !ggsw_ntt) return fail(CNTT_EINVAL, "ggsw_ntt is NULL");
    const size_t n = pl->n, ob = batch * (k + 1) * n * sizeof(T), ib = batch * m * n * sizeof(T),
                 kb = (size_t)depth * (k + 1) * levels * (k + 1) * n * sizeof(T);
    const CmuxTreeSizes Z = cmux_tree_sizes(pl, m, k, levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const Operand ops[4] = {{"glwe_out", glwe_out, ob, sizeof(T), true},
                            {"lut_in", lut_in, ib, sizeof(T), false},
                            {"ggsw_ntt", depth > 0 ? ggsw_ntt : nullptr, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 4)) return rc;
    Staging s(where, st);
    const T *din = (const T *)s.in(lut_in, ib), *dsel = depth > 0 ? (const T *)s.in(ggsw_ntt, kb) : nullptr;
    T *dout = (T *)s.out(glwe_out, ob);
    char *dws = (char *)s.workspace(workspace, need, depth > 0);   // one block for the whole call
    if (int rc = s.status()) return rc;
    T *terms = static_cast<T *>(static_cast<void *>(dws));
    T *buf_a = static_cast<T *>(static_cast<void *>(dws + up256(Z.digits)));
    T *buf_b = static_cast<T *>(static_cast<void *>(dws + up256(Z.digits) + up256(Z.buf_a)));
    if (int rc = cmux_tree_device<T>(pl, dout, din, dsel, m, k, base_log, levels, batch, terms, buf_a, buf_b, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_CMUX_API(BITS, T, PLAN)                                                                                                   \
    extern "C" int cntt_prime##BITS##_glwe_cmux_batch(const PLAN *pl, T *glwe_out, const T *glwe0, const T *glwe1, const T *ggsw_ntt,        \
                                                      size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,    \
                                                      size_t workspace_bytes, cntt_mem_t where, void *stream) {                              \
        return glwe_cmux<T>(pl, glwe_out, glwe0, glwe1, ggsw_ntt, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,      \
                            (hipStream_t)stream);                                                                                            \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_glwe_cmux_workspace_bytes(const PLAN *pl, size_t glwe_dim, unsigned levels, size_t batch) {         \
        return cmux_workspace_bytes<T>(pl, glwe_dim, levels, batch);                                                                         \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_cmux_tree_batch(const PLAN *pl, T *glwe_out, const T *lut_in, const T *ggsw_ntt, size_t lut_count,     \
                                                      size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,    \
                                                      size_t workspace_bytes, cntt_mem_t where, void *stream) {                              \
        return cmux_tree<T>(pl, glwe_out, lut_in, ggsw_ntt, lut_count, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where, \
                            (hipStream_t)stream);                                                                                            \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_cmux_tree_workspace_bytes(const PLAN *pl, size_t lut_count, size_t glwe_dim, unsigned levels,       \
                                                                   size_t batch) {                                                           \
        return cmux_tree_workspace_bytes<T>(pl, lut_count, glwe_dim, levels, batch);                                                         \
    }

CNTT_PRIME_CMUX_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_CMUX_API(32, uint32_t, cntt_plan32)

extern "C" unsigned cntt_prime_cmux_grid(size_t polys, int logn, size_t word_bytes) { return prime_cmux_grid(polys, logn, word_bytes); }
