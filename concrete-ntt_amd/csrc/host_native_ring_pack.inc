// Part of host_native_ext.hip (included at its end, after host_native_automorphism.inc, whose trace_device, autoks_digit_bytes,
// native_autom_check_t and testing switch it uses unchanged): ring packing of LWE ciphertexts through automorphisms
// (include/cntt_ring_pack.h) -- the argument checks, the workspace layout, the host-slice path and the C ABI over the two kernels of
// native_ring_pack.hpp (launched by native_ring_pack.hip), the family's external product (native_ext_device) and trace_device, which it
// calls and does not change.  Templates over a plan family F in the style of host_native_automorphism.inc: F is NativeAutom plus the two
// launchers below.
#include "../../include/cntt_ring_pack.h"
#include "native_ring_pack.hpp"

#pragma GCC visibility push(hidden)

struct NativeRing : NativeAutom {
    static hipError_t launch_glwe_embed(const cntt_native *pl, void *glwe, const void *lwe, size_t glwe_dim, size_t batch, hipStream_t st) {
        return launch_native_glwe_embed(pl->info.word, glwe, lwe, native_logn(pl), glwe_dim, batch, st);
    }
    static hipError_t launch_ring_merge(const cntt_native *pl, void *terms, void *out, const void *even, const void *odd, bool leaf,
                                        unsigned base_log, unsigned levels, size_t t, size_t shift, size_t glwe_dim, size_t h, size_t gs,
                                        size_t nct, bool stream, hipStream_t st) {
        const u128 off = gadget_offset(digit_bits(pl), base_log, levels);
        return launch_native_ring_merge(pl->info.word, terms, out, even, odd, leaf, (uint64_t)off, (uint64_t)(off >> 64), base_log, levels,
                                        (uint32_t)t, (uint32_t)shift, native_logn(pl), glwe_dim, h, gs, nct, stream, native_autom_lds_enabled(), st);
    }
};

// the three parts of the ring-pack workspace: the digits of the widest stage, and the two ciphertext buffers the stages alternate between
struct RingPackSizes {
    size_t digits, buf_a, buf_b;
    size_t total() const { return up256(digits) + up256(buf_a) + up256(buf_b); }
};
template <class F> static RingPackSizes ring_pack_sizes(const typename F::Plan *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    const size_t h = std::max<size_t>(m / 2, 1), q = std::max<size_t>(m / 4, 1), ct = (k + 1) * pl->n * F::word(pl);
    return RingPackSizes{batch * h * k * levels * pl->n * F::word(pl), batch * h * ct, batch * q * ct};
}
template <class F> static size_t ring_pack_workspace_bytes(const typename F::Plan *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    return pl ? ring_pack_sizes<F>(pl, m, k, levels, batch).total() : 0;
}

// the checks of the Galois keyswitch that the merge and the pack share; the widest launch holds cts_batch * cts_per ciphertexts
template <class F>
static int ring_check_sizes(const typename F::Plan *pl, size_t k, unsigned base_log, unsigned levels, size_t cts_batch, size_t cts_per) {
    if (pl->info.binary)
        return fail(CNTT_EINVAL, "plan is of a native_binary kind: a keyswitching key has full-width words, and the exactness of these kinds rests on "
                                 "a 0 / 1 key");
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (k * levels > pl->max_terms)   // (k < 2^32 and levels <= 128: the product does not wrap)
        return fail(CNTT_EINVAL, "glwe_dim * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range",
                    k * levels, pl->max_terms);
    const size_t launch = std::max<size_t>(k * levels, k + 1);
    if ((u128)cts_batch * cts_per >= ((u128)1 << 64) || (u128)cts_batch * cts_per * launch >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * ciphertexts per element * max(glwe_dim * levels, glwe_dim + 1) = %zu * %zu * %zu is not below 2^32: too large for one launch",
                    cts_batch, cts_per, launch);
    return CNTT_OK;
}

template <class F>
static int embed_device(const typename F::Plan *pl, typename F::Word *glwe, const typename F::Word *lwe, size_t k, size_t batch, hipStream_t st) {
    const hipError_t e = F::launch_glwe_embed(pl, glwe, lwe, k, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_glwe_embed_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}

// one tree node for nct output ciphertexts: one launch writes the prefilled output and the negated digits, the external product accumulates
template <class F>
static int merge_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *even, const typename F::Word *odd, bool leaf,
                        typename F::Key ak, size_t shift, size_t t, size_t k, unsigned base_log, unsigned levels, size_t h, size_t gs, size_t nct,
                        typename F::Word *terms, hipStream_t st) {
    const hipError_t e = F::launch_ring_merge(pl, terms, out, even, odd, leaf, base_log, levels, t, shift, k, h, gs, nct,
                                              autoks_digit_bytes<F>(pl, k, levels, nct) > STREAM_BYTES, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_ring_merge_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    if (k == 0) return CNTT_OK;
    return F::ext_product(pl, out, terms, ak, k * levels, k + 1, nct, true, st);
}

// call 1 of the header: every kind, no key is read
template <class F>
static int glwe_embed(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *lwe_in, size_t k, size_t batch, cntt_mem_t where,
                      hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t n = pl->n, w = F::word(pl);
    if (product_passes_2_63({batch, k + 1, n, w})) return fail(CNTT_EINVAL, "glwe_dim = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", k, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    const size_t gb = batch * (k + 1) * n * w, lb = batch * (k * n + 1) * w;
    const Operand ops[2] = {{"glwe_out", glwe_out, gb, w, true}, {"lwe_in", lwe_in, lb, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    W *dout = (W *)s.out(glwe_out, gb);
    const W *din = (const W *)s.in(lwe_in, lb);
    if (int rc = s.status()) return rc;
    if (int rc = embed_device<F>(pl, dout, din, k, batch, st)) return rc;
    return s.finish();
}

// call 2 of the header
template <class F>
static int glwe_merge(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *even, const typename F::Word *odd,
                      typename F::Key ak_ntt, size_t shift, size_t t, size_t k, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                      size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = native_autom_check_t(pl, t)) return rc;
    if (shift >= 2 * pl->n) return fail(CNTT_EINVAL, "shift = %zu is not below 2n = %zu", shift, 2 * pl->n);
    if (int rc = ring_check_sizes<F>(pl, k, base_log, levels, batch, 1)) return rc;
    // the byte counts -- ciphertexts, digits, key -- are products of the arguments: they must fit before they are formed
    const size_t n = pl->n, w = F::word(pl);
    if (product_passes_2_63({batch, k + 1, n, w}) || product_passes_2_63({batch, k, levels, n, w}) || product_passes_2_63({k, levels, k + 1, n, w}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the key pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!even) return fail(CNTT_EINVAL, "glwe_even is NULL");
    if (!odd) return fail(CNTT_EINVAL, "glwe_odd is NULL");
    if (k > 0)
        if (int rc = F::key_check(pl, ak_ntt, "ak_ntt")) return rc;
    const size_t cb = batch * (k + 1) * n * w, kb = k > 0 ? F::key_bytes(pl, k * levels * (k + 1)) : 0;
    const size_t need = autoks_workspace_bytes<F>(pl, k, levels, batch);
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    Operand ops[14] = {{"glwe_out", glwe_out, cb, w, true}, {"glwe_even", even, cb, w, false}, {"glwe_odd", odd, cb, w, false}};
    int cnt = 3;
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {AUTOM_KEY_PLANE[i], ak_ntt[i], kb, pl->rbytes(), false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *de = (const W *)s.in(even, cb), *dod = (const W *)s.in(odd, cb);
    const typename F::Key dak = k > 0 ? F::key_in(pl, s, ak_ntt, kb, ks) : typename F::Key{};
    W *dout = (W *)s.out(glwe_out, cb);
    W *dterms = (W *)s.workspace(workspace, need, k > 0);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = merge_device<F>(pl, dout, de, dod, false, dak, shift, t, k, base_log, levels, 1, 1, batch, dterms, st)) return rc;
    return s.finish();
}

// The tree and the trace.  Stage s = 1 .. l (l = log2 m, h = m / 2^s) merges ciphertexts j and j + h of the previous stage with
// shift = n / 2^s and t = 2^s + 1, the key of trace round log2 n - s; stage 1 reads the LWE rows as leaves.  Stage outputs alternate
// between buf_a (odd s) and buf_b (even s); the trace of log2 n - l steps follows on one ciphertext per batch element with the idle buffer
// as its second ciphertext.  The last operation of all writes `out`.
template <class F>
static int ring_pack_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *lwe, typename F::Key ak, size_t m, size_t k,
                            unsigned base_log, unsigned levels, size_t batch, typename F::Word *terms, typename F::Word *buf_a,
                            typename F::Word *buf_b, hipStream_t st) {
    using W = typename F::Word;
    const size_t n = pl->n, w = F::word(pl), slice = F::key_bytes(pl, k * levels * (k + 1));   // one key
    const unsigned logn = (unsigned)F::logn(pl);
    unsigned l = 0;
    while (((size_t)1 << l) < m) ++l;
    const unsigned steps = logn - l;
    const W *cur = nullptr;
    W *idle = buf_b;
    if (l == 0) {
        if (int rc = embed_device<F>(pl, buf_a, lwe, k, batch, st)) return rc;
        cur = buf_a;
    }
    typename F::KeyStore ks;
    for (unsigned s = 1; s <= l; ++s) {
        const size_t h = m >> s;
        W *dst = s == l && steps == 0 ? out : s % 2 ? buf_a : buf_b;
        const typename F::Key key = k ? F::key_at(pl, ak, (size_t)(logn - s) * slice, ks) : typename F::Key{};
        const W *even = s == 1 ? lwe : cur, *odd = cmux_at(even, h * (s == 1 ? k * n + 1 : (k + 1) * n) * w);
        if (int rc = merge_device<F>(pl, dst, even, odd, s == 1, key, n >> s, ((size_t)1 << s) + 1, k, base_log, levels, h, 2 * h, batch * h, terms, st))
            return rc;
        cur = dst;
        idle = s % 2 ? buf_b : buf_a;
    }
    if (steps == 0) return CNTT_OK;
    return trace_device<F>(pl, out, cur, ak, steps, k, base_log, levels, batch, terms, idle, st);
}

// call 3 of the header
template <class F>
static int ring_pack(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *lwe_in, typename F::Key ak_ntt, size_t m, size_t k,
                     unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (m == 0 || (m & (m - 1)) || m > pl->n)
        return fail(CNTT_EINVAL, "lwe_count = %zu is not a power of two in 1 .. ntt_size = %zu", m, pl->n);
    const size_t h = std::max<size_t>(m / 2, 1);
    if (int rc = ring_check_sizes<F>(pl, k, base_log, levels, batch, h)) return rc;
    // the byte counts are products of the arguments: they must fit before they are formed (batch * h * (k + 1) < 2^32 and m <= 2 h keep
    // the 128-bit product of the LWE rows itself from wrapping)
    const size_t n = pl->n, w = F::word(pl), logn = (size_t)F::logn(pl);
    if ((u128)batch * m * ((u128)k * n + 1) * w >= ((u128)1 << 63) || product_passes_2_63({batch, h, k + 1, n, w}) ||
        product_passes_2_63({batch, h, k, levels, n, w}) || product_passes_2_63({logn, k, levels, k + 1, n, w}))
        return fail(CNTT_EINVAL, "lwe_count = %zu, glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the keys pass 2^63 bytes", m, k,
                    levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (k > 0)
        if (int rc = F::key_check(pl, ak_ntt, "ak_ntt")) return rc;
    const size_t ob = batch * (k + 1) * n * w, ib = batch * m * (k * n + 1) * w, kb = k > 0 ? F::key_bytes(pl, logn * k * levels * (k + 1)) : 0;
    const RingPackSizes Z = ring_pack_sizes<F>(pl, m, k, levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    Operand ops[13] = {{"glwe_out", glwe_out, ob, w, true}, {"lwe_in", lwe_in, ib, w, false}};
    int cnt = 2;
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {AUTOM_KEY_PLANE[i], ak_ntt[i], kb, pl->rbytes(), false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *din = (const W *)s.in(lwe_in, ib);
    const typename F::Key dak = k > 0 ? F::key_in(pl, s, ak_ntt, kb, ks) : typename F::Key{};
    W *dout = (W *)s.out(glwe_out, ob);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    W *terms = static_cast<W *>(static_cast<void *>(dws));
    W *buf_a = static_cast<W *>(static_cast<void *>(dws + up256(Z.digits)));
    W *buf_b = static_cast<W *>(static_cast<void *>(dws + up256(Z.digits) + up256(Z.buf_a)));
    if (int rc = ring_pack_device<F>(pl, dout, din, dak, m, k, base_log, levels, batch, terms, buf_a, buf_b, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_glwe_embed_batch(const cntt_native_t *pl, void *glwe_out, const void *lwe_in, size_t glwe_dim, size_t batch,
                                            cntt_mem_t where, void *stream) {
    return glwe_embed<NativeRing>(pl, glwe_out, lwe_in, glwe_dim, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_glwe_merge_batch(const cntt_native_t *pl, void *glwe_out, const void *glwe_even, const void *glwe_odd,
                                            const void *const *ak_ntt, size_t shift, size_t t, size_t glwe_dim, unsigned base_log,
                                            unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                                            void *stream) {
    return glwe_merge<NativeRing>(pl, glwe_out, glwe_even, glwe_odd, ak_ntt, shift, t, glwe_dim, base_log, levels, batch, workspace,
                                  workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_glwe_merge_workspace_bytes(const cntt_native_t *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return autoks_workspace_bytes<NativeRing>(pl, glwe_dim, levels, batch);
}
extern "C" int cntt_native_ring_pack_batch(const cntt_native_t *pl, void *glwe_out, const void *lwe_in, const void *const *ak_ntt,
                                           size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                           size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return ring_pack<NativeRing>(pl, glwe_out, lwe_in, ak_ntt, lwe_count, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,
                                 (hipStream_t)stream);
}
extern "C" size_t cntt_native_ring_pack_workspace_bytes(const cntt_native_t *pl, size_t lwe_count, size_t glwe_dim, unsigned levels, size_t batch) {
    return ring_pack_workspace_bytes<NativeRing>(pl, lwe_count, glwe_dim, levels, batch);
}
extern "C" unsigned cntt_native_ring_pack_grid(size_t polys, int logn, size_t word_bytes) { return native_ring_pack_grid(polys, logn, word_bytes); }
