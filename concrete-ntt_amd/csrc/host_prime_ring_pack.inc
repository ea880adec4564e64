// Part of host_prime.hip (included at its end, after host_prime_automorphism.inc, whose autoks checks, trace_device and testing switch it
// uses): ring packing of LWE ciphertexts through automorphisms (include/cntt_prime_ring_pack.h) -- the argument checks, the workspace
// layout, the host-slice path and the C ABI over the two kernels of prime_ring_pack.hpp (launched by prime_ring_pack.hip),
// external_product_device and trace_device, which it calls and does not change.
#include "../../include/cntt_prime_ring_pack.h"
#include "prime_ring_pack.hpp"

#pragma GCC visibility push(hidden)

// the three parts of the ring-pack workspace: the digits of the widest stage, and the two ciphertext buffers the stages alternate between
struct RingPackSizes {
    size_t digits, buf_a, buf_b;
    size_t total() const { return up256(digits) + up256(buf_a) + up256(buf_b); }
};
template <class T> static RingPackSizes ring_pack_sizes(const PrimePlan<T> *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    const size_t h = std::max<size_t>(m / 2, 1), q = std::max<size_t>(m / 4, 1), ct = (k + 1) * pl->n * sizeof(T);
    return RingPackSizes{batch * h * k * levels * pl->n * sizeof(T), batch * h * ct, batch * q * ct};
}
template <class T> static size_t ring_pack_workspace_bytes(const PrimePlan<T> *pl, size_t m, size_t k, unsigned levels, size_t batch) {
    return pl ? ring_pack_sizes(pl, m, k, levels, batch).total() : 0;
}

// the checks of the Galois keyswitch that the merge and the pack share; the widest launch holds cts_batch * cts_per ciphertexts
template <class T> static int ring_check_sizes(const PrimePlan<T> *pl, size_t k, unsigned base_log, unsigned levels, size_t cts_batch, size_t cts_per) {
    if (int rc = gadget_check<PrimePbs<T>>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t launch = std::max<size_t>(k * levels, k + 1);
    if ((u128)cts_batch * cts_per * launch >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * ciphertexts per element * max(glwe_dim * levels, glwe_dim + 1) = %zu * %zu * %zu is not below 2^32: too large for one launch",
                    cts_batch, cts_per, launch);
    return CNTT_OK;
}

template <class T> static int embed_device(const PrimePlan<T> *pl, T *glwe, const T *lwe, size_t k, size_t batch, hipStream_t st) {
    const hipError_t e = launch_prime_glwe_embed<T>(glwe, lwe, pl->p, pl->logn, k, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_glwe_embed_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

// one tree node for nct output ciphertexts: one launch writes the prefilled output and the negated digits, the external product accumulates
template <class T>
static int merge_device(const PrimePlan<T> *pl, T *out, const T *even, const T *odd, bool leaf, const T *ak, size_t shift, size_t t, size_t k,
                        unsigned base_log, unsigned levels, size_t h, size_t gs, size_t nct, T *terms, hipStream_t st) {
    const hipError_t e = launch_prime_ring_merge<T>(terms, out, even, odd, leaf, prime_pack_const(pl, base_log, levels), (uint32_t)t, (uint32_t)shift,
                                                    pl->logn, k, h, gs, nct, autoks_digit_bytes(pl, k, levels, nct) > STREAM_BYTES, autom_lds_enabled(), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_ring_merge_kernel launch failed: %s", hipGetErrorString(e));
    if (k == 0) return CNTT_OK;
    return external_product_device<T>(pl, out, terms, ak, k * levels, k + 1, nct, true, st);
}

// call 1 of the header
template <class T> static int glwe_embed(const PrimePlan<T> *pl, T *glwe_out, const T *lwe_in, size_t k, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if ((u128)batch * (k + 1) * pl->n * sizeof(T) >= ((u128)1 << 63))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, batch = %zu: the ciphertexts pass 2^63 bytes", k, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    const size_t gb = batch * (k + 1) * pl->n * sizeof(T), lb = batch * (k * pl->n + 1) * sizeof(T);
    const Operand ops[2] = {{"glwe_out", glwe_out, gb, sizeof(T), true}, {"lwe_in", lwe_in, lb, sizeof(T), false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    T *dout = (T *)s.out(glwe_out, gb);
    const T *din = (const T *)s.in(lwe_in, lb);
    if (int rc = s.status()) return rc;
    if (int rc = embed_device<T>(pl, dout, din, k, batch, st)) return rc;
    return s.finish();
}

// call 2 of the header
template <class T>
static int glwe_merge(const PrimePlan<T> *pl, T *glwe_out, const T *even, const T *odd, const T *ak_ntt, size_t shift, size_t t, size_t k,
                      unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = autom_check_t(pl, t)) return rc;
    if (shift >= 2 * pl->n) return fail(CNTT_EINVAL, "shift = %zu is not below 2n = %zu", shift, 2 * pl->n);
    if (int rc = ring_check_sizes(pl, k, base_log, levels, batch, 1)) return rc;
    const u128 lim = (u128)1 << 63, wb = sizeof(T);
    if ((u128)batch * (k + 1) * pl->n * wb >= lim || (u128)batch * k * levels * pl->n * wb >= lim || (u128)k * levels * (k + 1) * pl->n * wb >= lim)
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the key pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!even) return fail(CNTT_EINVAL, "glwe_even is NULL");
    if (!odd) return fail(CNTT_EINVAL, "glwe_odd is NULL");
    if (k > 0 && !ak_ntt) return fail(CNTT_EINVAL, "ak_ntt is NULL");
    const size_t n = pl->n, cb = batch * (k + 1) * n * sizeof(T), kb = k * levels * (k + 1) * n * sizeof(T);
    const size_t need = autoks_workspace_bytes(pl, k, levels, batch);
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const Operand ops[5] = {{"glwe_out", glwe_out, cb, sizeof(T), true},
                            {"glwe_even", even, cb, sizeof(T), false},
                            {"glwe_odd", odd, cb, sizeof(T), false},
                            {"ak_ntt", ak_ntt, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 5)) return rc;
    Staging s(where, st);
    const T *de = (const T *)s.in(even, cb), *dod = (const T *)s.in(odd, cb), *dak = k > 0 ? (const T *)s.in(ak_ntt, kb) : nullptr;
    T *dout = (T *)s.out(glwe_out, cb);
    T *dterms = (T *)s.workspace(workspace, need, k > 0);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = merge_device<T>(pl, dout, de, dod, false, dak, shift, t, k, base_log, levels, 1, 1, batch, dterms, st)) return rc;
    return s.finish();
}

// The tree and the trace.  Stage s = 1 .. l (l = log2 m, h = m / 2^s) merges ciphertexts j and j + h of the previous stage with
// shift = n / 2^s and t = 2^s + 1, the key of trace round log2 n - s; stage 1 reads the LWE rows as leaves.  Stage outputs alternate
// between buf_a (odd s) and buf_b (even s); the trace of log2 n - l steps follows on one ciphertext per batch element with the idle buffer
// as its second ciphertext.  The last operation of all writes `out`.
template <class T>
static int ring_pack_device(const PrimePlan<T> *pl, T *out, const T *lwe, const T *ak, size_t m, size_t k, unsigned base_log, unsigned levels,
                            size_t batch, T *terms, T *buf_a, T *buf_b, hipStream_t st) {
    const size_t n = pl->n, key_polys = k * levels * (k + 1);
    unsigned l = 0;
    while (((size_t)1 << l) < m) ++l;
    const unsigned steps = (unsigned)pl->logn - l;
    const T *cur = nullptr;
    T *idle = buf_b;
    if (l == 0) {
        if (int rc = embed_device<T>(pl, buf_a, lwe, k, batch, st)) return rc;
        cur = buf_a;
    }
    for (unsigned s = 1; s <= l; ++s) {
        const size_t h = m >> s;
        T *dst = s == l && steps == 0 ? out : s % 2 ? buf_a : buf_b;
        const T *key = ak ? ak + ((size_t)pl->logn - s) * key_polys * n : nullptr;
        const T *even = s == 1 ? lwe : cur, *odd = even + h * (s == 1 ? k * n + 1 : (k + 1) * n);
        if (int rc = merge_device<T>(pl, dst, even, odd, s == 1, key, n >> s, ((size_t)1 << s) + 1, k, base_log, levels, h, 2 * h, batch * h, terms, st))
            return rc;
        cur = dst;
        idle = s % 2 ? buf_b : buf_a;
    }
    if (steps == 0) return CNTT_OK;
    return trace_device<T>(pl, out, cur, ak, steps, k, base_log, levels, batch, terms, idle, st);
}

// call 3 of the header
template <class T>
static int ring_pack(const PrimePlan<T> *pl, T *glwe_out, const T *lwe_in, const T *ak_ntt, size_t m, size_t k, unsigned base_log, unsigned levels,
                     size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (m == 0 || (m & (m - 1)) || m > pl->n)
        return fail(CNTT_EINVAL, "lwe_count = %zu is not a power of two in 1 .. ntt_size = %zu", m, pl->n);
    const size_t h = std::max<size_t>(m / 2, 1);
    if (int rc = ring_check_sizes(pl, k, base_log, levels, batch, h)) return rc;
    // the byte counts are products of the arguments: they must fit before they are formed (batch * h * (k + 1) < 2^32 and k + 1 < 2^32
    // keep the 128-bit products themselves from wrapping)
    const u128 lim = (u128)1 << 63, wb = sizeof(T);
    if ((u128)batch * m * ((u128)k * pl->n + 1) * wb >= lim || (u128)batch * h * (k + 1) * pl->n * wb >= lim ||
        (u128)batch * h * k * levels * pl->n * wb >= lim || (u128)pl->logn * k * levels * (k + 1) * pl->n * wb >= lim)
        return fail(CNTT_EINVAL, "lwe_count = %zu, glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the keys pass 2^63 bytes", m, k,
                    levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (k > 0 && !ak_ntt) return fail(CNTT_EINVAL, "ak_ntt is NULL");
    const size_t n = pl->n, ob = batch * (k + 1) * n * sizeof(T), ib = batch * m * (k * n + 1) * sizeof(T),
                 kb = (size_t)pl->logn * k * levels * (k + 1) * n * sizeof(T);
    const RingPackSizes Z = ring_pack_sizes(pl, m, k, levels, batch);
    const size_t need = Z.total();
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const Operand ops[4] = {{"glwe_out", glwe_out, ob, sizeof(T), true},
                            {"lwe_in", lwe_in, ib, sizeof(T), false},
                            {"ak_ntt", ak_ntt, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 4)) return rc;
    Staging s(where, st);
    const T *din = (const T *)s.in(lwe_in, ib), *dak = k > 0 ? (const T *)s.in(ak_ntt, kb) : nullptr;
    T *dout = (T *)s.out(glwe_out, ob);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    T *terms = static_cast<T *>(static_cast<void *>(dws));
    T *buf_a = static_cast<T *>(static_cast<void *>(dws + up256(Z.digits)));
    T *buf_b = static_cast<T *>(static_cast<void *>(dws + up256(Z.digits) + up256(Z.buf_a)));
    if (int rc = ring_pack_device<T>(pl, dout, din, dak, m, k, base_log, levels, batch, terms, buf_a, buf_b, st)) return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_RING_API(BITS, T, PLAN)                                                                                                   \
    extern "C" int cntt_prime##BITS##_glwe_embed_batch(const PLAN *pl, T *glwe_out, const T *lwe_in, size_t glwe_dim, size_t batch,          \
                                                       cntt_mem_t where, void *stream) {                                                     \
        return glwe_embed<T>(pl, glwe_out, lwe_in, glwe_dim, batch, where, (hipStream_t)stream);                                             \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_glwe_merge_batch(const PLAN *pl, T *glwe_out, const T *glwe_even, const T *glwe_odd, const T *ak_ntt,  \
                                                       size_t shift, size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,          \
                                                       size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,              \
                                                       void *stream) {                                                                       \
        return glwe_merge<T>(pl, glwe_out, glwe_even, glwe_odd, ak_ntt, shift, t, glwe_dim, base_log, levels, batch, workspace,              \
                             workspace_bytes, where, (hipStream_t)stream);                                                                   \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_glwe_merge_workspace_bytes(const PLAN *pl, size_t glwe_dim, unsigned levels, size_t batch) {        \
        return autoks_workspace_bytes<T>(pl, glwe_dim, levels, batch);                                                                       \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_ring_pack_batch(const PLAN *pl, T *glwe_out, const T *lwe_in, const T *ak_ntt, size_t lwe_count,       \
                                                      size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,    \
                                                      size_t workspace_bytes, cntt_mem_t where, void *stream) {                              \
        return ring_pack<T>(pl, glwe_out, lwe_in, ak_ntt, lwe_count, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where,   \
                            (hipStream_t)stream);                                                                                            \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_ring_pack_workspace_bytes(const PLAN *pl, size_t lwe_count, size_t glwe_dim, unsigned levels,       \
                                                                   size_t batch) {                                                           \
        return ring_pack_workspace_bytes<T>(pl, lwe_count, glwe_dim, levels, batch);                                                         \
    }

CNTT_PRIME_RING_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_RING_API(32, uint32_t, cntt_plan32)

extern "C" unsigned cntt_prime_ring_pack_grid(size_t polys, int logn, size_t word_bytes) { return prime_ring_pack_grid(polys, logn, word_bytes); }
