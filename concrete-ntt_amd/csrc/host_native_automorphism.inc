// Part of host_native_ext.hip (included at its end, after host_native_cbs.inc): the ring automorphism X -> X^t of the native plans, the
// Galois keyswitch and the trace (include/cntt_automorphism.h) -- the argument checks, the workspace layout, the host-slice path and the
// C ABI over the three kernels of native_automorphism.hpp (launched by native_automorphism.hip), gadget_check and the family's external
// product (native_ext_device), which it calls and does not change.  Templates over a plan family F in the style of host_native_cmux.inc:
// F is NativePbs plus the one launcher below.  The term bound is this call's own line, not F::check_terms: that one counts
// (glwe_dim + 1) * levels terms and says so in its message, and a Galois keyswitch sums glwe_dim * levels.
#include "../../include/cntt_automorphism.h"
#include "native_automorphism.hpp"

#pragma GCC visibility push(hidden)

// testing switch "autom_lds": stage the polynomial through LDS where it fits (1) or gather from global memory (0)
static bool native_autom_lds_enabled() { return debug_switch(DBG_AUTOM_LDS) != 0; }

struct NativeAutom : NativePbs {
    static hipError_t launch_autom_gadget(const cntt_native *pl, void *terms, void *out, const void *in, unsigned base_log, unsigned levels,
                                          size_t t, size_t glwe_dim, bool add_input, size_t batch, bool stream, hipStream_t st) {
        const u128 off = gadget_offset(digit_bits(pl), base_log, levels);
        return launch_native_automorphism_gadget(pl->info.word, terms, out, in, (uint64_t)off, (uint64_t)(off >> 64), base_log, levels,
                                                 (uint32_t)t, native_logn(pl), glwe_dim, add_input, batch, stream, native_autom_lds_enabled(), st);
    }
};

static int native_autom_check_t(const cntt_native *pl, size_t t) {
    if ((t & 1) == 0 || t >= 2 * pl->n) return fail(CNTT_EINVAL, "t = %zu is not an odd exponent below 2n = %zu", t, 2 * pl->n);
    return CNTT_OK;
}

// call 1 of the header
static int native_automorphism(const cntt_native *pl, void *out, const void *in, size_t t, size_t npolys, size_t batch, cntt_mem_t where,
                               hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = native_autom_check_t(pl, t)) return rc;
    const size_t w = (size_t)pl->info.word;
    if (product_passes_2_63({batch, npolys, pl->n, w}))
        return fail(CNTT_EINVAL, "npolys = %zu, batch = %zu: the polynomials pass 2^63 bytes", npolys, batch);
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (!out) return fail(CNTT_EINVAL, "out is NULL");
    if (!in) return fail(CNTT_EINVAL, "in is NULL");
    const size_t polys = batch * npolys, bytes = polys * pl->n * w;
    const Operand ops[2] = {{"out", out, bytes, w, true}, {"in", in, bytes, w, false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    void *dout = s.out(out, bytes);
    const void *din = s.in(in, bytes);
    if (int rc = s.status()) return rc;
    const hipError_t e = launch_native_automorphism(pl->info.word, dout, din, (uint32_t)t, false, native_logn(pl), polys, 2 * bytes > STREAM_BYTES,
                                                    native_autom_lds_enabled(), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_automorphism_kernel launch failed: %s", hipGetErrorString(e));
    return s.finish();
}

static const char *const AUTOM_OUT_PLANE[10] = {"out_planes[0]", "out_planes[1]", "out_planes[2]", "out_planes[3]", "out_planes[4]",
                                                "out_planes[5]", "out_planes[6]", "out_planes[7]", "out_planes[8]", "out_planes[9]"};
static const char *const AUTOM_IN_PLANE[10] = {"in_planes[0]", "in_planes[1]", "in_planes[2]", "in_planes[3]", "in_planes[4]",
                                               "in_planes[5]", "in_planes[6]", "in_planes[7]", "in_planes[8]", "in_planes[9]"};
static const char *const AUTOM_KEY_PLANE[10] = {"ak_ntt[0]", "ak_ntt[1]", "ak_ntt[2]", "ak_ntt[3]", "ak_ntt[4]",
                                                "ak_ntt[5]", "ak_ntt[6]", "ak_ntt[7]", "ak_ntt[8]", "ak_ntt[9]"};

// call 2 of the header: one launch per residue plane
static int native_automorphism_ntt(const cntt_native *pl, void *const *out_planes, const void *const *in_planes, size_t t, size_t npolys,
                                   size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = native_autom_check_t(pl, t)) return rc;
    const size_t rb = pl->rbytes();
    const int np = pl->info.nprimes;
    if (product_passes_2_63({batch, npolys, pl->n, rb}))
        return fail(CNTT_EINVAL, "npolys = %zu, batch = %zu: the residue polynomials pass 2^63 bytes", npolys, batch);
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (!out_planes) return fail(CNTT_EINVAL, "out_planes is NULL");
    if (!in_planes) return fail(CNTT_EINVAL, "in_planes is NULL");
    const size_t polys = batch * npolys, bytes = polys * pl->n * rb;
    Operand ops[20];
    for (int i = 0; i < np; ++i) {
        if (!out_planes[i]) return fail(CNTT_EINVAL, "NULL residue plane (out_planes[%d])", i);
        if (!in_planes[i]) return fail(CNTT_EINVAL, "NULL residue plane (in_planes[%d])", i);
        ops[i] = {AUTOM_OUT_PLANE[i], out_planes[i], bytes, rb, true};
        ops[np + i] = {AUTOM_IN_PLANE[i], in_planes[i], bytes, rb, false};
    }
    if (int rc = check_operands(ops, 2 * np)) return rc;
    Staging s(where, st);
    void *dout[10];
    const void *din[10];
    for (int i = 0; i < np; ++i) {
        dout[i] = s.out(out_planes[i], bytes);
        din[i] = s.in(in_planes[i], bytes);
    }
    if (int rc = s.status()) return rc;
    for (int i = 0; i < np; ++i) {
        const hipError_t e = launch_native_automorphism((int)rb, dout[i], din[i], (uint32_t)t, true, native_logn(pl), polys, 2 * bytes > STREAM_BYTES,
                                                        native_autom_lds_enabled(), st);
        if (e != hipSuccess) return fail(CNTT_EDEVICE, "native_automorphism_ntt_kernel launch failed: %s", hipGetErrorString(e));
    }
    return s.finish();
}

// bytes of the digit polynomials of one Galois keyswitch
template <class F> static size_t autoks_digit_bytes(const typename F::Plan *pl, size_t k, unsigned levels, size_t batch) {
    return batch * k * levels * pl->n * F::word(pl);
}
template <class F> static size_t autoks_workspace_bytes(const typename F::Plan *pl, size_t k, unsigned levels, size_t batch) {
    return pl ? up256(autoks_digit_bytes<F>(pl, k, levels, batch)) : 0;
}
template <class F> static size_t trace_workspace_bytes(const typename F::Plan *pl, size_t k, unsigned levels, size_t batch) {
    return pl ? up256(autoks_digit_bytes<F>(pl, k, levels, batch)) + up256(batch * (k + 1) * pl->n * F::word(pl)) : 0;
}

// one launch writes the negated digits and the prefilled output; the external product accumulates into the output.  out may not be in.
template <class F>
static int autoks_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *in, typename F::Key ak, size_t t, size_t k,
                         unsigned base_log, unsigned levels, bool add_input, size_t batch, typename F::Word *terms, hipStream_t st) {
    const hipError_t e = F::launch_autom_gadget(pl, terms, out, in, base_log, levels, t, k, add_input, batch,
                                                autoks_digit_bytes<F>(pl, k, levels, batch) > STREAM_BYTES, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_automorphism_gadget_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    if (k == 0) return CNTT_OK;
    return F::ext_product(pl, out, terms, ak, k * levels, k + 1, batch, true, st);
}

// cur <- cur + AutoKS_{n / 2^r + 1}(cur) for r < steps, alternating between out and tmp so that the last step lands in out
template <class F>
static int trace_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *in, typename F::Key ak, unsigned steps, size_t k,
                        unsigned base_log, unsigned levels, size_t batch, typename F::Word *terms, typename F::Word *tmp, hipStream_t st) {
    const size_t n = pl->n, slice = F::key_bytes(pl, k * levels * (k + 1));   // one key
    if (steps == 0) {
        HIP_TRY(hipMemcpyAsync(out, in, batch * (k + 1) * n * F::word(pl), hipMemcpyDeviceToDevice, st));
        return CNTT_OK;
    }
    const typename F::Word *src = in;
    typename F::KeyStore ks;
    for (unsigned r = 0; r < steps; ++r) {
        typename F::Word *dst = (steps - 1 - r) % 2 == 0 ? out : tmp;
        const typename F::Key key = k ? F::key_at(pl, ak, (size_t)r * slice, ks) : typename F::Key{};
        if (int rc = autoks_device<F>(pl, dst, src, key, (n >> r) + 1, k, base_log, levels, true, batch, terms, st)) return rc;
        src = dst;
    }
    return CNTT_OK;
}

// calls 3 (trace = false: one step with exponent t) and 4 (trace = true: `steps` steps) of the header: they share every check
template <class F>
static int glwe_autoks(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *glwe_in, typename F::Key ak_ntt, bool trace,
                       size_t t, unsigned steps, size_t k, unsigned base_log, unsigned levels, bool add_input, size_t batch, void *workspace,
                       size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (pl->info.binary)
        return fail(CNTT_EINVAL, "plan is of a native_binary kind: a keyswitching key has full-width words, and the exactness of these kinds rests on "
                                 "a 0 / 1 key");
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    const int logn = F::logn(pl);
    if (trace) {
        if (steps > (unsigned)logn) return fail(CNTT_EINVAL, "steps = %u exceeds log2(ntt_size) = %d", steps, logn);
    } else {
        if (int rc = native_autom_check_t(pl, t)) return rc;
        steps = 1;
    }
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (k * levels > pl->max_terms)   // (k < 2^32 and levels <= 128: the product does not wrap)
        return fail(CNTT_EINVAL, "glwe_dim * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range",
                    k * levels, pl->max_terms);
    const size_t launch = std::max<size_t>(k * levels, k + 1);   // what the external product would refuse halfway through the call
    if ((u128)batch * launch >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * max(glwe_dim * levels, glwe_dim + 1) = %zu * %zu is not below 2^32: too large for one launch", batch, launch);
    // the byte counts -- ciphertexts, digits, key -- are products of the arguments: they must fit before they are formed
    const size_t n = pl->n, w = F::word(pl);
    if (product_passes_2_63({batch, k + 1, n, w}) || product_passes_2_63({batch, k, levels, n, w}) ||
        product_passes_2_63({(size_t)steps, k, levels, k + 1, n, w}))
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the key pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!glwe_in) return fail(CNTT_EINVAL, "glwe_in is NULL");
    const bool keyed = k > 0 && steps > 0;
    if (keyed)
        if (int rc = F::key_check(pl, ak_ntt, "ak_ntt")) return rc;
    const size_t cb = batch * (k + 1) * n * w, kb = keyed ? F::key_bytes(pl, (size_t)steps * k * levels * (k + 1)) : 0;
    const size_t digits = up256(autoks_digit_bytes<F>(pl, k, levels, batch));
    const size_t need = trace ? trace_workspace_bytes<F>(pl, k, levels, batch) : digits;
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    Operand ops[13] = {{"glwe_out", glwe_out, cb, w, true}, {"glwe_in", glwe_in, cb, w, false}};
    int cnt = 2;
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {AUTOM_KEY_PLANE[i], ak_ntt[i], kb, pl->rbytes(), false};
    ops[cnt++] = {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true};
    if (int rc = check_operands(ops, cnt)) return rc;
    Staging s(where, st);
    typename F::KeyStore ks;
    const W *din = (const W *)s.in(glwe_in, cb);
    const typename F::Key dak = keyed ? F::key_in(pl, s, ak_ntt, kb, ks) : typename F::Key{};
    W *dout = (W *)s.out(glwe_out, cb);
    // what the call touches of the workspace: nothing without a step, the digits with a key, the second ciphertext from two steps on
    char *dws = (char *)s.workspace(workspace, need, steps > 0 && (k > 0 || (trace && steps > 1)));   // one block for the whole call
    if (int rc = s.status()) return rc;
    W *terms = static_cast<W *>(static_cast<void *>(dws)), *tmp = dws ? static_cast<W *>(static_cast<void *>(dws + digits)) : nullptr;
    if (int rc = trace ? trace_device<F>(pl, dout, din, dak, steps, k, base_log, levels, batch, terms, tmp, st)
                       : autoks_device<F>(pl, dout, din, dak, t, k, base_log, levels, add_input, batch, terms, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_automorphism_batch(const cntt_native_t *pl, void *out, const void *in, size_t t, size_t npolys, size_t batch,
                                              cntt_mem_t where, void *stream) {
    return native_automorphism(pl, out, in, t, npolys, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_automorphism_ntt_batch(const cntt_native_t *pl, void *const *out_planes, const void *const *in_planes, size_t t,
                                                  size_t npolys, size_t batch, cntt_mem_t where, void *stream) {
    return native_automorphism_ntt(pl, out_planes, in_planes, t, npolys, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_glwe_automorphism_keyswitch_batch(const cntt_native_t *pl, void *glwe_out, const void *glwe_in,
                                                             const void *const *ak_ntt, size_t t, size_t glwe_dim, unsigned base_log,
                                                             unsigned levels, int add_input, size_t batch, void *workspace,
                                                             size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return glwe_autoks<NativeAutom>(pl, glwe_out, glwe_in, ak_ntt, false, t, 0, glwe_dim, base_log, levels, add_input != 0, batch, workspace,
                                    workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_glwe_automorphism_keyswitch_workspace_bytes(const cntt_native_t *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return autoks_workspace_bytes<NativeAutom>(pl, glwe_dim, levels, batch);
}
extern "C" int cntt_native_glwe_trace_batch(const cntt_native_t *pl, void *glwe_out, const void *glwe_in, const void *const *ak_ntt, unsigned steps,
                                            size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                                            size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return glwe_autoks<NativeAutom>(pl, glwe_out, glwe_in, ak_ntt, true, 1, steps, glwe_dim, base_log, levels, true, batch, workspace,
                                    workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_glwe_trace_workspace_bytes(const cntt_native_t *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return trace_workspace_bytes<NativeAutom>(pl, glwe_dim, levels, batch);
}
extern "C" unsigned cntt_native_automorphism_grid(size_t polys, int logn, size_t word_bytes) {
    return native_automorphism_grid(polys, logn, word_bytes);
}
