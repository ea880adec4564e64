// Part of host_prime.hip (included at its end, after host_prime_pack.inc, whose prime_pack_const it uses): the ring automorphism
// X -> X^t of the prime plans, the Galois keyswitch and the trace (include/cntt_prime_automorphism.h) -- the argument checks, the
// workspace layout, the host-slice path and the C ABI over the three kernels of prime_automorphism.hpp (launched by
// prime_automorphism.hip) and external_product_device above, which it calls and does not change.
#include "../../include/cntt_prime_automorphism.h"
#include "prime_automorphism.hpp"

#pragma GCC visibility push(hidden)

// testing switch "autom_lds": stage the polynomial through LDS where it fits (1) or gather from global memory (0)
static bool autom_lds_enabled() { return debug_switch(DBG_AUTOM_LDS) != 0; }

template <class T> static int autom_check_t(const PrimePlan<T> *pl, size_t t) {
    if ((t & 1) == 0 || t >= 2 * pl->n) return fail(CNTT_EINVAL, "t = %zu is not an odd exponent below 2n = %zu", t, 2 * pl->n);
    return CNTT_OK;
}

template <class T>
static int automorphism_device(const PrimePlan<T> *pl, T *out, const T *in, size_t t, bool ntt, size_t polys, hipStream_t st) {
    const hipError_t e = launch_prime_automorphism<T>(out, in, pl->p, (uint32_t)t, ntt, pl->logn, polys, 2 * polys * pl->n * sizeof(T) > STREAM_BYTES,
                                                      autom_lds_enabled(), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_automorphism%s_kernel launch failed: %s", ntt ? "_ntt" : "", hipGetErrorString(e));
    return CNTT_OK;
}

// calls 1 and 2 of the header
template <class T>
static int automorphism(const PrimePlan<T> *pl, T *out, const T *in, size_t t, size_t npolys, size_t batch, bool ntt, cntt_mem_t where,
                        hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = autom_check_t(pl, t)) return rc;
    if ((u128)batch * npolys * pl->n * sizeof(T) >= ((u128)1 << 63))
        return fail(CNTT_EINVAL, "npolys = %zu, batch = %zu: the polynomials pass 2^63 bytes", npolys, batch);
    if (batch == 0 || npolys == 0) return CNTT_OK;
    const char *on = ntt ? "out_ntt" : "out", *in_name = ntt ? "in_ntt" : "in";
    if (!out) return fail(CNTT_EINVAL, "%s is NULL", on);
    if (!in) return fail(CNTT_EINVAL, "%s is NULL", in_name);
    const size_t polys = batch * npolys, bytes = polys * pl->n * sizeof(T);
    const Operand ops[2] = {{on, out, bytes, sizeof(T), true}, {in_name, in, bytes, sizeof(T), false}};
    if (int rc = check_operands(ops, 2)) return rc;
    Staging s(where, st);
    T *dout = (T *)s.out(out, bytes);
    const T *din = (const T *)s.in(in, bytes);
    if (int rc = s.status()) return rc;
    if (int rc = automorphism_device<T>(pl, dout, din, t, ntt, polys, st)) return rc;
    return s.finish();
}

// bytes of the digit polynomials of one Galois keyswitch / of one ciphertext batch
template <class T> static size_t autoks_digit_bytes(const PrimePlan<T> *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return batch * glwe_dim * levels * pl->n * sizeof(T);
}
template <class T> static size_t autoks_workspace_bytes(const PrimePlan<T> *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return pl ? up256(autoks_digit_bytes(pl, glwe_dim, levels, batch)) : 0;
}
template <class T> static size_t trace_workspace_bytes(const PrimePlan<T> *pl, size_t glwe_dim, unsigned levels, size_t batch) {
    return pl ? up256(autoks_digit_bytes(pl, glwe_dim, levels, batch)) + up256(batch * (glwe_dim + 1) * pl->n * sizeof(T)) : 0;
}

// one launch writes the negated digits and the prefilled output; the external product accumulates into the output.  out may not be in.
template <class T>
static int autoks_device(const PrimePlan<T> *pl, T *out, const T *in, const T *ak, size_t t, size_t k, unsigned base_log, unsigned levels,
                         bool add_input, size_t batch, T *terms, hipStream_t st) {
    const hipError_t e = launch_prime_automorphism_gadget<T>(terms, out, in, prime_pack_const(pl, base_log, levels), (uint32_t)t, pl->logn, k, add_input,
                                                             batch, autoks_digit_bytes(pl, k, levels, batch) > STREAM_BYTES, autom_lds_enabled(), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_automorphism_gadget_kernel launch failed: %s", hipGetErrorString(e));
    if (k == 0) return CNTT_OK;
    return external_product_device<T>(pl, out, terms, ak, k * levels, k + 1, batch, true, st);
}

// cur <- cur + AutoKS_{n / 2^r + 1}(cur) for r < steps, ping-pong between out and tmp so that the last step lands in out
template <class T>
static int trace_device(const PrimePlan<T> *pl, T *out, const T *in, const T *ak, unsigned steps, size_t k, unsigned base_log, unsigned levels,
                        size_t batch, T *terms, T *tmp, hipStream_t st) {
    const size_t n = pl->n, key_polys = k * levels * (k + 1);
    if (steps == 0) {
        HIP_TRY(hipMemcpyAsync(out, in, batch * (k + 1) * n * sizeof(T), hipMemcpyDeviceToDevice, st));
        return CNTT_OK;
    }
    const T *src = in;
    for (unsigned r = 0; r < steps; ++r) {
        T *dst = (steps - 1 - r) % 2 == 0 ? out : tmp;
        if (int rc = autoks_device<T>(pl, dst, src, ak ? ak + r * key_polys * n : nullptr, (n >> r) + 1, k, base_log, levels, true, batch, terms, st))
            return rc;
        src = dst;
    }
    return CNTT_OK;
}

// calls 3 (trace = false: one step with exponent t) and 4 (trace = true: `steps` steps) of the header: they share every check
template <class T>
static int glwe_autoks(const PrimePlan<T> *pl, T *glwe_out, const T *glwe_in, const T *ak_ntt, bool trace, size_t t, unsigned steps, size_t k,
                       unsigned base_log, unsigned levels, bool add_input, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                       hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check<PrimePbs<T>>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (trace) {
        if (steps > (unsigned)pl->logn) return fail(CNTT_EINVAL, "steps = %u exceeds log2(ntt_size) = %d", steps, pl->logn);
    } else {
        if (int rc = autom_check_t(pl, t)) return rc;
        steps = 1;
    }
    if (k + 1 >= ((size_t)1 << 32) || k + 1 == 0) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t launch = std::max<size_t>(k * levels, k + 1);   // what external_product_device would refuse halfway through the call
    if ((u128)batch * launch >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "batch * max(glwe_dim * levels, glwe_dim + 1) = %zu * %zu is not below 2^32: too large for one launch", batch, launch);
    // the byte counts -- ciphertexts, digits, key -- are products of the arguments: they must fit before they are formed (the bound above
    // and glwe_dim + 1 < 2^32 keep the 128-bit products themselves from wrapping)
    const u128 lim = (u128)1 << 63, wb = sizeof(T);
    if ((u128)batch * (k + 1) * pl->n * wb >= lim || (u128)batch * k * levels * pl->n * wb >= lim ||
        (u128)steps * k * levels * (k + 1) * pl->n * wb >= lim)
        return fail(CNTT_EINVAL, "glwe_dim = %zu, levels = %u, batch = %zu: the ciphertexts, the digits or the key pass 2^63 bytes", k, levels, batch);
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!glwe_in) return fail(CNTT_EINVAL, "glwe_in is NULL");
    const bool keyed = k > 0 && steps > 0;
    if (keyed && !ak_ntt) return fail(CNTT_EINVAL, "ak_ntt is NULL");
    const size_t n = pl->n, cb = batch * (k + 1) * n * sizeof(T), kb = keyed ? steps * k * levels * (k + 1) * n * sizeof(T) : 0;
    const size_t digits = up256(autoks_digit_bytes(pl, k, levels, batch));
    const size_t need = trace ? trace_workspace_bytes(pl, k, levels, batch) : digits;
    if (workspace)
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
    const Operand ops[4] = {{"glwe_out", glwe_out, cb, sizeof(T), true},
                            {"glwe_in", glwe_in, cb, sizeof(T), false},
                            {"ak_ntt", ak_ntt, kb, sizeof(T), false},
                            {"workspace", workspace, workspace ? workspace_bytes : 0, 16, true}};
    if (int rc = check_operands(ops, 4)) return rc;
    Staging s(where, st);
    const T *din = (const T *)s.in(glwe_in, cb), *dak = keyed ? (const T *)s.in(ak_ntt, kb) : nullptr;
    T *dout = (T *)s.out(glwe_out, cb);
    // what the call touches of the workspace: nothing without a step, the digits with a key, the second ciphertext from two steps on
    char *dws = (char *)s.workspace(workspace, need, steps > 0 && (k > 0 || (trace && steps > 1)));   // one block for the whole call
    if (int rc = s.status()) return rc;
    T *terms = static_cast<T *>(static_cast<void *>(dws)), *tmp = dws ? static_cast<T *>(static_cast<void *>(dws + digits)) : nullptr;
    if (int rc = trace ? trace_device<T>(pl, dout, din, dak, steps, k, base_log, levels, batch, terms, tmp, st)
                       : autoks_device<T>(pl, dout, din, dak, t, k, base_log, levels, add_input, batch, terms, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_AUTOM_API(BITS, T, PLAN)                                                                                                  \
    extern "C" int cntt_prime##BITS##_automorphism_batch(const PLAN *pl, T *out, const T *in, size_t t, size_t npolys, size_t batch,         \
                                                         cntt_mem_t where, void *stream) {                                                   \
        return automorphism<T>(pl, out, in, t, npolys, batch, false, where, (hipStream_t)stream);                                            \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_automorphism_ntt_batch(const PLAN *pl, T *out_ntt, const T *in_ntt, size_t t, size_t npolys,           \
                                                             size_t batch, cntt_mem_t where, void *stream) {                                 \
        return automorphism<T>(pl, out_ntt, in_ntt, t, npolys, batch, true, where, (hipStream_t)stream);                                     \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_glwe_automorphism_keyswitch_batch(const PLAN *pl, T *glwe_out, const T *glwe_in, const T *ak_ntt,      \
                                                                        size_t t, size_t glwe_dim, unsigned base_log, unsigned levels,       \
                                                                        int add_input, size_t batch, void *workspace,                        \
                                                                        size_t workspace_bytes, cntt_mem_t where, void *stream) {            \
        return glwe_autoks<T>(pl, glwe_out, glwe_in, ak_ntt, false, t, 0, glwe_dim, base_log, levels, add_input != 0, batch, workspace,      \
                              workspace_bytes, where, (hipStream_t)stream);                                                                  \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_glwe_automorphism_keyswitch_workspace_bytes(const PLAN *pl, size_t glwe_dim, unsigned levels,       \
                                                                                     size_t batch) {                                         \
        return autoks_workspace_bytes<T>(pl, glwe_dim, levels, batch);                                                                       \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_glwe_trace_batch(const PLAN *pl, T *glwe_out, const T *glwe_in, const T *ak_ntt, unsigned steps,       \
                                                       size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,   \
                                                       size_t workspace_bytes, cntt_mem_t where, void *stream) {                             \
        return glwe_autoks<T>(pl, glwe_out, glwe_in, ak_ntt, true, 1, steps, glwe_dim, base_log, levels, true, batch, workspace,             \
                              workspace_bytes, where, (hipStream_t)stream);                                                                  \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_glwe_trace_workspace_bytes(const PLAN *pl, size_t glwe_dim, unsigned levels, size_t batch) {        \
        return trace_workspace_bytes<T>(pl, glwe_dim, levels, batch);                                                                        \
    }

CNTT_PRIME_AUTOM_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_AUTOM_API(32, uint32_t, cntt_plan32)

extern "C" unsigned cntt_prime_automorphism_grid(size_t polys, int logn, size_t word_bytes) {
    return prime_automorphism_grid(polys, logn, word_bytes);
}
