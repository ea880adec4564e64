// Part of host_prime.hip (included at its end; kept apart so that file stays readable): the C ABI of the prime plans' programmable
// bootstrap (include/cntt_prime_pbs.h) -- argument checks, the host-slice staging and the blind rotation loop over prime_gadget_kernel
// (prime_pbs.hpp; launched by prime_pbs.hip) and external_product_device above, which it calls and does not change.
#include "../../include/cntt_prime_pbs.h"
#include "prime_pbs.hpp"

#pragma GCC visibility push(hidden)

static bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return abytes && bbytes && x < y + bbytes && y < x + abytes;
}
// W of the header: the bit length of p
template <class T> static unsigned modulus_bits(const PrimePlan<T> *pl) {
    unsigned w = 0;
    while (w < PrimePlan<T>::B && ((uint64_t)pl->p >> w) != 0) ++w;
    return w;
}
// the checks every call with digits shares
template <class T> static int gadget_check(const PrimePlan<T> *pl, unsigned base_log, unsigned levels, int mode, const uint32_t *rot) {
    const unsigned wbits = modulus_bits(pl);
    if (base_log == 0) return fail(CNTT_EINVAL, "base_log is 0");
    if (levels == 0) return fail(CNTT_EINVAL, "levels is 0");
    if ((uint64_t)base_log * levels > wbits)
        return fail(CNTT_EINVAL, "base_log * levels = %u * %u exceeds the bit length %u of the modulus", base_log, levels, wbits);
    if (mode != CNTT_SRC_PLAIN && mode != CNTT_SRC_ROTATE && mode != CNTT_SRC_CMUX) return fail(CNTT_EINVAL, "src_mode %d is not a cntt_src_mode_t", mode);
    if (mode != CNTT_SRC_PLAIN && !rot) return fail(CNTT_EINVAL, "rot is NULL and src_mode reads it");
    return CNTT_OK;
}
// host path: the rotation exponents are in reach, so one that is not below 2n is an error there (`name`: the argument in the message)
template <class T> static int check_rot_host(const PrimePlan<T> *pl, const uint32_t *rot, size_t count, const char *name) {
    for (size_t i = 0; i < count; ++i)
        if ((size_t)rot[i] >= 2 * pl->n) return fail(CNTT_EINVAL, "%s[%zu] = %u is not below 2n = %zu", name, i, rot[i], 2 * pl->n);
    return CNTT_OK;
}

// the constants of prime_pbs.hpp: off = 2^(s-1) + K' 2^s with K' = sum_{l >= 2} (B/2) B^(levels-l), and what the two digit forms need
template <class T> static PrimeGadgetConst<T> gadget_const(const PrimePlan<T> *pl, size_t npolys, unsigned base_log, unsigned levels, int mode) {
    constexpr unsigned TB = sizeof(T) * 8;
    const unsigned wbits = modulus_bits(pl), s = wbits - base_log * levels, sh1 = wbits - base_log;
    u128 off = s ? (u128)1 << (s - 1) : 0;
    for (unsigned l = 2; l <= levels; ++l) off += (u128)1 << (wbits - base_log * l + base_log - 1);   // (B/2) B^(levels-l) 2^s
    PrimeGadgetConst<T> G{};
    G.p = pl->p;
    G.hp = (T)((pl->p - 1) / 2);
    G.off = (T)off;   // < 2^(W-1) < p
    G.thr = (T)(pl->p - G.off);
    G.mask = base_log >= TB ? (T)~(T)0 : (T)((((T)1) << base_log) - 1);
    G.half = (T)((T)1 << (base_log - 1));
    G.pmh = (T)(pl->p - G.half);   // used by the levels below the top only: base_log <= W / 2 there
    G.topsub = sh1 ? (T)((T)1 << (TB - sh1)) : (T)0;
    G.sh1 = sh1;
    G.base_log = base_log;
    G.levels = levels;
    G.npolys = (uint32_t)npolys;
    G.rotated = mode != CNTT_SRC_PLAIN;
    G.cmux = mode == CNTT_SRC_CMUX;
    return G;
}

template <class T>
static int gadget_device(const PrimePlan<T> *pl, T *terms, const T *polys, const uint32_t *rot, size_t npolys, unsigned base_log, unsigned levels,
                         int mode, size_t batch, hipStream_t st) {
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (npolys >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "npolys too large");
    const PrimeGadgetConst<T> G = gadget_const(pl, npolys, base_log, levels, mode);
    const size_t total = batch * npolys;
    // the terms against STREAM_BYTES, as the pointwise kernels decide it: larger ones pass through once (non-temporal stores)
    const hipError_t e = launch_prime_gadget<T>(terms, polys, rot, G, pl->logn, total, total * levels * pl->n * sizeof(T) > STREAM_BYTES,
                                                ew_grid(total * pl->n * sizeof(T) / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_gadget_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}

template <class T>
static int gadget_decompose(const PrimePlan<T> *pl, T *terms, const T *polys, const uint32_t *rot, size_t npolys, unsigned base_log,
                            unsigned levels, int mode, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check(pl, base_log, levels, mode, rot)) return rc;
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (!terms || !polys) return fail(CNTT_EINVAL, "NULL argument");
    const size_t pb = batch * npolys * pl->n * sizeof(T), tb = pb * levels;
    if (ranges_overlap(terms, tb, polys, pb)) return fail(CNTT_EINVAL, "terms overlaps polys");
    if (where == CNTT_MEM_DEVICE) return gadget_device<T>(pl, terms, polys, rot, npolys, base_log, levels, mode, batch, st);
    const bool rotated = mode != CNTT_SRC_PLAIN;
    if (rotated)
        if (int rc = check_rot_host(pl, rot, batch, "rot")) return rc;
    Staging s(st);
    T *dt = (T *)s.out(terms, tb);
    const T *dp = (const T *)s.in(polys, pb);
    const uint32_t *dr = rotated ? (const uint32_t *)s.in(rot, batch * sizeof(uint32_t)) : nullptr;
    if (int rc = s.status()) return rc;
    if (int rc = gadget_device<T>(pl, dt, dp, dr, npolys, base_log, levels, mode, batch, st)) return rc;
    return s.finish();
}

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// the three parts of the workspace, in bytes and in this order (cntt_prime_pbs.h states the formula)
struct PbsSizes {
    size_t digits, rot, acc;
    size_t total() const { return up256(digits) + up256(rot) + up256(acc); }
};
template <class T> static PbsSizes pbs_sizes(const PrimePlan<T> *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    const size_t pb = batch * (glwe_dim + 1) * pl->n * sizeof(T);
    return PbsSizes{pb * levels, (lwe_dim + 1) * batch * sizeof(uint32_t), pb};
}

template <class T> static int modswitch_device(const PrimePlan<T> *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch, hipStream_t st) {
    if (pl->logn > 29) return fail(CNTT_EINVAL, "ntt_size too large for the modulus switch");   // floor(x 4n / p) in 32 bits
    const size_t tiles = ((lwe_dim + PRIME_PBS_TILE) / PRIME_PBS_TILE) * ((batch + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE);
    const hipError_t e = launch_prime_lwe_modswitch<T>(rot_t, lwe, pl->p, pl->logn, lwe_dim, batch, ew_grid(tiles * 256), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_lwe_modswitch_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}
template <class T>
static int extract_device(const PrimePlan<T> *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t index, size_t batch, hipStream_t st) {
    const hipError_t e = launch_prime_sample_extract<T>(lwe_out, glwe, pl->p, pl->logn, glwe_dim, (uint32_t)index, batch,
                                                        ew_grid(batch * (glwe_dim * pl->n + 1)), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_sample_extract_kernel launch failed: %s", hipGetErrorString(e));
    return CNTT_OK;
}
// acc = X^(body row of rot_t) lut, then lwe_dim times decomposition (CMux difference) into `digits` and the fused chain accumulating into
// acc.  In place is sound: the digits are complete before the product starts (stream order), and the product reads only the digits and
// the key besides the output words it adds to.
template <class T>
static int blind_rotate_device(const PrimePlan<T> *pl, T *acc, const T *lut, bool lut_per_element, const uint32_t *rot_t, const T *bsk,
                               size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, T *digits, hipStream_t st) {
    const size_t npolys = glwe_dim + 1, nterms = npolys * levels, n = pl->n;
    const size_t slice = nterms * npolys * n;   // one iteration's key, words
    const hipError_t e = launch_prime_pbs_init<T>(acc, lut, rot_t + lwe_dim * batch, pl->p, pl->logn, (uint32_t)npolys, lut_per_element, batch,
                                                  batch * npolys * n * sizeof(T) > STREAM_BYTES, ew_grid(batch * npolys * n * sizeof(T) / 16), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "prime_pbs_init_kernel launch failed: %s", hipGetErrorString(e));
    for (size_t i = 0; i < lwe_dim; ++i) {
        if (int rc = gadget_device<T>(pl, digits, acc, rot_t + i * batch, npolys, base_log, levels, CNTT_SRC_CMUX, batch, st)) return rc;
        if (int rc = external_product_device<T>(pl, acc, digits, bsk + i * slice, nterms, npolys, batch, true, st)) return rc;
    }
    return CNTT_OK;
}

template <class T>
static int lwe_modswitch(const PrimePlan<T> *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch == 0) return CNTT_OK;
    if (!rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    if (!lwe) return fail(CNTT_EINVAL, "lwe is NULL");
    const size_t rb = (lwe_dim + 1) * batch * sizeof(uint32_t), lb = (lwe_dim + 1) * batch * sizeof(T);
    if (ranges_overlap(rot_t, rb, lwe, lb)) return fail(CNTT_EINVAL, "rot_t overlaps lwe");
    if (where == CNTT_MEM_DEVICE) return modswitch_device<T>(pl, rot_t, lwe, lwe_dim, batch, st);
    Staging s(st);
    uint32_t *dr = (uint32_t *)s.out(rot_t, rb);
    const T *dl = (const T *)s.in(lwe, lb);
    if (int rc = s.status()) return rc;
    if (int rc = modswitch_device<T>(pl, dr, dl, lwe_dim, batch, st)) return rc;
    return s.finish();
}

template <class T>
static int sample_extract(const PrimePlan<T> *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t index, size_t batch, cntt_mem_t where,
                          hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (index >= pl->n) return fail(CNTT_EINVAL, "index = %zu is not below ntt_size = %zu", index, pl->n);
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!glwe) return fail(CNTT_EINVAL, "glwe is NULL");
    const size_t ob = batch * (glwe_dim * pl->n + 1) * sizeof(T), gb = batch * (glwe_dim + 1) * pl->n * sizeof(T);
    if (ranges_overlap(lwe_out, ob, glwe, gb)) return fail(CNTT_EINVAL, "lwe_out overlaps glwe");
    if (where == CNTT_MEM_DEVICE) return extract_device<T>(pl, lwe_out, glwe, glwe_dim, index, batch, st);
    Staging s(st);
    T *dout = (T *)s.out(lwe_out, ob);
    const T *dg = (const T *)s.in(glwe, gb);
    if (int rc = s.status()) return rc;
    if (int rc = extract_device<T>(pl, dout, dg, glwe_dim, index, batch, st)) return rc;
    return s.finish();
}

// the argument checks blind_rotate and bootstrap share; `need` = what the workspace must hold
template <class T>
static int pbs_check(const PrimePlan<T> *pl, const T *bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch,
                     const void *workspace, size_t workspace_bytes, size_t need) {
    const uint32_t some_rot = 0;
    if (int rc = gadget_check(pl, base_log, levels, CNTT_SRC_CMUX, &some_rot)) return rc;
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (batch == 0) return CNTT_OK;
    if (lwe_dim && !bsk) return fail(CNTT_EINVAL, "bsk_ntt is NULL");
    if (workspace) {
        if ((uintptr_t)workspace % 16) return fail(CNTT_EINVAL, "workspace is not 16-byte aligned");
        if (workspace_bytes < need) return fail(CNTT_EINVAL, "workspace_bytes = %zu is below the %zu bytes this call needs", workspace_bytes, need);
    }
    return CNTT_OK;
}

template <class T>
static int blind_rotate(const PrimePlan<T> *pl, T *acc, const T *lut, int lut_per_element, const uint32_t *rot_t, const T *bsk, size_t lwe_dim,
                        size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                        cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch && !rot_t) return fail(CNTT_EINVAL, "rot_t is NULL");
    const PbsSizes Z = pbs_sizes(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = pbs_check(pl, bsk, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, Z.digits)) return rc;
    if (batch == 0) return CNTT_OK;
    if (!acc) return fail(CNTT_EINVAL, "acc is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch;
    if (ranges_overlap(acc, Z.acc, lut, lb)) return fail(CNTT_EINVAL, "acc overlaps lut");
    if (ranges_overlap(acc, Z.acc, rot_t, Z.rot)) return fail(CNTT_EINVAL, "acc overlaps rot_t");
    if (workspace && ranges_overlap(acc, Z.acc, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "acc overlaps workspace");
    if (where == CNTT_MEM_DEVICE) {
        void *digits = workspace;
        if (!digits && lwe_dim) HIP_TRY(hipMallocAsync(&digits, Z.digits, st));   // one allocation for the whole loop
        const int rc = blind_rotate_device<T>(pl, acc, lut, lut_per_element != 0, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, batch,
                                              (T *)digits, st);
        if (!workspace && digits) (void)hipFreeAsync(digits, st);
        return rc;
    }
    if (int rc = check_rot_host(pl, rot_t, (lwe_dim + 1) * batch, "rot_t")) return rc;
    const size_t kb = lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1) * pl->n * sizeof(T);
    Staging s(st);
    const T *dkey = lwe_dim ? (const T *)s.in(bsk, kb) : nullptr;
    const T *dlut = (const T *)s.in(lut, lb);
    const uint32_t *drot = (const uint32_t *)s.in(rot_t, Z.rot);
    T *dacc = (T *)s.out(acc, Z.acc), *ddig = (T *)s.alloc(Z.digits);
    if (int rc = s.status()) return rc;
    if (int rc = blind_rotate_device<T>(pl, dacc, dlut, lut_per_element != 0, drot, dkey, lwe_dim, glwe_dim, base_log, levels, batch, ddig, st))
        return rc;
    return s.finish();
}

// modulus switch -> blind rotation -> extraction of coefficient 0 on device buffers; ws holds digits | rot_t | acc (PbsSizes)
template <class T>
static int bootstrap_device(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *lut, bool lut_per_element, const T *bsk, size_t lwe_dim,
                            size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, const PbsSizes &Z, char *ws, hipStream_t st) {
    uint32_t *rot_t = reinterpret_cast<uint32_t *>(ws + up256(Z.digits));
    T *acc = reinterpret_cast<T *>(ws + up256(Z.digits) + up256(Z.rot));
    if (int rc = modswitch_device<T>(pl, rot_t, lwe_in, lwe_dim, batch, st)) return rc;
    if (int rc = blind_rotate_device<T>(pl, acc, lut, lut_per_element, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, batch,
                                        reinterpret_cast<T *>(ws), st))
        return rc;
    return extract_device<T>(pl, lwe_out, acc, glwe_dim, 0, batch, st);
}

template <class T>
static int bootstrap(const PrimePlan<T> *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element, const T *bsk, size_t lwe_dim,
                     size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,
                     hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    const PbsSizes Z = pbs_sizes(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = pbs_check(pl, bsk, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, Z.total())) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    const size_t ob = batch * (glwe_dim * pl->n + 1) * sizeof(T), ib = batch * (lwe_dim + 1) * sizeof(T);
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch;
    if (ranges_overlap(lwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "lwe_out overlaps lwe_in");
    if (ranges_overlap(lwe_out, ob, lut, lb)) return fail(CNTT_EINVAL, "lwe_out overlaps lut");
    if (workspace) {
        if (ranges_overlap(lwe_out, ob, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_out overlaps workspace");
        if (ranges_overlap(lwe_in, ib, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_in overlaps workspace");
        if (ranges_overlap(lut, lb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lut overlaps workspace");
    }
    if (where == CNTT_MEM_DEVICE) {
        void *ws = workspace;
        if (!ws) HIP_TRY(hipMallocAsync(&ws, Z.total(), st));   // one allocation for the whole call
        const int rc = bootstrap_device<T>(pl, lwe_out, lwe_in, lut, lut_per_element != 0, bsk, lwe_dim, glwe_dim, base_log, levels, batch, Z,
                                           static_cast<char *>(ws), st);
        if (!workspace) (void)hipFreeAsync(ws, st);
        return rc;
    }
    const size_t kb = lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1) * pl->n * sizeof(T);
    Staging s(st);
    const T *dkey = lwe_dim ? (const T *)s.in(bsk, kb) : nullptr;
    const T *din = (const T *)s.in(lwe_in, ib), *dlut = (const T *)s.in(lut, lb);
    T *dout = (T *)s.out(lwe_out, ob);
    char *dws = (char *)s.alloc(Z.total());
    if (int rc = s.status()) return rc;
    if (int rc = bootstrap_device<T>(pl, dout, din, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels, batch, Z, dws, st))
        return rc;
    return s.finish();
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_PBS_API(BITS, T, PLAN)                                                                                                    \
    extern "C" int cntt_prime##BITS##_gadget_decompose_batch(const PLAN *pl, T *terms, const T *polys, const uint32_t *rot, size_t npolys,    \
                                                             unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t batch,     \
                                                             cntt_mem_t where, void *stream) {                                               \
        return gadget_decompose<T>(pl, terms, polys, rot, npolys, base_log, levels, (int)src_mode, batch, where, (hipStream_t)stream);       \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_lwe_modswitch_batch(const PLAN *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch,        \
                                                          cntt_mem_t where, void *stream) {                                                  \
        return lwe_modswitch<T>(pl, rot_t, lwe, lwe_dim, batch, where, (hipStream_t)stream);                                                 \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_blind_rotate_batch(const PLAN *pl, T *acc, const T *lut, int lut_per_element, const uint32_t *rot_t,    \
                                                         const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,               \
                                                         unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,             \
                                                         cntt_mem_t where, void *stream) {                                                   \
        return blind_rotate<T>(pl, acc, lut, lut_per_element, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace,         \
                               workspace_bytes, where, (hipStream_t)stream);                                                                 \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_sample_extract_batch(const PLAN *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t index,          \
                                                           size_t batch, cntt_mem_t where, void *stream) {                                   \
        return sample_extract<T>(pl, lwe_out, glwe, glwe_dim, index, batch, where, (hipStream_t)stream);                                     \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_bootstrap_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element,         \
                                                      const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, \
                                                      size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,               \
                                                      void *stream) {                                                                        \
        return bootstrap<T>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace,       \
                            workspace_bytes, where, (hipStream_t)stream);                                                                    \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,                \
                                                             size_t batch) {                                                                 \
        return pl ? pbs_sizes<T>(pl, lwe_dim, glwe_dim, levels, batch).total() : 0;                                                          \
    }

CNTT_PRIME_PBS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_PBS_API(32, uint32_t, cntt_plan32)
