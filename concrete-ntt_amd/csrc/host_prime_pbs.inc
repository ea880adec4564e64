// Part of host_prime.hip (included at its end; kept apart so that file stays readable): the prime plans' side of the programmable
// bootstrap (include/cntt_prime_pbs.h) -- the constants and the launch of prime_gadget_kernel (prime_pbs.hpp; launched by prime_pbs.hip),
// what the shared pipelines (pbs_host.hpp, multibit_host.hpp, cbs_host.hpp) need to know of these plans, and the C ABI over the first.  The loop's
// external product is external_product_device above, which it calls and does not change.
#include "../../include/cntt_prime_pbs.h"
#include "cbs_host.hpp"
#include "multibit_host.hpp"
#include "prime_manylut.hpp"
#include "prime_pbs.hpp"

#pragma GCC visibility push(hidden)

// W of the header: the bit length of p
template <class T> static unsigned modulus_bits(const PrimePlan<T> *pl) {
    unsigned w = 0;
    while (w < PrimePlan<T>::B && ((uint64_t)pl->p >> w) != 0) ++w;
    return w;
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

// What the shared bootstrap pipelines need to know of the prime plans: words of type T, digits of the bit length of p, and a key in one
// buffer of T.  One struct for the bootstrap, the multi-bit bootstrap, the circuit bootstrap and the many-LUT calls.
template <class T> struct PrimePbs {
    using Plan = PrimePlan<T>;
    using Word = T;
    static constexpr const char *NAME = "prime";
    static size_t word(const Plan *) { return sizeof(T); }
    static int logn(const Plan *pl) { return pl->logn; }
    static unsigned digit_bits(const Plan *pl) { return modulus_bits(pl); }
    static constexpr const char *DIGIT_BUDGET_MSG = "%sbase_log * %slevels = %u * %u exceeds the bit length %u of the modulus";
    static int check_terms(const Plan *, size_t, unsigned) { return CNTT_OK; }   // the sums are taken mod p: any number of terms

    using Key = const T *;
    struct KeyStore {};
    static int key_check(const Plan *, Key key, const char *name) { return key ? CNTT_OK : fail(CNTT_EINVAL, "%s is NULL", name); }
    static size_t key_bytes(const Plan *pl, size_t polys) { return polys * pl->n * sizeof(T); }
    static Key key_in(const Plan *, Staging &s, Key bsk, size_t bytes, KeyStore &) { return (Key)s.in(bsk, bytes); }
    static Key key_at(const Plan *, Key bsk, size_t offset, KeyStore &) { return bsk + offset / sizeof(T); }

    static constexpr int MODSWITCH_MAX_LOGN = 29;   // floor(x 4n / p) in 32 bits
    static constexpr int TILE = PRIME_PBS_TILE;
    static hipError_t launch_modswitch(const Plan *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch, unsigned grid, hipStream_t st) {
        return launch_prime_lwe_modswitch<T>(rot_t, lwe, pl->p, pl->logn, lwe_dim, batch, grid, st);
    }
    static hipError_t launch_pbs_init(const Plan *pl, T *acc, const T *lut, const uint32_t *rot, uint32_t npolys, bool per_element, size_t batch,
                                      bool stream, unsigned grid, hipStream_t st) {
        return launch_prime_pbs_init<T>(acc, lut, rot, pl->p, pl->logn, npolys, per_element, batch, stream, grid, st);
    }
    static hipError_t launch_sample_extract(const Plan *pl, T *lwe_out, const T *glwe, size_t glwe_dim, uint32_t index, size_t batch,
                                            unsigned grid, hipStream_t st) {
        return launch_prime_sample_extract<T>(lwe_out, glwe, pl->p, pl->logn, glwe_dim, index, batch, grid, st);
    }
    static constexpr auto gadget = gadget_device<T>;   // the two steps of the loop
    static constexpr auto ext_product = external_product_device<T>;

    // the multi-bit blind rotation and bootstrap (multibit_host.hpp): every plan has them, the sums are taken mod p, no size is refused,
    // and the step works in place on the digits and acc, so the workspace has no scratch.  multibit_step: host_prime_multibit.inc
    static bool multibit_supported(const Plan *) { return true; }
    static int multibit_plan_check(const Plan *) { return CNTT_OK; }
    static bool multibit_sizes_fit(const Plan *, size_t, size_t, unsigned, size_t) { return true; }
    static int multibit_check_terms(const Plan *, size_t, unsigned, unsigned) { return CNTT_OK; }
    static constexpr int MAX_LDS_LOGN = MaxLdsLogN<T>::value;
    static void multibit_scratch(const Plan *, size_t, unsigned, size_t *) {}
    static int multibit_key_operands(const Plan *, Operand *ops, int cnt, Key bsk, size_t kb) {
        ops[cnt++] = {"bsk_mb", bsk, kb, sizeof(T), false};
        return cnt;
    }
    static int multibit_step(const Plan *pl, T *acc, T *digits, char *scratch, const MultibitSizes &Z, const uint32_t *rot_rows, Key key,
                             size_t nterms, size_t npolys, unsigned grouping, size_t batch, hipStream_t st);

    // the circuit bootstrap and the many-LUT calls (cbs_host.hpp); what is only declared: host_prime_cbs.inc.  Every plan has them, the
    // selector gadget may fill the bit length, the extraction takes any size, the output is one buffer that the sum of the slabs writes
    // (no selector words, nothing to finish), and the functional key is in the NTT domain like the other keys.
    using CbsConst = PrimeCbsSetup<T>;
    using CbsShape = ::CbsShape;
    using CbsOut = T *;
    static constexpr auto cbs_shape = prime_cbs_shape;
    static constexpr bool CBS_SEL = false;
    static constexpr size_t EXTRACT_MANY_ROWS = EXM_ROWS;
    static size_t key_word(const Plan *) { return sizeof(T); }   // bytes of one key or output residue
    static Operand fpksk_operand(const Plan *, const T *fpksk, size_t bytes) { return {"fpksk_ntt", fpksk, bytes, sizeof(T), false}; }
    static CbsConst cbs_const(const Plan *pl, size_t k, unsigned cbs_base_log, unsigned cbs_levels);
    static int cbs_plan_check(const Plan *) { return CNTT_OK; }
    static int cbs_budget_check(const Plan *, unsigned, unsigned) { return CNTT_OK; }
    static int extract_many_check(const Plan *) { return CNTT_OK; }
    static int bsk_operands(const Plan *, Operand *ops, int cnt, Key bsk, size_t kb) {
        ops[cnt++] = {"bsk_ntt", bsk, kb, sizeof(T), false};
        return cnt;
    }
    static int cbs_out_planes(const Plan *, CbsOut out, void **planes, const char **names) {
        planes[0] = out;
        names[0] = "ggsw_ntt_out";
        return 1;
    }
    static hipError_t launch_modswitch_manylut(const Plan *pl, uint32_t *rot_t, const T *lwe, unsigned log_lut, size_t lwe_dim, size_t batch,
                                               unsigned grid, hipStream_t st) {
        return launch_prime_modswitch_manylut<T>(rot_t, lwe, pl->p, pl->logn, log_lut, lwe_dim, batch, grid, st);
    }
    static hipError_t launch_extract_many(const Plan *pl, T *lwe_out, const T *glwe, size_t k, size_t count, size_t batch, bool stream,
                                          unsigned grid, hipStream_t st) {
        return launch_prime_sample_extract_many<T>(lwe_out, glwe, pl->p, pl->logn, k, count, batch, stream, grid, st);
    }
    static hipError_t launch_cbs_setup(const Plan *pl, uint32_t *rot_t, T *table, const T *lwe, const CbsConst &C, const unsigned *log_lut,
                                       size_t lwe_dim, size_t rotations, unsigned grid, hipStream_t st);
    static hipError_t launch_cbs_extract(const Plan *pl, int32_t *digits, const T *acc, unsigned ks_base_log, unsigned ks_levels,
                                         const CbsConst &C, bool one_rotation, size_t rotations, unsigned grid, hipStream_t st);
    static hipError_t launch_cbs_ks(const Plan *pl, T *part, const int32_t *digits, const T *fpksk, size_t k, size_t rows, size_t elements,
                                    const CbsShape &shape, unsigned ks_base_log, hipStream_t st);
    static hipError_t launch_cbs_sum(const Plan *pl, T *out, const T *part, size_t k, unsigned cbs_levels, size_t elements, size_t slabs,
                                     unsigned grid, hipStream_t st) {
        return launch_prime_cbs_sum<T>(out, part, pl->p, pl->logn, k, cbs_levels, elements, slabs, grid, st);
    }
    static int cbs_finish(const Plan *, void *const *, const T *, size_t, hipStream_t) { return CNTT_OK; }
};
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
#define CNTT_PRIME_PBS_API(BITS, T, PLAN)                                                                                                    \
    extern "C" int cntt_prime##BITS##_gadget_decompose_batch(const PLAN *pl, T *terms, const T *polys, const uint32_t *rot, size_t npolys,    \
                                                             unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t batch,     \
                                                             cntt_mem_t where, void *stream) {                                               \
        return gadget_decompose<PrimePbs<T>>(pl, terms, polys, rot, npolys, base_log, levels, (int)src_mode, batch, where,                    \
                                             (hipStream_t)stream);                                                                            \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_lwe_modswitch_batch(const PLAN *pl, uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch,        \
                                                          cntt_mem_t where, void *stream) {                                                  \
        return lwe_modswitch<PrimePbs<T>>(pl, rot_t, lwe, lwe_dim, batch, where, (hipStream_t)stream);                                        \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_blind_rotate_batch(const PLAN *pl, T *acc, const T *lut, int lut_per_element, const uint32_t *rot_t,    \
                                                         const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log,               \
                                                         unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,             \
                                                         cntt_mem_t where, void *stream) {                                                   \
        return blind_rotate<PrimePbs<T>>(pl, acc, lut, lut_per_element, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch,           \
                                         workspace, workspace_bytes, where, (hipStream_t)stream);                                             \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_sample_extract_batch(const PLAN *pl, T *lwe_out, const T *glwe, size_t glwe_dim, size_t index,          \
                                                           size_t batch, cntt_mem_t where, void *stream) {                                   \
        return sample_extract<PrimePbs<T>>(pl, lwe_out, glwe, glwe_dim, index, batch, where, (hipStream_t)stream);                            \
    }                                                                                                                                        \
    extern "C" int cntt_prime##BITS##_bootstrap_batch(const PLAN *pl, T *lwe_out, const T *lwe_in, const T *lut, int lut_per_element,         \
                                                      const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, \
                                                      size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where,               \
                                                      void *stream) {                                                                        \
        return bootstrap<PrimePbs<T>>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch,         \
                                      workspace, workspace_bytes, where, (hipStream_t)stream);                                                \
    }                                                                                                                                        \
    extern "C" size_t cntt_prime##BITS##_pbs_workspace_bytes(const PLAN *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels,                \
                                                             size_t batch) {                                                                 \
        return pbs_workspace_bytes<PrimePbs<T>>(pl, lwe_dim, glwe_dim, levels, batch);                                                        \
    }

CNTT_PRIME_PBS_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_PBS_API(32, uint32_t, cntt_plan32)
