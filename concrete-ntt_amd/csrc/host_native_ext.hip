// libcntt_hip.so host side, what is built on the native plans without a counterpart in the reference: the external product
// (include/cntt_ext.h), rotation / gadget decomposition and the external product on undecomposed polynomials (include/cntt_gadget.h),
// the programmable bootstrap (include/cntt_pbs.h), the LWE keyswitch and keyswitch + bootstrap (include/cntt_keyswitch.h), the
// LWE-to-GLWE packing keyswitch (include/cntt_pack.h), the multi-bit blind rotation and bootstrap (include/cntt_multibit.h).  The last
// four are the templates of pbs_host.hpp, lwe_host.hpp and multibit_host.hpp, shared with the prime plans: here are the family struct that
// fits them to the native plans (NativePbs) and the C ABI over them (the multi-bit part: host_native_multibit.inc).  The CMux and the
// CMux tree against GGSW selectors (include/cntt_cmux.h) are host_native_cmux.inc, over the same struct; the circuit bootstrap that
// makes such selectors from LWE bits (include/cntt_cbs.h) and the many-LUT calls (include/cntt_manylut.h) are the templates of
// cbs_host.hpp, with the struct's members and the C ABI in host_native_cbs.inc.  The ring automorphism, the Galois keyswitch and the trace
// (include/cntt_automorphism.h) are host_native_automorphism.inc, and ring packing of LWE ciphertexts through them (include/cntt_ring_pack.h) is
// host_native_ring_pack.inc.
#include <cstdio>

#include "cbs_host.hpp"
#include "host_common.hpp"
#include "lwe_host.hpp"
#include "multibit_host.hpp"
#include "native_gadget.hpp"
#include "native_keyswitch.hpp"
#include "native_manylut.hpp"
#include "native_pack.hpp"
#include "native_pbs.hpp"

// ---------------------------------------------------------------------------------------------
// external product of the native plans (include/cntt_ext.h; no counterpart in the reference)
// ---------------------------------------------------------------------------------------------
extern "C" size_t cntt_native_max_terms(const cntt_native_t *pl) { return pl ? pl->max_terms : 0; }

// fused kernel (native_ext.hpp) for the Plan32 kinds at 32 <= n <= 4096; FUSED_NONE where it does not exist
static int native_ext_fused(const cntt_native *pl, void *out, const void *terms, const void *const *key, size_t nterms, size_t nout,
                            size_t batch, bool accumulate, hipStream_t st) {
    if (pl->info.is52 || !pl->has_acc || debug_switch(DBG_NATIVE_EXT) == 0 || batch >= ((size_t)1 << 32) ||
        nterms >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32))
        return FUSED_NONE;
    return native_fused_launch(pl, "fused external product", [&](auto kind, int &rc) {
        constexpr int KIND = decltype(kind)::value;
        FusedTables<NativeShape<KIND>::KP> Facc{};
        KeyPlanes K{};
        if ((rc = native_acc_tables<KIND>(pl, key, &Facc, &K))) return hipErrorUnknown;
        const SplitArgs S = native_split_args(pl, nullptr);
        return launch_native_ext<KIND>(pl->p32[0]->logn, out, terms, K, &Facc, S, pl->acc, (uint32_t)batch, (uint32_t)nterms, (uint32_t)nout,
                                       accumulate, st);
    });
}

// word width of a native kind -> its word type, handed to f as a value
template <class F> static auto with_word(const cntt_native *pl, F &&f) {
    switch (pl->info.word) {
    case 4: return f(uint32_t{});
    case 8: return f(uint64_t{});
    default: return f(Word128{});
    }
}
// a[i] += b[i] modulo 2^w
static int word_add_launch(const cntt_native *pl, void *a, const void *b, size_t count, hipStream_t st) {
    with_word(pl, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_word_add_kernel<W>), dim3(ew_grid(count)), dim3(256), 0, st, (W *)a, (const W *)b, count);
    });
    if (hipGetLastError() != hipSuccess) return fail(CNTT_EDEVICE, "native_word_add_kernel launch failed");
    return CNTT_OK;
}

// composed: residue split of all terms, one mul_accumulate chain per prime on the plane layout (its unnormalised inverse carries a
// factor n: a normalize pass takes it off), one CRT -- into `out`, or into scratch and then added to `out` modulo 2^w
static int native_ext_composed(const cntt_native *pl, void *out, const void *terms, const void *const *key, size_t nterms, size_t nout,
                               size_t batch, bool accumulate, hipStream_t st) {
    const int k = pl->info.nprimes;
    const size_t n = pl->n, rb = pl->rbytes(), tcount = batch * nterms * n, ocount = batch * nout * n;
    const size_t wbytes = (size_t)pl->info.word;
    const size_t bytes = (size_t)k * (tcount + ocount) * rb + (accumulate ? ocount * wbytes : 0);
    StreamBlock block(st);
    if (int rc = block.alloc(bytes)) return rc;
    char *scratch = (char *)block.get();
    void *T[10], *O[10];
    for (int i = 0; i < k; ++i) {
        T[i] = scratch + (size_t)i * tcount * rb;
        O[i] = scratch + ((size_t)k * tcount + (size_t)i * ocount) * rb;
    }
    void *crt_out = accumulate ? scratch + (size_t)k * (tcount + ocount) * rb : out;
    int rc = native_split_device(pl, terms, T, tcount, false, st);
    for (int i = 0; i < k && rc == CNTT_OK; ++i) {
        if (pl->info.is52) {
            const cntt_plan64 *sub = pl->p64[(size_t)i].get();
            rc = external_product_device<uint64_t>(sub, (uint64_t *)O[i], (const uint64_t *)T[i], (const uint64_t *)key[i], nterms, nout,
                                                   batch, false, st);
            if (rc == CNTT_OK) rc = pointwise_device<uint64_t, PW_NORMALIZE>(sub, (uint64_t *)O[i], nullptr, nullptr, ocount, st);
        } else {
            const cntt_plan32 *sub = pl->p32[(size_t)i].get();
            rc = external_product_device<uint32_t>(sub, (uint32_t *)O[i], (const uint32_t *)T[i], (const uint32_t *)key[i], nterms, nout,
                                                   batch, false, st);
            if (rc == CNTT_OK) rc = pointwise_device<uint32_t, PW_NORMALIZE>(sub, (uint32_t *)O[i], nullptr, nullptr, ocount, st);
        }
    }
    if (rc == CNTT_OK) rc = native_crt_device(pl, crt_out, O, ocount, st);
    if (rc == CNTT_OK && accumulate) rc = word_add_launch(pl, out, crt_out, ocount, st);
    return rc;
}

static int native_ext_device(const cntt_native *pl, void *out, const void *terms, const void *const *key, size_t nterms, size_t nout,
                             size_t batch, bool accumulate, hipStream_t st) {
    if (nterms == 0) {   // the empty sum
        if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, batch * nout * pl->n * (size_t)pl->info.word, st));
        return CNTT_OK;
    }
    const int rc = native_ext_fused(pl, out, terms, key, nterms, nout, batch, accumulate, st);
    if (rc != FUSED_NONE) return rc;
    return native_ext_composed(pl, out, terms, key, nterms, nout, batch, accumulate, st);
}

// key residue planes, one per prime: none may be NULL (`name`: the argument as the message names it, or nullptr)
static int check_key_planes(const cntt_native *pl, const void *const *key, const char *name) {
    for (int i = 0; i < pl->info.nprimes; ++i) {
        if (key[i]) continue;
        char where[48] = "";
        if (name) snprintf(where, sizeof where, " (%s[%d])", name, i);
        return fail(CNTT_EINVAL, "NULL key residue plane%s", where);
    }
    return CNTT_OK;
}
// the planes as the _device functions take them: the caller's pointers (device path) or device copies of `bytes` each (host path);
// no bytes: `key` itself may be NULL
static void key_planes_to_device(const cntt_native *pl, Staging &s, const void *const *key, size_t bytes, const void **dkey) {
    for (int i = 0; i < pl->info.nprimes; ++i) dkey[i] = s.in(bytes ? key[i] : nullptr, bytes);
}

extern "C" int cntt_native_external_product_batch(const cntt_native_t *pl, void *out, const void *terms, const void *const *key_ntt,
                                                  size_t nterms, size_t nout, size_t batch, int accumulate, cntt_mem_t where,
                                                  void *stream) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (nterms > pl->max_terms)
        return fail(CNTT_EINVAL, "nterms = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range", nterms,
                    pl->max_terms);
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (!out) return fail(CNTT_EINVAL, "NULL argument");
    if (nterms) {
        if (!terms || !key_ntt) return fail(CNTT_EINVAL, "NULL argument");
        if (int rc = check_key_planes(pl, key_ntt, nullptr)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t n = pl->n, w = (size_t)pl->info.word, ob = batch * nout * n * w, tb = batch * nterms * n * w;
    Staging s(where, st);
    const void *dkey[10];
    key_planes_to_device(pl, s, key_ntt, nterms * nout * n * pl->rbytes(), dkey);
    void *dout = accumulate ? s.inout(out, ob) : s.out(out, ob);
    const void *dt = s.in(terms, tb);
    if (int rc = s.status()) return rc;
    if (int rc = native_ext_device(pl, dout, dt, dkey, nterms, nout, batch, accumulate != 0, st)) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------
// rotation / CMux difference / signed gadget decomposition and the external product on undecomposed polynomials
// (include/cntt_gadget.h, native_gadget.hpp)
// ---------------------------------------------------------------------------------------------
// off = 2^(s-1) + K 2^s mod 2^w, K = sum_l (B/2) B^(levels-l), s = w - base_log levels (native_gadget.hpp)
static u128 gadget_offset(unsigned wbits, unsigned base_log, unsigned levels) {
    const unsigned s = wbits - base_log * levels;
    u128 off = s ? (u128)1 << (s - 1) : 0;
    for (unsigned l = 1; l <= levels; ++l) off += (u128)1 << (wbits - base_log * l + base_log - 1);   // (B/2) B^(levels-l) 2^s
    return off;   // (wbits < 128: the caller truncates)
}
template <class W> static W word_from(u128 v) { return (W)v; }
template <> Word128 word_from<Word128>(u128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

template <class W>
static int gadget_launch_w(void *terms, const void *polys, const uint32_t *rot, size_t npolys, unsigned base_log, unsigned levels, int mode,
                           size_t batch, int logn, hipStream_t st) {
    constexpr unsigned WB = sizeof(W) * 8;
    GadgetConst<W> G{};
    G.off = word_from<W>(gadget_offset(WB, base_log, levels));
    G.mask = word_from<W>(base_log == 128 ? ~(u128)0 : ((u128)1 << base_log) - 1);
    G.half = word_from<W>((u128)1 << (base_log - 1));
    G.base_log = base_log;
    G.levels = levels;
    G.npolys = (uint32_t)npolys;
    G.rotated = mode != CNTT_SRC_PLAIN;
    G.cmux = mode == CNTT_SRC_CMUX;
    const size_t total = batch * npolys, n = (size_t)1 << logn;
    const unsigned grid = ew_grid(total * n * sizeof(W) / 16);
    // the terms against STREAM_BYTES, as the pointwise kernels decide it: larger ones pass through once (non-temporal stores)
    if (total * levels * n * sizeof(W) > STREAM_BYTES)
        hipLaunchKernelGGL((native_gadget_kernel<W, true>), dim3(grid), dim3(256), 0, st, (W *)terms, (const W *)polys, rot, G, (uint32_t)logn, total);
    else
        hipLaunchKernelGGL((native_gadget_kernel<W, false>), dim3(grid), dim3(256), 0, st, (W *)terms, (const W *)polys, rot, G, (uint32_t)logn, total);
    if (hipGetLastError() != hipSuccess) return fail(CNTT_EDEVICE, "native_gadget_kernel launch failed");
    return CNTT_OK;
}
static int native_logn(const cntt_native *pl) {
    int logn = 0;
    while (((size_t)1 << logn) < pl->n) ++logn;
    return logn;
}
static int native_gadget_device(const cntt_native *pl, void *terms, const void *polys, const uint32_t *rot, size_t npolys, unsigned base_log,
                                unsigned levels, int mode, size_t batch, hipStream_t st) {
    if (batch == 0 || npolys == 0) return CNTT_OK;
    if (npolys >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "npolys too large");
    return with_word(pl, [&](auto w) {
        return gadget_launch_w<decltype(w)>(terms, polys, rot, npolys, base_log, levels, mode, batch, native_logn(pl), st);
    });
}

// What the shared host pipelines (pbs_host.hpp, lwe_host.hpp, multibit_host.hpp, cbs_host.hpp) need to know of the native plans: words of
// 4, 8 or 16 bytes behind void pointers, digits of the whole word, and a key of one residue plane per prime.  One struct for the bootstrap,
// the keyswitch, the packing keyswitch, the multi-bit bootstrap, the circuit bootstrap and the many-LUT calls (the name is from its first
// user), so that the combined calls run the bootstrap's own instantiation of the loop.
#pragma GCC visibility push(hidden)
struct NativePbs {
    using Plan = cntt_native;
    using Word = void;
    static constexpr const char *NAME = "native";
    static size_t word(const cntt_native *pl) { return (size_t)pl->info.word; }
    static int logn(const cntt_native *pl) { return native_logn(pl); }
    static unsigned digit_bits(const cntt_native *pl) { return 8u * (unsigned)pl->info.word; }
    static constexpr const char *DIGIT_BUDGET_MSG = "%sbase_log * %slevels = %u * %u exceeds the word width %u";
    static int check_terms(const cntt_native *pl, size_t glwe_dim, unsigned levels) {
        const size_t nterms = (glwe_dim + 1) * levels;
        if (nterms > pl->max_terms)
            return fail(CNTT_EINVAL, "(glwe_dim + 1) * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range",
                        nterms, pl->max_terms);
        return CNTT_OK;
    }

    using Key = const void *const *;
    struct KeyStore {
        const void *plane[10];
    };
    static int key_check(const cntt_native *pl, Key key, const char *name) {
        if (!key) return fail(CNTT_EINVAL, "%s is NULL", name);
        return check_key_planes(pl, key, name);
    }
    static size_t key_bytes(const cntt_native *pl, size_t polys) { return polys * pl->n * pl->rbytes(); }
    static Key key_in(const cntt_native *pl, Staging &s, Key bsk, size_t bytes, KeyStore &ks) {
        key_planes_to_device(pl, s, bsk, bytes, ks.plane);
        return ks.plane;
    }
    static Key key_at(const cntt_native *pl, Key bsk, size_t offset, KeyStore &ks) {
        for (int j = 0; j < pl->info.nprimes; ++j) ks.plane[j] = static_cast<const char *>(bsk[j]) + offset;
        return ks.plane;
    }

    static constexpr int MODSWITCH_MAX_LOGN = 30;   // ms() reads the top 32 bits
    static constexpr int TILE = PBS_TILE;
    static hipError_t launch_modswitch(const cntt_native *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim, size_t batch, unsigned grid,
                                       hipStream_t st) {
        return launch_native_lwe_modswitch(pl->info.word, rot_t, lwe, native_logn(pl), lwe_dim, batch, grid, st);
    }
    static hipError_t launch_pbs_init(const cntt_native *pl, void *acc, const void *lut, const uint32_t *rot, uint32_t npolys, bool per_element,
                                      size_t batch, bool stream, unsigned grid, hipStream_t st) {
        return launch_native_pbs_init(pl->info.word, acc, lut, rot, native_logn(pl), npolys, per_element, batch, stream, grid, st);
    }
    static hipError_t launch_sample_extract(const cntt_native *pl, void *lwe_out, const void *glwe, size_t glwe_dim, uint32_t index, size_t batch,
                                            unsigned grid, hipStream_t st) {
        return launch_native_sample_extract(pl->info.word, lwe_out, glwe, native_logn(pl), glwe_dim, index, batch, grid, st);
    }
    static constexpr auto gadget = native_gadget_device;   // the two steps of the loop
    static constexpr auto ext_product = native_ext_device;

    // the keyswitch (lwe_host.hpp); these plans have no bound on the key rows
    static constexpr bool KS_ROWS_GUARD = false;
    static hipError_t launch_keyswitch(const cntt_native *pl, void *out, const void *in, const void *ksk, size_t lin, size_t lout,
                                       size_t row_stride, unsigned base_log, unsigned levels, size_t batch, hipStream_t st) {
        const u128 off = gadget_offset(digit_bits(pl), base_log, levels);
        return launch_native_keyswitch(pl->info.word, out, in, ksk, (uint64_t)off, (uint64_t)(off >> 64), base_log, levels, lin, lout,
                                       row_stride, batch, st);
    }

    // the packing keyswitch (lwe_host.hpp)
    static size_t pack_chunk_terms(const cntt_native *pl) { return std::min<size_t>(pl->max_terms, CNTT_PACK_TERMS); }
    static int pack_check_levels(const cntt_native *pl, unsigned levels) {
        if (levels > pl->max_terms)
            return fail(CNTT_EINVAL, "levels = %u exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range", levels,
                        pl->max_terms);
        return CNTT_OK;
    }
    static int pack_check_sizes(const cntt_native *, size_t, size_t, size_t, unsigned, size_t) { return CNTT_OK; }
    static bool pack_key_overlaps(const void *, size_t, Key, size_t) { return false; }
    static hipError_t launch_pack_body(const cntt_native *pl, void *out, const void *in, size_t glwe_dim, size_t lin, size_t m, size_t batch,
                                       unsigned grid, hipStream_t st) {
        return launch_native_pack_body(pl->info.word, out, in, native_logn(pl), glwe_dim, lin, m, batch, grid, st);
    }
    static hipError_t launch_pack_decompose(const cntt_native *pl, void *terms, const void *in, unsigned base_log, unsigned levels, size_t lin,
                                            size_t m, size_t i0, size_t nw, size_t batch, hipStream_t st) {
        const u128 off = gadget_offset(digit_bits(pl), base_log, levels);
        return launch_native_pack_decompose(pl->info.word, terms, in, (uint64_t)off, (uint64_t)(off >> 64), base_log, levels, native_logn(pl),
                                            lin, m, i0, nw, batch, st);
    }

    // the multi-bit blind rotation and bootstrap (multibit_host.hpp): the Plan32 kinds only; all but the first: host_native_multibit.inc
    static bool multibit_supported(const cntt_native *pl) { return !pl->info.is52; }
    static int multibit_plan_check(const cntt_native *pl);
    static bool multibit_sizes_fit(const cntt_native *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch);
    static int multibit_check_terms(const cntt_native *pl, size_t glwe_dim, unsigned levels, unsigned grouping);
    static constexpr int MAX_LDS_LOGN = MaxLdsLogN<uint32_t>::value;   // the sub-plans' transforms
    static void multibit_scratch(const cntt_native *pl, size_t polys, unsigned levels, size_t *bytes);   // term planes, output planes
    static int multibit_key_operands(const cntt_native *pl, Operand *ops, int cnt, Key bsk, size_t kb);
    static int multibit_step(const cntt_native *pl, void *acc, void *digits, char *scratch, const MultibitSizes &Z,
                             const uint32_t *rot_rows, Key key, size_t nterms, size_t npolys, unsigned grouping, size_t batch, hipStream_t st);

    // the circuit bootstrap and the many-LUT calls (cbs_host.hpp); what is only declared: host_native_cbs.inc.  The output is one residue
    // plane per prime; the sum of the slabs goes to selector words in the workspace (CBS_SEL), which cbs_finish splits and transforms into
    // the planes, 2^46 words at most; the functional key is in words, read in 16-byte vectors.
    using CbsConst = NativeCbsConst;
    using CbsShape = NativeCbsShape;
    using CbsOut = void *const *;
    static constexpr auto cbs_shape = native_cbs_shape;
    static constexpr bool CBS_SEL = true;
    static constexpr size_t EXTRACT_MANY_ROWS = NEXM_ROWS;
    static size_t key_word(const cntt_native *pl) { return pl->rbytes(); }   // bytes of one key or output residue
    static Operand fpksk_operand(const cntt_native *, const void *fpksk, size_t bytes) { return {"fpksk", fpksk, bytes, 16, false}; }
    static CbsConst cbs_const(const cntt_native *pl, size_t k, unsigned cbs_base_log, unsigned cbs_levels) {
        return CbsConst{(uint32_t)native_logn(pl), (uint32_t)k, cbs_base_log, cbs_levels};
    }
    static int cbs_plan_check(const cntt_native *pl);                                                // no binary kinds
    static int cbs_budget_check(const cntt_native *pl, unsigned cbs_base_log, unsigned cbs_levels);   // w - 1 bits, not w
    static int extract_many_check(const cntt_native *pl);                                            // a row holds a 16-byte vector
    static int bsk_operands(const cntt_native *pl, Operand *ops, int cnt, Key bsk, size_t kb);
    static int cbs_out_planes(const cntt_native *pl, CbsOut out, void **planes, const char **names);
    static hipError_t launch_modswitch_manylut(const cntt_native *pl, uint32_t *rot_t, const void *lwe, unsigned log_lut, size_t lwe_dim,
                                               size_t batch, unsigned grid, hipStream_t st);
    static hipError_t launch_extract_many(const cntt_native *pl, void *lwe_out, const void *glwe, size_t k, size_t count, size_t batch,
                                          bool stream, unsigned grid, hipStream_t st);
    static hipError_t launch_cbs_setup(const cntt_native *pl, uint32_t *rot_t, void *table, const void *lwe, const CbsConst &C,
                                       const unsigned *log_lut, size_t lwe_dim, size_t rotations, unsigned grid, hipStream_t st);
    static hipError_t launch_cbs_extract(const cntt_native *pl, int32_t *digits, const void *acc, unsigned ks_base_log, unsigned ks_levels,
                                         const CbsConst &C, bool one_rotation, size_t rotations, unsigned grid, hipStream_t st);
    static hipError_t launch_cbs_ks(const cntt_native *pl, void *part, const int32_t *digits, const void *fpksk, size_t k, size_t rows,
                                    size_t elements, const CbsShape &shape, unsigned ks_base_log, hipStream_t st);
    static hipError_t launch_cbs_sum(const cntt_native *pl, void *sel, const void *part, size_t k, unsigned cbs_levels, size_t elements,
                                     size_t slabs, unsigned grid, hipStream_t st);
    static int cbs_finish(const cntt_native *pl, void *const *out, const void *sel, size_t polys, hipStream_t st);
};
#pragma GCC visibility pop

extern "C" int cntt_native_gadget_decompose_batch(const cntt_native_t *pl, void *terms, const void *polys, const uint32_t *rot,
                                                  size_t npolys, unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t batch,
                                                  cntt_mem_t where, void *stream) {
    return gadget_decompose<NativePbs>(pl, terms, polys, rot, npolys, base_log, levels, (int)src_mode, batch, where, (hipStream_t)stream);
}

// fused kernel (native_gadget.hpp): the 32- and 64-bit Plan32 kinds at 32 <= n <= 4096, base_log <= 31; FUSED_NONE elsewhere
static int native_ext_gadget_fused(const cntt_native *pl, void *out, const GadgetCall &G, const void *const *key, size_t nout, size_t batch,
                                   hipStream_t st) {
    if (pl->info.is52 || !pl->has_acc || pl->info.word > 8 || G.base_log > 31 || debug_switch(DBG_NATIVE_GADGET) <= 0 ||
        batch >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32))
        return FUSED_NONE;
    return native_fused_launch(pl, "fused decomposing external product", [&](auto kind, int &rc) {
        constexpr int KIND = decltype(kind)::value;
        if constexpr (sizeof(typename NativeShape<KIND>::W) > 8) {
            return hipErrorNotSupported;
        } else {
            FusedTables<NativeShape<KIND>::KP> Facc{};
            KeyPlanes K{};
            if ((rc = native_acc_tables<KIND>(pl, key, &Facc, &K))) return hipErrorUnknown;
            const SplitArgs S = native_split_args(pl, nullptr);
            return launch_native_ext_gadget<KIND>(pl->p32[0]->logn, out, G, K, &Facc, S, pl->acc, (uint32_t)batch, (uint32_t)nout, st);
        }
    });
}
// addend: nullptr, `out`, or a buffer that does not overlap out (checked by the caller)
static int native_ext_gadget_device(const cntt_native *pl, void *out, const void *polys, const uint32_t *rot, const void *addend,
                                    const void *const *key, size_t npolys, unsigned base_log, unsigned levels, int mode, size_t nout,
                                    size_t batch, hipStream_t st) {
    const size_t n = pl->n, w = (size_t)pl->info.word, ocount = batch * nout * n, nterms = npolys * levels;
    if (nterms == 0) {   // the empty sum: out = addend, or zero
        if (!addend) HIP_TRY(hipMemsetAsync(out, 0, ocount * w, st));
        else if (addend != out) HIP_TRY(hipMemcpyAsync(out, addend, ocount * w, hipMemcpyDeviceToDevice, st));
        return CNTT_OK;
    }
    GadgetCall G{};
    G.polys = polys;
    G.rot = mode == CNTT_SRC_PLAIN ? nullptr : rot;
    G.addend = addend == out ? nullptr : addend;
    G.off = w <= 8 ? (uint64_t)gadget_offset(8u * (unsigned)w, base_log, levels) : 0;   // (the fused kernel: u32 / u64 words)
    G.npolys = (uint32_t)npolys;
    G.levels = levels;
    G.base_log = base_log;
    G.cmux = mode == CNTT_SRC_CMUX;
    G.add_out = addend == out;
    const int rc = native_ext_gadget_fused(pl, out, G, key, nout, batch, st);
    if (rc != FUSED_NONE) return rc;
    // composed: the digits into stream-ordered scratch, the external product on them, then the addend
    StreamBlock digits(st);
    if (int rc2 = digits.alloc(batch * nterms * n * w)) return rc2;
    if (int rc2 = native_gadget_device(pl, digits.get(), polys, rot, npolys, base_log, levels, mode, batch, st)) return rc2;
    if (int rc2 = native_ext_device(pl, out, digits.get(), key, nterms, nout, batch, addend == out, st)) return rc2;
    return addend && addend != out ? word_add_launch(pl, out, addend, ocount, st) : CNTT_OK;
}

extern "C" int cntt_native_external_product_decomposed_batch(const cntt_native_t *pl, void *out, const void *polys, const uint32_t *rot,
                                                             const void *addend, const void *const *key_ntt, size_t npolys,
                                                             unsigned base_log, unsigned levels, cntt_src_mode_t src_mode, size_t nout,
                                                             size_t batch, cntt_mem_t where, void *stream) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check<NativePbs>(pl, base_log, levels, (int)src_mode, rot)) return rc;
    const size_t nterms = npolys * levels;
    if (nterms > pl->max_terms)
        return fail(CNTT_EINVAL, "npolys * levels = %zu exceeds cntt_native_max_terms() = %zu: the sum would leave the exact CRT range", nterms,
                    pl->max_terms);
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (!out) return fail(CNTT_EINVAL, "out is NULL");
    const size_t n = pl->n, w = (size_t)pl->info.word, ob = batch * nout * n * w, pb = batch * npolys * n * w;
    if (nterms) {
        if (!polys || !key_ntt) return fail(CNTT_EINVAL, "NULL argument");
        if (int rc = check_key_planes(pl, key_ntt, nullptr)) return rc;
        if (ranges_overlap(out, ob, polys, pb)) return fail(CNTT_EINVAL, "out overlaps polys");
    }
    if (addend && addend != out && ranges_overlap(out, ob, addend, ob)) return fail(CNTT_EINVAL, "addend overlaps out without being out");
    hipStream_t st = (hipStream_t)stream;
    const bool rotated = nterms && src_mode != CNTT_SRC_PLAIN;
    Staging s(where, st);
    if (s.host() && rotated)
        if (int rc = check_rot_host(pl->n, rot, batch, "rot")) return rc;
    const void *dkey[10];
    key_planes_to_device(pl, s, key_ntt, nterms * nout * n * pl->rbytes(), dkey);
    const void *dp = s.in(polys, pb);
    const uint32_t *dr = rotated ? (const uint32_t *)s.in(rot, batch * sizeof(uint32_t)) : nullptr;
    void *dout = addend == out ? s.inout(out, ob) : s.out(out, ob);
    const void *dadd = addend == out ? dout : addend && addend == polys && pb == ob ? dp : addend ? s.in(addend, ob) : nullptr;
    if (int rc = s.status()) return rc;
    if (int rc = native_ext_gadget_device(pl, dout, dp, dr, dadd, dkey, npolys, base_log, levels, (int)src_mode, nout, batch, st)) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------
// programmable bootstrap: modulus switch, blind rotation in place, sample extraction (include/cntt_pbs.h, native_pbs.hpp)
// ---------------------------------------------------------------------------------------------
extern "C" size_t cntt_native_pbs_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    return pbs_workspace_bytes<NativePbs>(pl, lwe_dim, glwe_dim, levels, batch);
}
extern "C" int cntt_native_lwe_modswitch_batch(const cntt_native_t *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim, size_t batch,
                                               cntt_mem_t where, void *stream) {
    return lwe_modswitch<NativePbs>(pl, rot_t, lwe, lwe_dim, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_sample_extract_batch(const cntt_native_t *pl, void *lwe_out, const void *glwe, size_t glwe_dim, size_t index,
                                                size_t batch, cntt_mem_t where, void *stream) {
    return sample_extract<NativePbs>(pl, lwe_out, glwe, glwe_dim, index, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_blind_rotate_batch(const cntt_native_t *pl, void *acc, const void *lut, int lut_per_element, const uint32_t *rot_t,
                                              const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                              size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return blind_rotate<NativePbs>(pl, acc, lut, lut_per_element, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace,
                                   workspace_bytes, where, (hipStream_t)stream);
}
extern "C" int cntt_native_bootstrap_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *lut, int lut_per_element,
                                           const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels,
                                           size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return bootstrap<NativePbs>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace,
                                workspace_bytes, where, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// LWE keyswitch, and keyswitch + bootstrap in one call (include/cntt_keyswitch.h, native_keyswitch.hpp; host side: lwe_host.hpp)
// ---------------------------------------------------------------------------------------------

extern "C" int cntt_native_keyswitch_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *ksk, size_t lwe_dim_in,
                                           size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels, size_t batch,
                                           cntt_mem_t where, void *stream) {
    return keyswitch<NativePbs>(pl, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_ks_pbs_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    return ks_pbs_workspace_bytes<NativePbs>(pl, lwe_dim, glwe_dim, levels, batch);
}
extern "C" int cntt_native_keyswitch_bootstrap_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *ksk,
                                                     size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const void *lut,
                                                     int lut_per_element, const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                                     unsigned base_log, unsigned levels, size_t batch, void *workspace, size_t workspace_bytes,
                                                     cntt_mem_t where, void *stream) {
    return keyswitch_bootstrap<NativePbs>(pl, lwe_out, lwe_in, ksk, row_stride, ks_base_log, ks_levels, lut, lut_per_element, bsk_ntt, lwe_dim,
                                         glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// LWE-to-GLWE packing keyswitch through the NTT (include/cntt_pack.h, native_pack.hpp; host side: lwe_host.hpp)
// ---------------------------------------------------------------------------------------------

extern "C" size_t cntt_native_pack_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim_in, unsigned levels, size_t batch) {
    return pack_workspace_bytes<NativePbs>(pl, lwe_dim_in, levels, batch);
}
extern "C" int cntt_native_pack_keyswitch_batch(const cntt_native_t *pl, void *glwe_out, const void *lwe_in, const void *const *pksk_ntt,
                                                size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels,
                                                size_t batch, void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return pack_keyswitch<NativePbs>(pl, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, workspace,
                                      workspace_bytes, where, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// multi-bit blind rotation and bootstrap (include/cntt_multibit.h, native_multibit.hpp)
// ---------------------------------------------------------------------------------------------
#include "host_native_multibit.inc"

// ---------------------------------------------------------------------------------------------
// the CMux and the CMux tree against GGSW selectors (include/cntt_cmux.h, native_cmux.hpp)
// ---------------------------------------------------------------------------------------------
#include "host_native_cmux.inc"

// ---------------------------------------------------------------------------------------------
// the circuit bootstrap from LWE bits to GGSW selectors, the many-LUT bootstrap and the circuit bootstrap with one rotation per input bit
// (include/cntt_cbs.h, cntt_manylut.h; native_cbs.hpp, native_manylut.hpp; host side: cbs_host.hpp)
// ---------------------------------------------------------------------------------------------
#include "host_native_cbs.inc"

// ---------------------------------------------------------------------------------------------
// the ring automorphism X -> X^t, the Galois keyswitch and the trace (include/cntt_automorphism.h, native_automorphism.hpp)
// ---------------------------------------------------------------------------------------------
#include "host_native_automorphism.inc"

// ---------------------------------------------------------------------------------------------
// ring packing of LWE ciphertexts through automorphisms (include/cntt_ring_pack.h, native_ring_pack.hpp)
// ---------------------------------------------------------------------------------------------
#include "host_native_ring_pack.inc"
