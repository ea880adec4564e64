// libcntt_hip.so host side, product::Plan (include/cntt.h): residue split, per-prime steps through host_prime.hip, Garner.
#include "aux_kernels.hpp"
#include "host_common.hpp"
#include "product_fused.hpp"

// ---------------------------------------------------------------------------------------------
// product::Plan  (src/product.rs:139-967)
// ---------------------------------------------------------------------------------------------
// Plan::try_new src/product.rs:153-247
extern "C" int cntt_product_plan_new(size_t n, uint64_t modulus, const uint64_t *factors, size_t nfactors,
                                     cntt_product_t **out) {
    if (!out) return fail(CNTT_EINVAL, "out is NULL");
    *out = nullptr;
    if (nfactors && !factors) return fail(CNTT_EINVAL, "factors is NULL");
    if (n % 2 != 0) return CNTT_NONE;
    std::vector<uint64_t> primes(factors, factors + nfactors);
    std::sort(primes.begin(), primes.end());
    uint64_t prev = 0;
    for (uint64_t f : primes) {  // zero or repeated factor: src/product.rs:163-169
        if (f == prev) return CNTT_NONE;
        prev = f;
    }
    primes.erase(primes.begin(), std::find_if(primes.begin(), primes.end(), [](uint64_t f) { return f != 1; }));
    uint64_t prod = 1;
    for (uint64_t f : primes) {  // checked_mul: src/product.rs:173-177
        const u128 w = (u128)prod * f;
        if (w >> 64) return CNTT_NONE;
        prod = (uint64_t)w;
    }
    if (prod != modulus) return CNTT_NONE;
    // distinct primes = 1 mod 2n >= 65 whose product fits u64: never more than 7; anything longer has a
    // non-prime factor and try_new of that factor would return None anyway
    if (primes.size() >= (size_t)PRODUCT_MAX_PRIMES) return CNTT_NONE;
    std::unique_ptr<cntt_product> pl(new (std::nothrow) cntt_product());
    if (!pl) return fail(CNTT_ENOMEM, "out of memory");
    pl->n = n;
    pl->modulus = modulus;
    pl->primes = primes;
    for (uint64_t f : primes) {
        if (f < ((uint64_t)1 << 32)) {
            cntt_plan32 *sub = nullptr;
            if (int rc = plan_new<uint32_t, cntt_plan32>(n, (uint32_t)f, &sub)) return rc;
            pl->p32.emplace_back(sub);
        } else {
            cntt_plan64 *sub = nullptr;
            if (int rc = plan_new<uint64_t, cntt_plan64>(n, f, &sub)) return rc;
            pl->p64.emplace_back(sub);
        }
    }
    ProductArgs &A = pl->args;
    A.n32 = (int)pl->p32.size();
    A.n64 = (int)pl->p64.size();
    A.modulus = modulus;
    for (size_t j = 0; j < primes.size(); ++j) {
        A.prime[j] = primes[j];
        A.barrett[j] = (uint64_t)((((u128)1) << 64) / primes[j]);
        for (size_t i = 0; i < j; ++i) {  // every factor is prime here, so Fermat gives the Euclid inverse of :22-64
            const uint64_t inv = host::powmod(primes[i] % primes[j], primes[j] - 2, primes[j]);
            pl->modular_inverses.push_back(inv);
            A.inv[j * (j - 1) / 2 + i] = inv;
            A.inv_shoup[j * (j - 1) / 2 + i] = (uint64_t)((((u128)inv) << 64) / primes[j]);
        }
    }
    *out = pl.release();
    return CNTT_OK;
}
extern "C" cntt_product_t *cntt_product_plan_clone(const cntt_product_t *pl) {
    return pl ? new (std::nothrow) cntt_product(*pl) : nullptr;  // prime plans are immutable and shared
}
extern "C" void cntt_product_plan_free(cntt_product_t *pl) { delete pl; }
extern "C" size_t cntt_product_ntt_size(const cntt_product_t *pl) { return pl ? pl->n : 0; }
extern "C" uint64_t cntt_product_modulus(const cntt_product_t *pl) { return pl ? pl->modulus : 0; }
extern "C" size_t cntt_product_ntt_domain_len(const cntt_product_t *pl) { return pl ? pl->domain_len() : 0; }
extern "C" int cntt_product_nprimes32(const cntt_product_t *pl) { return pl ? (int)pl->p32.size() : 0; }
extern "C" int cntt_product_nprimes64(const cntt_product_t *pl) { return pl ? (int)pl->p64.size() : 0; }
extern "C" uint64_t cntt_product_prime(const cntt_product_t *pl, int i) {
    return (pl && i >= 0 && (size_t)i < pl->primes.size()) ? pl->primes[(size_t)i] : 0;
}
extern "C" const cntt_plan32_t *cntt_product_ntt32(const cntt_product_t *pl, int i) {
    return (pl && i >= 0 && (size_t)i < pl->p32.size()) ? pl->p32[(size_t)i].get() : nullptr;
}
extern "C" const cntt_plan64_t *cntt_product_ntt64(const cntt_product_t *pl, int i) {
    return (pl && i >= 0 && (size_t)i < pl->p64.size()) ? pl->p64[(size_t)i].get() : nullptr;
}
extern "C" int cntt_product_modular_inverses(const cntt_product_t *pl, uint64_t *out, size_t len) {
    if (!pl || (!out && len)) return fail(CNTT_EINVAL, "NULL argument");
    if (len != pl->modular_inverses.size()) return fail(CNTT_ELEN, "expected %zu inverses", pl->modular_inverses.size());
    std::copy(pl->modular_inverses.begin(), pl->modular_inverses.end(), out);
    return CNTT_OK;
}

// plane-major device views of a batched NTT-domain buffer (see aux_kernels.hpp)
struct ProductView {
    uint32_t *r32;
    uint64_t *r64;
};
static ProductView product_view(const cntt_product *pl, uint64_t *ntt, size_t batch) {
    return {reinterpret_cast<uint32_t *>(ntt), ntt + pl->len32() * batch};
}
static int product_ntt_device(const cntt_product *pl, ProductView v, size_t batch, bool inv, hipStream_t st) {
    const size_t count = batch * pl->n;
    for (size_t k = 0; k < pl->p32.size(); ++k)
        if (int rc = ntt_device<uint32_t>(pl->p32[k].get(), v.r32 + k * count, batch, inv, st)) return rc;
    for (size_t k = 0; k < pl->p64.size(); ++k)
        if (int rc = ntt_device<uint64_t>(pl->p64[k].get(), v.r64 + k * count, batch, inv, st)) return rc;
    return CNTT_OK;
}

// residue split of `batch` polynomials into the plane-major view v (the first half of Plan::fwd, src/product.rs:282-355)
static int product_split_device(const cntt_product *pl, ProductView v, const uint64_t *standard, size_t batch, bool bounded,
                                uint64_t bound, hipStream_t st) {
    const size_t count = batch * pl->n, k = pl->primes.size();
    if (count == 0 || k == 0) return CNTT_OK;
    ProductArgs A = pl->args;
    A.bound = bound;
    const dim3 grid(ew_grid(count / 2)), block(256);
    if (k == 1)
        hipLaunchKernelGGL((product_split_kernel<2>), grid, block, 0, st, v.r32, v.r64, standard, A, count);
    else if (A.n32 == 2 && A.n64 == 0 && bounded && bound < A.prime[0] && bound < A.prime[1])
        hipLaunchKernelGGL((product_split_kernel<1>), grid, block, 0, st, v.r32, v.r64, standard, A, count);
    else
        hipLaunchKernelGGL((product_split_kernel<0>), grid, block, 0, st, v.r32, v.r64, standard, A, count);
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}

// u32x2 plans whose primes share an arithmetic class: split + both forward transforms, or both inverse transforms +
// Garner, in one kernel (product_fused.hpp).  Returns hipErrorNotSupported when the plan / size is not covered.
static hipError_t product_fused2_try(const cntt_product *pl, bool inv, uint64_t *standard, uint32_t *res32, size_t batch,
                                     bool flag, hipStream_t st, int *rc_out) {
    if (pl->p32.size() != 2 || !pl->p64.empty() || batch == 0 || batch >= ((size_t)1 << 32)) return hipErrorNotSupported;
    // Round 3: with the element-wise kernels on uncapped grids the composed forward (split kernel + two batched transforms) is
    // 8 % faster than the fused forward kernel (N = 2048, 32768 polynomials: 0.497 vs 0.542 ms) -- the fused one reads its
    // twiddles from L2 at three wavefronts per SIMD, the batched transforms from an LDS image -- while the fused inverse
    // (two transforms + Garner, no residue round trip) still wins (Replace 0.445 vs 0.522 ms; Accumulate 0.599 vs 0.582: a
    // tie).  cntt_debug_set("product_fused", 0 / 1) forces neither / both for A/B timing; results are identical
    // (tests/test_gpu_switch_settings.py: test_gpu_product_fused_settings runs every call under -1, 0 and 1 against the oracle).
    const int force = debug_switch(DBG_PRODUCT_FUSED);
    if (force == 0 || (force < 0 && !inv)) return hipErrorNotSupported;
    const cntt_plan32 *q0 = pl->p32[0].get(), *q1 = pl->p32[1].get();
    const int cls = transform_class(q0);  // both primes above 2^31 (the reference's fast-path shape): CLS_FPW
    if (cls != transform_class(q1)) return hipErrorNotSupported;
    ProductFusedTables F{};
    for (int i = 0; i < 2; ++i) {
        DeviceTables<uint32_t> t;
        if (int rc = device_tables(pl->p32[(size_t)i].get(), &t)) {
            *rc_out = rc;
            return hipErrorUnknown;
        }
        F.twf[i] = alt_tables(cls) ? t.fwd_fp : t.fwd;
        F.twi[i] = alt_tables(cls) ? t.inv_fp : t.inv;
        F.P[i] = pl->p32[(size_t)i]->mp;
    }
    return launch_product_fused2(q0->logn, cls, inv, standard, res32, &F, pl->args, (uint32_t)batch, flag, st);
}

// Plan::fwd src/product.rs:273-357  (device pointers)
static int product_fwd_device(const cntt_product *pl, uint64_t *ntt, const uint64_t *standard, size_t batch,
                              bool bounded, uint64_t bound, hipStream_t st) {
    if (batch == 0 || pl->primes.empty()) return CNTT_OK;
    const ProductView v = product_view(pl, ntt, batch);
    {
        int rc = CNTT_OK;
        const bool fast = bounded && pl->p32.size() == 2 && bound < pl->args.prime[0] && bound < pl->args.prime[1];
        const hipError_t e = product_fused2_try(pl, false, const_cast<uint64_t *>(standard), v.r32, batch, fast, st, &rc);
        if (rc != CNTT_OK) return rc;
        if (e == hipSuccess) return CNTT_OK;
        if (e != hipErrorNotSupported) return fail(CNTT_EDEVICE, "fused product forward launch failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
    }
    if (int rc = product_split_device(pl, v, standard, batch, bounded, bound, st)) return rc;
    return product_ntt_device(pl, v, batch, false, st);
}

template <int K>
static void launch_product_crt(uint64_t *standard, ProductView v, const ProductArgs &A, size_t count, int acc,
                               hipStream_t st) {
    const dim3 grid(ew_grid(count / 2)), block(256);
    if (acc == 0) hipLaunchKernelGGL((product_crt_kernel<K, 0>), grid, block, 0, st, standard, v.r32, v.r64, A, count);
    else if (acc == 1) hipLaunchKernelGGL((product_crt_kernel<K, 1>), grid, block, 0, st, standard, v.r32, v.r64, A, count);
    else hipLaunchKernelGGL((product_crt_kernel<K, 2>), grid, block, 0, st, standard, v.r32, v.r64, A, count);
}

// Garner recombination of `batch` polynomials from the plane-major view v (the second half of Plan::inv, src/product.rs:386-879)
static int product_crt_device(const cntt_product *pl, uint64_t *standard, ProductView v, size_t batch, bool accumulate,
                              hipStream_t st) {
    const size_t count = batch * pl->n, k = pl->primes.size();
    if (count == 0) return CNTT_OK;
    const int acc = !accumulate ? 0 : (k == 1 && pl->p32.size() == 1 ? 2 : 1);
    switch (k) {
    case 1: launch_product_crt<1>(standard, v, pl->args, count, acc, st); break;
    case 2: launch_product_crt<2>(standard, v, pl->args, count, acc, st); break;
    case 3: launch_product_crt<3>(standard, v, pl->args, count, acc, st); break;
    case 4: launch_product_crt<4>(standard, v, pl->args, count, acc, st); break;
    case 5: launch_product_crt<5>(standard, v, pl->args, count, acc, st); break;
    case 6: launch_product_crt<6>(standard, v, pl->args, count, acc, st); break;
    default: launch_product_crt<7>(standard, v, pl->args, count, acc, st); break;
    }
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}

// Plan::inv src/product.rs:360-879  (device pointers)
static int product_inv_device(const cntt_product *pl, uint64_t *standard, uint64_t *ntt, size_t batch, bool accumulate,
                              hipStream_t st) {
    const size_t count = batch * pl->n;
    if (count == 0) return CNTT_OK;
    if (pl->primes.empty()) {  // src/product.rs:378-384
        if (!accumulate) HIP_TRY(hipMemsetAsync(standard, 0, count * 8, st));
        return CNTT_OK;
    }
    const ProductView v = product_view(pl, ntt, batch);
    {
        int rc = CNTT_OK;
        const hipError_t e = product_fused2_try(pl, true, standard, v.r32, batch, accumulate, st, &rc);
        if (rc != CNTT_OK) return rc;
        if (e == hipSuccess) return CNTT_OK;
        if (e != hipErrorNotSupported) return fail(CNTT_EDEVICE, "fused product inverse launch failed: %s", hipGetErrorString(e));
        (void)hipGetLastError();
    }
    if (int rc = product_ntt_device(pl, v, batch, true, st)) return rc;
    return product_crt_device(pl, standard, v, batch, accumulate, st);
}

// The external-product step of the reference's caller at the product::Plan level (device pointers):
//     for j { plan.fwd(t_j, terms[b][j], fwd_mode); for o { plan.mul_accumulate(acc_o, t_j, key[j][o]) } }
//     for o { plan.inv(out[b][o], acc_o, inv_mode) }
// = residue split of all terms, one fused mul_accumulate chain per prime plane, one Garner recombination.
static int product_external_product_device(const cntt_product *pl, uint64_t *out, const uint64_t *terms, const uint64_t *key,
                                           size_t nterms, size_t nout, size_t batch, bool bounded, uint64_t bound,
                                           bool accumulate, hipStream_t st) {
    if (batch == 0 || nout == 0) return CNTT_OK;
    const size_t n = pl->n, dl = pl->domain_len();
    if (pl->primes.empty() || nterms == 0) {
        if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, batch * nout * n * 8, st));
        return CNTT_OK;
    }
    if (pl->primes.size() == 1 && pl->p64.size() == 1)
        // u64x1 plan: fwd copies (src/product.rs:282-286) and inv copies / add_mod_u64s (:386-398), so the per-prime
        // chain reads `terms` and writes `out` directly -- no residue buffers at all
        return external_product_device<uint64_t>(pl->p64[0].get(), out, terms, key, nterms, nout, batch, accumulate, st);
    const size_t tpolys = batch * nterms, opolys = batch * nout, kpolys = nterms * nout;
    StreamBlock scratch(st);
    if (int rc = scratch.alloc((tpolys + opolys) * dl * 8)) return rc;
    uint64_t *tres = (uint64_t *)scratch.get(), *ores = tres + tpolys * dl;
    const ProductView tv = product_view(pl, tres, tpolys), ov = product_view(pl, ores, opolys);
    const ProductView kv = product_view(pl, const_cast<uint64_t *>(key), kpolys);
    int rc = product_split_device(pl, tv, terms, tpolys, bounded, bound, st);
    for (size_t i = 0; i < pl->p32.size() && rc == CNTT_OK; ++i)
        rc = external_product_device<uint32_t>(pl->p32[i].get(), ov.r32 + i * opolys * n, tv.r32 + i * tpolys * n,
                                               kv.r32 + i * kpolys * n, nterms, nout, batch, false, st);
    for (size_t i = 0; i < pl->p64.size() && rc == CNTT_OK; ++i)
        rc = external_product_device<uint64_t>(pl->p64[i].get(), ov.r64 + i * opolys * n, tv.r64 + i * tpolys * n,
                                               kv.r64 + i * kpolys * n, nterms, nout, batch, false, st);
    if (rc == CNTT_OK) rc = product_crt_device(pl, out, ov, opolys, accumulate, st);
    return rc;
}

// op 2 mul_assign_normalize, 3 normalize, 4 mul_accumulate, per prime on the plane-major layout: src/product.rs:885-966
static int product_pointwise_device(const cntt_product *pl, int op, uint64_t *a, const uint64_t *b, const uint64_t *c,
                                    size_t batch, hipStream_t st) {
    const size_t count = batch * pl->n;
    if (count == 0) return CNTT_OK;
    const size_t off64 = pl->len32() * batch;
    for (size_t k = 0; k < pl->p32.size() + pl->p64.size(); ++k) {
        int rc;
        if (k < pl->p32.size()) {
            const cntt_plan32 *sub = pl->p32[k].get();
            uint32_t *pa = reinterpret_cast<uint32_t *>(a) + k * count;
            const uint32_t *pb = b ? reinterpret_cast<const uint32_t *>(b) + k * count : nullptr;
            const uint32_t *pc = c ? reinterpret_cast<const uint32_t *>(c) + k * count : nullptr;
            rc = op == 2   ? pointwise_device<uint32_t, PW_MUL_NORMALIZE>(sub, pa, pb, nullptr, count, st)
                 : op == 3 ? pointwise_device<uint32_t, PW_NORMALIZE>(sub, pa, nullptr, nullptr, count, st)
                           : pointwise_device<uint32_t, PW_MUL_ACCUMULATE>(sub, pa, pb, pc, count, st);
        } else {
            const size_t o = off64 + (k - pl->p32.size()) * count;
            const cntt_plan64 *sub = pl->p64[k - pl->p32.size()].get();
            rc = op == 2   ? pointwise_device<uint64_t, PW_MUL_NORMALIZE>(sub, a + o, b + o, nullptr, count, st)
                 : op == 3 ? pointwise_device<uint64_t, PW_NORMALIZE>(sub, a + o, nullptr, nullptr, count, st)
                           : pointwise_device<uint64_t, PW_MUL_ACCUMULATE>(sub, a + o, b + o, c + o, count, st);
        }
        if (rc) return rc;
    }
    return CNTT_OK;
}

// op: 0 fwd (a = ntt out, b = standard in), 1 inv (a = standard, b = ntt, both written),
//     2 mul_assign_normalize (a lhs, b rhs), 3 normalize (a), 4 mul_accumulate (a acc, b lhs, c rhs)
static int product_op(const cntt_product *pl, int op, uint64_t *a, uint64_t *b, const uint64_t *c, size_t batch, int mode,
                      uint64_t bound, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch == 0) return CNTT_OK;
    if (batch * pl->n >= ((size_t)1 << 40)) return fail(CNTT_EINVAL, "batch too large");
    const size_t std_words = batch * pl->n, dom_words = batch * pl->domain_len();
    const size_t aw = op == 1 ? std_words : dom_words, bw = op == 0 ? std_words : dom_words;
    if ((!a && aw) || (op != 3 && !b && bw) || (op == 4 && !c && dom_words)) return fail(CNTT_EINVAL, "NULL buffer");
    {   // inv writes both of its buffers; lhs and rhs of mul_accumulate are read only and may be one buffer (include/cntt.h, "Operands")
        static const char *const NAMES[5][3] = {{"ntt", "standard"}, {"standard", "ntt"}, {"lhs", "rhs"}, {"values"}, {"acc", "lhs", "rhs"}};
        const Operand ops[3] = {{NAMES[op][0], a, aw * 8, 8, true},
                                {NAMES[op][1], b, op == 3 ? 0 : bw * 8, 8, op == 1},
                                {NAMES[op][2], c, op == 4 ? dom_words * 8 : 0, 8, false}};
        if (int rc = check_operands(ops, 3)) return rc;
    }
    // a: read unless the op only writes it (fwd; inv replacing), written back unless inv accumulates onto it with no primes at all
    const bool a_in = op != 0 && !(op == 1 && mode == 0), a_out = !(op == 1 && mode != 0 && pl->primes.empty());
    Staging s(where, st);
    uint64_t *da = (uint64_t *)(a_in && a_out ? s.inout(a, aw * 8) : a_in ? s.in(a, aw * 8) : s.out(a, aw * 8));
    // inv leaves the inverse-transformed residues in the caller's ntt buffer: src/product.rs:368-373
    uint64_t *db = (uint64_t *)(op == 3 ? nullptr : op == 1 ? s.inout(b, bw * 8) : s.in(b, bw * 8));
    const uint64_t *dc = op == 4 ? (const uint64_t *)s.in(c, dom_words * 8) : nullptr;
    if (int rc = s.status()) return rc;
    if (int rc = op == 0   ? product_fwd_device(pl, da, db, batch, mode != 0, bound, st)
                 : op == 1 ? product_inv_device(pl, da, db, batch, mode != 0, st)
                           : product_pointwise_device(pl, op, da, db, dc, batch, st))
        return rc;
    return s.finish();
}

#define PRODUCT_LEN(have, want, what)                                                                          \
    if ((have) != (want)) return fail(CNTT_ELEN, "assert_eq!(" what "): %zu != %zu", (size_t)(have), (size_t)(want))

extern "C" int cntt_product_fwd(const cntt_product_t *pl, uint64_t *ntt, size_t ntt_len, const uint64_t *standard,
                                size_t standard_len, cntt_fwd_mode_t mode, uint64_t bound) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    PRODUCT_LEN(standard_len, pl->n, "standard.len(), ntt_size");
    PRODUCT_LEN(ntt_len, pl->domain_len(), "ntt.len(), ntt_domain_len");
    return product_op(pl, 0, ntt, const_cast<uint64_t *>(standard), nullptr, 1, (int)mode, bound, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_product_inv(const cntt_product_t *pl, uint64_t *standard, size_t standard_len, uint64_t *ntt,
                                size_t ntt_len, cntt_inv_mode_t mode) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    PRODUCT_LEN(standard_len, pl->n, "standard.len(), ntt_size");
    PRODUCT_LEN(ntt_len, pl->domain_len(), "ntt.len(), ntt_domain_len");
    return product_op(pl, 1, standard, ntt, nullptr, 1, (int)mode, 0, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_product_mul_assign_normalize(const cntt_product_t *pl, uint64_t *lhs, size_t lhs_len,
                                                 const uint64_t *rhs, size_t rhs_len) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    PRODUCT_LEN(lhs_len, pl->domain_len(), "lhs.len(), ntt_domain_len");
    PRODUCT_LEN(rhs_len, pl->domain_len(), "rhs.len(), ntt_domain_len");
    return product_op(pl, 2, lhs, const_cast<uint64_t *>(rhs), nullptr, 1, 0, 0, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_product_normalize(const cntt_product_t *pl, uint64_t *values, size_t len) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    PRODUCT_LEN(len, pl->domain_len(), "values.len(), ntt_domain_len");
    return product_op(pl, 3, values, nullptr, nullptr, 1, 0, 0, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_product_mul_accumulate(const cntt_product_t *pl, uint64_t *acc, size_t acc_len, const uint64_t *lhs,
                                           size_t lhs_len, const uint64_t *rhs, size_t rhs_len) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    PRODUCT_LEN(lhs_len, pl->domain_len(), "lhs.len(), ntt_domain_len");
    PRODUCT_LEN(rhs_len, pl->domain_len(), "rhs.len(), ntt_domain_len");
    PRODUCT_LEN(acc_len, pl->domain_len(), "acc.len(), ntt_domain_len");
    return product_op(pl, 4, acc, const_cast<uint64_t *>(lhs), rhs, 1, 0, 0, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_product_fwd_batch(const cntt_product_t *pl, uint64_t *ntt, const uint64_t *standard, size_t batch,
                                      cntt_fwd_mode_t mode, uint64_t bound, cntt_mem_t where, void *stream) {
    return product_op(pl, 0, ntt, const_cast<uint64_t *>(standard), nullptr, batch, (int)mode, bound, where, (hipStream_t)stream);
}
extern "C" int cntt_product_inv_batch(const cntt_product_t *pl, uint64_t *standard, uint64_t *ntt, size_t batch,
                                      cntt_inv_mode_t mode, cntt_mem_t where, void *stream) {
    return product_op(pl, 1, standard, ntt, nullptr, batch, (int)mode, 0, where, (hipStream_t)stream);
}
extern "C" int cntt_product_mul_assign_normalize_batch(const cntt_product_t *pl, uint64_t *lhs, const uint64_t *rhs,
                                                       size_t batch, cntt_mem_t where, void *stream) {
    return product_op(pl, 2, lhs, const_cast<uint64_t *>(rhs), nullptr, batch, 0, 0, where, (hipStream_t)stream);
}
extern "C" int cntt_product_normalize_batch(const cntt_product_t *pl, uint64_t *values, size_t batch, cntt_mem_t where,
                                            void *stream) {
    return product_op(pl, 3, values, nullptr, nullptr, batch, 0, 0, where, (hipStream_t)stream);
}
extern "C" int cntt_product_mul_accumulate_batch(const cntt_product_t *pl, uint64_t *acc, const uint64_t *lhs,
                                                 const uint64_t *rhs, size_t batch, cntt_mem_t where, void *stream) {
    return product_op(pl, 4, acc, const_cast<uint64_t *>(lhs), rhs, batch, 0, 0, where, (hipStream_t)stream);
}

extern "C" int cntt_product_external_product_batch(const cntt_product_t *pl, uint64_t *out, const uint64_t *terms,
                                                   const uint64_t *key_ntt, size_t nterms, size_t nout, size_t batch,
                                                   cntt_fwd_mode_t fwd_mode, uint64_t bound, cntt_inv_mode_t inv_mode,
                                                   cntt_mem_t where, void *stream) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch == 0 || nout == 0) return CNTT_OK;
    const size_t n = pl->n, dl = pl->domain_len();
    if (!out || (nterms && (!terms || (dl && !key_ntt)))) return fail(CNTT_EINVAL, "NULL buffer");
    if (batch * std::max(nterms, nout) * n >= ((size_t)1 << 40)) return fail(CNTT_EINVAL, "batch too large");
    hipStream_t st = (hipStream_t)stream;
    const bool bounded = fwd_mode == CNTT_FWD_BOUNDED, accumulate = inv_mode == CNTT_INV_ACCUMULATE;
    const size_t ob = batch * nout * n * 8, tb = batch * nterms * n * 8, kb = nterms * nout * dl * 8;
    const Operand ops[3] = {{"out", out, ob, 8, true}, {"terms", terms, tb, 8, false}, {"key_ntt", key_ntt, kb, 8, false}};
    if (int rc = check_operands(ops, 3)) return rc;
    Staging s(where, st);
    uint64_t *dout = (uint64_t *)(accumulate ? s.inout(out, ob) : s.out(out, ob));
    const uint64_t *dt = (const uint64_t *)s.in(terms, tb), *dk = (const uint64_t *)s.in(key_ntt, kb);
    if (int rc = s.status()) return rc;
    if (int rc = product_external_product_device(pl, dout, dt, dk, nterms, nout, batch, bounded, bound, accumulate, st)) return rc;
    return s.finish();
}
