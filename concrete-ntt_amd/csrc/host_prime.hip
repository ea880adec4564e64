// libcntt_hip.so host side, prime plans: plan construction, the per-device twiddle tables and every launcher of the transforms,
// the pointwise kernels and the mul_accumulate chain; the C ABI of prime32 / prime64 (include/cntt.h).  The native and product
// plans (host_native*.hip, host_product.hip) run their per-prime steps through the launchers instantiated at the end of this file.
#include <map>

#include "aux_kernels.hpp"
#include "host_common.hpp"

template <class T> struct DeviceCache {
    std::mutex mu;
    std::map<int, DeviceTables<T>> per_device;
    ~DeviceCache() {
        for (auto &kv : per_device) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) continue;
            (void)hipSetDevice(kv.first);
            (void)hipFree(kv.second.fwd);
            (void)hipFree(kv.second.inv);
            (void)hipFree(kv.second.fwd_fp);
            (void)hipFree(kv.second.inv_fp);
            (void)hipFree(kv.second.mono);
            (void)hipSetDevice(cur);
        }
    }
};

// Plan::try_new  (src/prime64.rs:704-771, src/prime32.rs:630-686)
template <class T, class PlanT> int plan_new(size_t n, T p, PlanT **out) {
    constexpr int B = sizeof(T) * 8;
    if (!out) return fail(CNTT_EINVAL, "out is NULL");
    *out = nullptr;
    if (p <= 1) return fail(CNTT_EINVAL, "modulus <= 1: the reference panics in Div%d::new (src/fastdiv.rs)", B);
    const size_t min_n = (B == 64) ? 16 : 32;
    if (n < min_n || (n & (n - 1)) != 0) return fail(CNTT_NONE, "polynomial_size must be a power of two >= %zu", min_n);
    if (n > ((size_t)1 << 30)) return fail(CNTT_NONE, "polynomial_size too large");
    if (!host::is_prime((uint64_t)p)) return fail(CNTT_NONE, "modulus is not prime");
    uint64_t w = 0;
    if (!host::primitive_root((uint64_t)p, 2 * (uint64_t)n, &w))
        return fail(CNTT_NONE, "no primitive 2n-th root of unity modulo the modulus");

    PlanT *pl = new (std::nothrow) PlanT();
    if (!pl) return fail(CNTT_ENOMEM, "out of memory");
    pl->n = n;
    pl->p = p;
    pl->root = w;
    while (((size_t)1 << pl->logn) < n) ++pl->logn;
    pl->has_shoup = (uint64_t)p < ((uint64_t)1 << (B - 1));
    pl->twid.assign(n, 0);
    pl->inv_twid.assign(n, 0);
    if (pl->has_shoup) {
        pl->twid_shoup.assign(n, 0);
        pl->inv_twid_shoup.assign(n, 0);
    }
    // twid[bitrev(k)] = w^k ; inv_twid[bitrev((n-k) mod n)] = (k == 0 ? 1 : p - w^k)
    uint64_t wk = 1;
    for (size_t k = 0; k < n; ++k) {
        const size_t fi = host::bit_reverse((uint32_t)pl->logn, (uint32_t)k);
        const size_t ii = host::bit_reverse((uint32_t)pl->logn, (uint32_t)((n - k) % n));
        const T x = (k == 0) ? (T)wk : (T)(p - (T)wk);
        pl->twid[fi] = (T)wk;
        pl->inv_twid[ii] = x;
        if (pl->has_shoup) {
            pl->twid_shoup[fi] = shoup_of<T>((T)wk, p);
            pl->inv_twid_shoup[ii] = shoup_of<T>(x, p);
        }
        wk = host::mulmod(wk, w, (uint64_t)p);
    }
    pl->n_inv = (T)host::powmod((uint64_t)n % p, (uint64_t)p - 2, (uint64_t)p);
    pl->n_inv_shoup = shoup_of<T>(pl->n_inv, p);
    uint32_t ilog = 0;
    while (ilog + 1 < (uint32_t)B && (((uint64_t)p) >> (ilog + 1)) != 0) ++ilog;
    pl->big_q = ilog + 1;
    {
        const uint32_t big_l = pl->big_q + (B - 1);
        pl->p_barrett = (T)((((u128)1) << big_l) / p);  // unused garbage when p >= 2^(B-1), as in the reference
        if (big_l >= 128) pl->p_barrett = 0;
    }
    // device-side parameters
    ModParams<T> &mp = pl->mp;
    mp.p = p;
    mp.neg_p = (T)0 - p;
    mp.two_p = (T)(2 * p);
    mp.neg_two_p = (T)0 - (T)(2 * p);
    mp.big_q = pl->big_q;
    mp.p_barrett = pl->p_barrett;
    const uint64_t p64 = (uint64_t)p;
    if (p64 < ((uint64_t)1 << (B - 2)))
        mp.cls = CLS_LAZY;
    else if (p64 < ((uint64_t)1 << (B - 1)))
        mp.cls = CLS_STRICT;
    else
        mp.cls = CLS_GENERIC;
    mp.pinv_neg = (T)host::neg_inv_pow2(p64);
    const u128 R = ((u128)1) << B;
    const uint64_t r1 = (uint64_t)(R % p64);
    const uint64_t r2 = host::mulmod(r1, r1, p64);
    mp.r2 = (T)r2;
    const uint64_t w_last = host::mulmod((uint64_t)pl->inv_twid[1], (uint64_t)pl->n_inv, p64);  // inv_twid[1] / N
    if (mp.cls == CLS_GENERIC) {
        mp.n_inv = (T)host::mulmod((uint64_t)pl->n_inv, r2, p64);  // N^-1 * R^2 (see mul_normalize)
        mp.n_inv_shoup = 0;
        mp.last_w = (T)host::mulmod(w_last, r2, p64);
        mp.last_w_shoup = 0;
    } else {
        mp.n_inv = pl->n_inv;
        mp.n_inv_shoup = pl->n_inv_shoup;
        mp.last_w = (T)w_last;
        mp.last_w_shoup = shoup_of<T>((T)w_last, p);
        // the same two constants times 2^B: the fused product kernels of the lazy class multiply pointwise with a Montgomery product
        // (ntt_arith.hpp mul_fused), whose 2^-B is undone where 1/N is applied
        mp.mont_n_inv = (T)host::mulmod((uint64_t)pl->n_inv, r1, p64);
        mp.mont_n_inv_shoup = shoup_of<T>(mp.mont_n_inv, p);
        mp.mont_last_w = (T)host::mulmod(w_last, r1, p64);
        mp.mont_last_w_shoup = shoup_of<T>(mp.mont_last_w, p);
        mp.mont_r = (T)r1;   // the fused mul_accumulate chains multiply their accumulators by 2^B once (ntt_arith.hpp chain_pre_inverse)
        mp.mont_r_shoup = shoup_of<T>(mp.mont_r, p);
    }
    // CLS_FP / CLS_FP51: 64-bit words, p < 2^50 / 2^51 (the classes of src/prime64/less_than_50bit.rs and
    // less_than_51bit.rs).  cntt_debug_set("fp", 0) keeps such plans on the integer butterflies (A/B measurements, and tests
    // that compare the two paths).
    mp.fp = 0;
    if constexpr (B == 64) {
        if (p64 < ((uint64_t)1 << 51) && debug_switch(DBG_FP) != 0) {
            mp.fp = p64 < ((uint64_t)1 << 50) ? (uint32_t)CLS_FP : (uint32_t)CLS_FP51;
            const double pd = (double)p64;
            mp.fp_p = host::double_bits(pd);
            mp.fp_pinv = host::double_bits(1.0 / pd);
            const double ni = host::centred(pl->n_inv, p64), wl = host::centred(w_last, p64);
            mp.fp_n_inv = host::double_bits(ni);
            mp.fp_n_inv_q = host::double_bits(ni / pd);
            mp.fp_last_w = host::double_bits(wl);
            mp.fp_last_w_q = host::double_bits(wl / pd);
        }
    }
    // CLS_FPW: 32-bit words, p >= 2^31 (no lazy headroom in 32 bits: the Montgomery class otherwise): the LDS-resident
    // transforms run on doubles (ntt_arith.hpp).  cntt_debug_set("fp", 0) keeps the Montgomery class here too.
    if constexpr (B == 32) {
        if (mp.cls == CLS_GENERIC && debug_switch(DBG_FP) != 0) {
            mp.fp = (uint32_t)CLS_FPW;
            const double pd = (double)p64;
            mp.fp_p = host::double_bits(pd);
            mp.fp_pinv = host::double_bits(1.0 / pd);
            const double ni = host::centred(pl->n_inv, p64), wl = host::centred(w_last, p64);
            mp.fp_n_inv = host::double_bits(ni);
            mp.fp_n_inv_q = host::double_bits(ni / pd);
            mp.fp_last_w = host::double_bits(wl);
            mp.fp_last_w_q = host::double_bits(wl / pd);
        }
    }
    // CLS_PM64: p = 2^64 - c with c < 2^32 (Solinas, and the largest primes below 2^64).  cntt_debug_set("pm64", 0) keeps the
    // Montgomery class (A/B measurements and tests).
    mp.pm_c = 0;
    if constexpr (B == 64) {
        const uint64_t c = (uint64_t)0 - p64;
        if (p64 >= ((uint64_t)1 << 63) && c < ((uint64_t)1 << 32) && debug_switch(DBG_PM64) != 0) {
            mp.pm_c = (uint32_t)c;
            mp.pm_n_inv = pl->n_inv;
            mp.pm_last_w = (T)w_last;
        }
    }
    pl->cache = std::make_shared<DeviceCache<T>>();
    *out = pl;
    return CNTT_OK;
}

// per-device table replica, created on first use under the cache mutex
template <class T> int device_tables(const PrimePlan<T> *pl, DeviceTables<T> *out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(pl->cache->mu);
    auto it = pl->cache->per_device.find(dev);
    if (it != pl->cache->per_device.end()) {
        *out = it->second;
        return CNTT_OK;
    }
    const size_t n = pl->n;
    std::vector<TwPair<T>> f(n), i(n);
    const uint64_t p64 = (uint64_t)pl->p;
    const uint64_t r1 = (uint64_t)((((u128)1) << (sizeof(T) * 8)) % p64);
    for (size_t k = 0; k < n; ++k) {
        if (pl->mp.cls == CLS_GENERIC) {  // Montgomery form
            f[k].w = (T)host::mulmod((uint64_t)pl->twid[k], r1, p64);
            f[k].ws = 0;
            i[k].w = (T)host::mulmod((uint64_t)pl->inv_twid[k], r1, p64);
            i[k].ws = 0;
        } else {
            f[k].w = pl->twid[k];
            f[k].ws = pl->twid_shoup[k];
            i[k].w = pl->inv_twid[k];
            i[k].ws = pl->inv_twid_shoup[k];
        }
    }
    DeviceTables<T> t;
    // every early return below (allocation or upload failure) releases what this call allocated so far
    struct Release {
        DeviceTables<T> *t;
        ~Release() {
            if (!t) return;
            (void)hipFree(t->fwd);
            (void)hipFree(t->inv);
            (void)hipFree(t->fwd_fp);
            (void)hipFree(t->inv_fp);
        }
    } release{&t};
    if (hipMalloc((void **)&t.fwd, n * sizeof(TwPair<T>)) != hipSuccess || hipMalloc((void **)&t.inv, n * sizeof(TwPair<T>)) != hipSuccess)
        return fail(CNTT_ENOMEM, "hipMalloc of the twiddle tables failed");
    HIP_TRY(hipMemcpy(t.fwd, f.data(), n * sizeof(TwPair<T>), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(t.inv, i.data(), n * sizeof(TwPair<T>), hipMemcpyHostToDevice));
    if (pl->mp.fp || pl->mp.pm_c) {
        const double pd = (double)p64;
        for (size_t k = 0; k < n; ++k) {
            if constexpr (sizeof(T) == 8) {
                if (pl->mp.fp) {
                    const double cf = host::centred((uint64_t)pl->twid[k], p64), ci = host::centred((uint64_t)pl->inv_twid[k], p64);
                    f[k].w = host::double_bits(cf);
                    f[k].ws = host::double_bits(cf / pd);
                    i[k].w = host::double_bits(ci);
                    i[k].ws = host::double_bits(ci / pd);
                } else {
                    f[k].w = pl->twid[k];
                    f[k].ws = 0;
                    i[k].w = pl->inv_twid[k];
                    i[k].ws = 0;
                }
            } else {  // CLS_FPW: the 8-byte entry is the centred twiddle as a double (w = low, ws = high word)
                (void)pd;
                const uint64_t bf = host::double_bits(host::centred((uint64_t)pl->twid[k], p64));
                const uint64_t bi = host::double_bits(host::centred((uint64_t)pl->inv_twid[k], p64));
                f[k].w = (T)bf;
                f[k].ws = (T)(bf >> 32);
                i[k].w = (T)bi;
                i[k].ws = (T)(bi >> 32);
            }
        }
        if (hipMalloc((void **)&t.fwd_fp, n * sizeof(TwPair<T>)) != hipSuccess ||
            hipMalloc((void **)&t.inv_fp, n * sizeof(TwPair<T>)) != hipSuccess)
            return fail(CNTT_ENOMEM, "hipMalloc of the twiddle tables failed");
        HIP_TRY(hipMemcpy(t.fwd_fp, f.data(), n * sizeof(TwPair<T>), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.inv_fp, i.data(), n * sizeof(TwPair<T>), hipMemcpyHostToDevice));
    }
    release.t = nullptr;  // the cache owns the tables from here
    pl->cache->per_device[dev] = t;
    *out = t;
    return CNTT_OK;
}

template <class T, bool INV, int CLS>
static void launch_global_stage(T *data, const TwPair<T> *tw, const ModParams<T> &P, uint32_t logn, uint32_t s,
                                size_t nb, bool finish, hipStream_t st) {
    hipLaunchKernelGGL((global_stage_kernel<T, INV, CLS>), dim3(ew_grid(nb)), dim3(256), 0, st, data, tw, P, logn, s, nb,
                       finish);
}
template <class T, bool INV>
static void global_stage(T *data, const TwPair<T> *tw, const ModParams<T> &P, uint32_t logn, uint32_t s, size_t nb,
                         bool finish, hipStream_t st) {
    switch (P.cls) {
    case CLS_LAZY: launch_global_stage<T, INV, CLS_LAZY>(data, tw, P, logn, s, nb, finish, st); break;
    case CLS_STRICT: launch_global_stage<T, INV, CLS_STRICT>(data, tw, P, logn, s, nb, finish, st); break;
    default: launch_global_stage<T, INV, CLS_GENERIC>(data, tw, P, logn, s, nb, finish, st); break;
    }
}

// batched transform on device memory
template <class T> int ntt_device(const PrimePlan<T> *pl, T *d, size_t batch, bool inv, hipStream_t st) {
    if (batch == 0) return CNTT_OK;
    DeviceTables<T> t;
    if (int rc = device_tables(pl, &t)) return rc;
    const int maxl = MaxLdsLogN<T>::value;
    const int depth = pl->logn > maxl ? pl->logn - maxl : 0;
    const int sub_logn = pl->logn - depth;
    if ((batch << depth) >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "batch too large for one launch");
    const uint32_t nsub = (uint32_t)(batch << depth);
    const size_t nbfly = batch * (pl->n / 2);
    const int tcls = transform_class(pl);
    // per-launch copy of the plan's parameters: a batch beyond STREAM_BYTES streams (ModParams::stream, ntt_kernel.hpp)
    ModParams<T> mp = pl->mp;
    mp.stream = batch * pl->n * sizeof(T) > STREAM_BYTES ? 1u : 0u;
    hipError_t e;
    if (depth == 1 && batch < ((size_t)1 << 32)) {
        // one size past the LDS-resident ones: a single-pass kernel exists for 64-bit words (Ntt32k), in the plan's
        // 64-bit-only class where it has one (those tables exist at every size)
        int c1 = tcls;
        if constexpr (sizeof(T) == 8) c1 = pl->mp.fp ? (int)pl->mp.fp : pl->mp.pm_c ? (int)CLS_PM64 : tcls;
        e = inv ? launch_ntt<T, true>(pl->logn, c1, d, alt_tables(c1) ? t.inv_fp : t.inv, mp, (uint32_t)batch, 0u, st)
                : launch_ntt<T, false>(pl->logn, c1, d, alt_tables(c1) ? t.fwd_fp : t.fwd, mp, (uint32_t)batch, 0u, st);
        if (e == hipSuccess) return CNTT_OK;
        (void)hipGetLastError();
        if (e != hipErrorNotSupported && e != hipErrorInvalidValue)
            return fail(CNTT_EDEVICE, "NTT kernel launch failed: %s", hipGetErrorString(e));
    }
    if (!inv) {
        for (int s = 0; s < depth; ++s) global_stage<T, false>(d, t.fwd, pl->mp, (uint32_t)pl->logn, (uint32_t)s, nbfly, false, st);
        e = launch_ntt<T, false>(sub_logn, tcls, d, alt_tables(tcls) ? t.fwd_fp : t.fwd, mp, nsub, (uint32_t)depth, st);
    } else {
        e = launch_ntt<T, true>(sub_logn, tcls, d, alt_tables(tcls) ? t.inv_fp : t.inv, mp, nsub, (uint32_t)depth, st);
        for (int s = depth - 1; s >= 0 && e == hipSuccess; --s)
            global_stage<T, true>(d, t.inv, pl->mp, (uint32_t)pl->logn, (uint32_t)s, nbfly, s == 0, st);
    }
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "NTT kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}

template <class T, int OP>
int pointwise_device(const PrimePlan<T> *pl, T *a, const T *b, const T *c, size_t count, hipStream_t st) {
    if (count == 0) return CNTT_OK;
    const size_t nv = count / (16 / sizeof(T)) + 1;
    // working set of the call against STREAM_BYTES: larger ones stream (non-temporal policy, aux_kernels.hpp)
    constexpr size_t NARR = OP == PW_NORMALIZE ? 1 : OP == PW_MUL_ACCUMULATE ? 3 : 2;
    if (NARR * count * sizeof(T) > STREAM_BYTES)
        hipLaunchKernelGGL((pointwise_kernel<T, OP, true>), dim3(ew_grid(nv)), dim3(256), 0, st, a, b, c, pl->mp, count);
    else
        hipLaunchKernelGGL((pointwise_kernel<T, OP, false>), dim3(ew_grid(nv)), dim3(256), 0, st, a, b, c, pl->mp, count);
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}

// fused lhs <- inv(mul_assign_normalize(fwd(lhs), rhs_ntt)); three launches when no fused kernel exists
template <class T> int mul_ntt_device(const PrimePlan<T> *pl, T *lhs, const T *rhs, size_t batch, hipStream_t st) {
    if (batch == 0) return CNTT_OK;
    if (batch >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "batch too large for one launch");
    DeviceTables<T> t;
    if (int rc = device_tables(pl, &t)) return rc;
    int tcls = transform_class(pl);
    // one size past the LDS-resident ones (64-bit words): the single-pass kernels run in the plan's 64-bit-only class where
    // it has one, like ntt_device
    if (sizeof(T) == 8 && pl->logn == MaxLdsLogN<T>::value + 1) tcls = pl->mp.fp ? (int)pl->mp.fp : pl->mp.pm_c ? (int)CLS_PM64 : tcls;
    const hipError_t e = launch_mul_ntt<T>(pl->logn, tcls, lhs, rhs, alt_tables(tcls) ? t.fwd_fp : t.fwd,
                                           alt_tables(tcls) ? t.inv_fp : t.inv, pl->mp, (uint32_t)batch, st);
    if (e == hipSuccess) return CNTT_OK;
    if (e != hipErrorNotSupported) return fail(CNTT_EDEVICE, "fused product launch failed: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    if (int rc = ntt_device<T>(pl, lhs, batch, false, st)) return rc;
    if (int rc = pointwise_device<T, PW_MUL_NORMALIZE>(pl, lhs, rhs, nullptr, batch * pl->n, st)) return rc;
    return ntt_device<T>(pl, lhs, batch, true, st);
}

// Three / four outputs of the fused mul_accumulate chain where only the one- / two-output kernels exist (64-bit words at n = 16384,
// 32-bit words at n = 32768): two fused launches of <= 2 outputs against the composed path, measured per class with J = 6
// (profiles/r04_chain_split.jsonl, ms per 1024 elements, split / composed):
//   u64 n = 16384   p < 2^50 (doubles)  0.99 / 1.48, 1.12 / 1.61     2^64 - c  1.77 / 2.00, 1.98 / 2.31     -> split
//                   62-bit  1.74 / 1.61, 1.98 / 1.88     63-bit  1.87 / 1.70, 2.16 / 1.99                     -> composed
//   u32 n = 32768   30-bit  1.45 / 1.61, 1.73 / 1.94                                                          -> split
//                   31-bit  1.70 / 1.75, 2.01 / 1.97     p >= 2^31 (doubles)  2.14 / 2.07, 2.58 / 2.48        -> composed
// cntt_debug_set("ext_split", 0) never splits, 1 always does (A/B runs); the decision of the call in flight sits in a thread-local because
// launch_ext_ntt() (ntt_launch.hpp) only asks ext_split_enabled().
static thread_local bool g_ext_split_wins = true;
static bool ext_split_wins(size_t word, int logn, int cls) {
    if (word == 8 && logn == 14) return cls == CLS_FP || cls == CLS_FP51 || cls == CLS_PM64;
    if (word == 4 && logn == 15) return cls == CLS_LAZY;
    return true;
}
bool cntt::ext_split_enabled() {
    const int mode = debug_switch(DBG_EXT_SPLIT);
    return mode < 0 ? g_ext_split_wins : mode == 1;
}
// mul_accumulate chain: out[b][o] (+)= inv(sum_j fwd(terms[b][j]) . key_ntt[j][o])  (device pointers).
// Fused kernel when the transform lives in one wavefront group and nout <= 4; otherwise composed from the batched
// kernels through a stream-ordered scratch allocation.
template <class T>
int external_product_device(const PrimePlan<T> *pl, T *out, const T *terms, const T *key, size_t nterms,
                                   size_t nout, size_t batch, bool accumulate, hipStream_t st) {
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (batch * std::max(nterms, nout) >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "batch too large for one launch");
    const size_t n = pl->n;
    if (nterms == 0) {  // empty sum
        if (!accumulate) HIP_TRY(hipMemsetAsync(out, 0, batch * nout * n * sizeof(T), st));
        return CNTT_OK;
    }
    DeviceTables<T> t;
    if (int rc = device_tables(pl, &t)) return rc;
    const int tcls = transform_class(pl);
    g_ext_split_wins = ext_split_wins(sizeof(T), pl->logn, tcls);
    const hipError_t e = launch_ext_ntt<T>(pl->logn, tcls, out, terms, key, alt_tables(tcls) ? t.fwd_fp : t.fwd,
                                           alt_tables(tcls) ? t.inv_fp : t.inv, pl->mp, (uint32_t)batch, (uint32_t)nterms,
                                           (uint32_t)nout, accumulate, st);
    if (e == hipSuccess) return CNTT_OK;
    if (e != hipErrorNotSupported) return fail(CNTT_EDEVICE, "fused mul_accumulate chain launch failed: %s", hipGetErrorString(e));
    (void)hipGetLastError();
    const size_t tw = batch * nterms * n, ow = batch * nout * n;
    StreamBlock scratch(st);
    if (int rc = scratch.alloc((tw + (accumulate ? ow : 0)) * sizeof(T))) return rc;
    T *tn = (T *)scratch.get(), *acc = accumulate ? tn + tw : out;
    if (hipMemcpyAsync(tn, terms, tw * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess) return fail(CNTT_EDEVICE, "device copy failed");
    if (int rc = ntt_device<T>(pl, tn, batch * nterms, false, st)) return rc;
    hipLaunchKernelGGL((ext_accumulate_kernel<T>), dim3(ew_grid(ow / (16 / sizeof(T)))), dim3(256), 0, st, acc, tn, key,
                       pl->mp, (uint32_t)pl->logn, (uint32_t)nterms, (uint32_t)nout, batch);
    if (hipGetLastError() != hipSuccess) return fail(CNTT_EDEVICE, "ext_accumulate_kernel launch failed");
    if (int rc = ntt_device<T>(pl, acc, batch * nout, true, st)) return rc;
    return accumulate ? pointwise_device<T, PW_ADD>(pl, out, acc, nullptr, ow, st) : CNTT_OK;
}

template <class T>
static int external_product(const PrimePlan<T> *pl, T *out, const T *terms, const T *key, size_t nterms, size_t nout,
                            size_t batch, int accumulate, cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (batch == 0 || nout == 0) return CNTT_OK;
    if (!out || (nterms && (!terms || !key))) return fail(CNTT_EINVAL, "NULL buffer");
    const size_t n = pl->n, ob = batch * nout * n * sizeof(T), tb = batch * nterms * n * sizeof(T), kb = nterms * nout * n * sizeof(T);
    const Operand ops[3] = {{"out", out, ob, sizeof(T), true}, {"terms", terms, tb, sizeof(T), false}, {"key_ntt", key, kb, sizeof(T), false}};
    if (int rc = check_operands(ops, 3)) return rc;
    Staging s(where, st);
    T *dout = (T *)(accumulate ? s.inout(out, ob) : s.out(out, ob));
    const T *dt = (const T *)s.in(terms, tb), *dk = (const T *)s.in(key, kb);
    if (int rc = s.status()) return rc;
    if (int rc = external_product_device<T>(pl, dout, dt, dk, nterms, nout, batch, accumulate != 0, st)) return rc;
    return s.finish();
}

// op: 0 fwd, 1 inv, 2 mul_assign_normalize, 3 normalize, 4 mul_accumulate, 5 mul_ntt ; count = total elements
template <class T>
static int prime_op_device(const PrimePlan<T> *pl, int op, T *a, const T *b, const T *c, size_t count, size_t batch, hipStream_t st) {
    switch (op) {
    case 0: return ntt_device<T>(pl, a, batch, false, st);
    case 1: return ntt_device<T>(pl, a, batch, true, st);
    case 2: return pointwise_device<T, PW_MUL_NORMALIZE>(pl, a, b, nullptr, count, st);
    case 3: return pointwise_device<T, PW_NORMALIZE>(pl, a, nullptr, nullptr, count, st);
    case 5: return mul_ntt_device<T>(pl, a, b, batch, st);
    default: return pointwise_device<T, PW_MUL_ACCUMULATE>(pl, a, b, c, count, st);
    }
}
template <class T>
static int prime_op(const PrimePlan<T> *pl, int op, T *a, const T *b, const T *c, size_t count, size_t batch,
                    cntt_mem_t where, hipStream_t st) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (count == 0) return CNTT_OK;
    if (!a || ((op == 2 || op == 5) && !b) || (op == 4 && (!b || !c))) return fail(CNTT_EINVAL, "NULL buffer");
    {   // the written operand first; lhs and rhs of mul_accumulate are read only and may be one buffer (include/cntt.h, "Operands")
        static const char *const NAMES[6][3] = {{"bufs"}, {"bufs"}, {"lhs", "rhs"}, {"values"}, {"acc", "lhs", "rhs"}, {"lhs", "rhs_ntt"}};
        const Operand ops[3] = {{NAMES[op][0], a, count * sizeof(T), sizeof(T), true},
                                {NAMES[op][1], b, b ? count * sizeof(T) : 0, sizeof(T), false},
                                {NAMES[op][2], c, c ? count * sizeof(T) : 0, sizeof(T), false}};
        if (int rc = check_operands(ops, 3)) return rc;
    }
    const size_t bytes = count * sizeof(T);
    Staging s(where, st);
    T *da = (T *)s.inout(a, bytes);
    const T *db = op == 2 || op == 4 || op == 5 ? (const T *)s.in(b, bytes) : nullptr;
    const T *dc = op == 4 ? (const T *)s.in(c, bytes) : nullptr;
    if (int rc = s.status()) return rc;
    if (int rc = prime_op_device<T>(pl, op, da, db, dc, count, batch, st)) return rc;
    return s.finish();
}

template <class T> static int plan_info(const PrimePlan<T> *pl, cntt_plan_info_t *out) {
    if (!pl || !out) return fail(CNTT_EINVAL, "NULL argument");
    out->ntt_size = pl->n;
    out->modulus = pl->p;
    out->p_barrett = pl->p_barrett;
    out->big_q = pl->big_q;
    out->n_inv_mod_p = pl->n_inv;
    out->n_inv_mod_p_shoup = pl->n_inv_shoup;
    out->root = pl->root;
    out->has_shoup = pl->has_shoup ? 1 : 0;
    out->arith_class = (int32_t)transform_class(pl);
    return CNTT_OK;
}
template <class T> static int plan_table(const PrimePlan<T> *pl, cntt_table_t which, T *out, size_t len) {
    if (!pl || !out) return fail(CNTT_EINVAL, "NULL argument");
    if (len != pl->n) return fail(CNTT_ELEN, "len %zu != ntt_size %zu", len, pl->n);
    const std::vector<T> *src = nullptr;
    switch (which) {
    case CNTT_TWID: src = &pl->twid; break;
    case CNTT_TWID_SHOUP: src = &pl->twid_shoup; break;
    case CNTT_INV_TWID: src = &pl->inv_twid; break;
    case CNTT_INV_TWID_SHOUP: src = &pl->inv_twid_shoup; break;
    default: return fail(CNTT_EINVAL, "unknown table");
    }
    if (src->empty()) return fail(CNTT_NONE, "the plan has no Shoup tables (modulus >= 2^(B-1))");
    std::memcpy(out, src->data(), len * sizeof(T));
    return CNTT_OK;
}

// ---- C ABI: prime64 ---------------------------------------------------------------------------
#define CNTT_PRIME_API(BITS, T, PLAN)                                                                               \
    extern "C" int cntt_prime##BITS##_plan_new(size_t n, T p, PLAN **out) { return plan_new<T, PLAN>(n, p, out); }  \
    extern "C" PLAN *cntt_prime##BITS##_plan_clone(const PLAN *pl) {                                                \
        if (!pl) return nullptr;                                                                                    \
        return new (std::nothrow) PLAN(*pl); /* host tables copied, immutable device replicas shared */             \
    }                                                                                                               \
    extern "C" void cntt_prime##BITS##_plan_free(PLAN *pl) { delete pl; }                                           \
    extern "C" size_t cntt_prime##BITS##_ntt_size(const PLAN *pl) { return pl ? pl->n : 0; }                        \
    extern "C" T cntt_prime##BITS##_modulus(const PLAN *pl) { return pl ? pl->p : 0; }                              \
    extern "C" int cntt_prime##BITS##_plan_info(const PLAN *pl, cntt_plan_info_t *out) { return plan_info<T>(pl, out); } \
    extern "C" int cntt_prime##BITS##_plan_table(const PLAN *pl, cntt_table_t w, T *out, size_t len) {              \
        return plan_table<T>(pl, w, out, len);                                                                      \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_fwd(const PLAN *pl, T *buf, size_t len) {                                     \
        if (!pl) return fail(CNTT_EINVAL, "plan is NULL");                                                          \
        if (len != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", len, pl->n);        \
        return prime_op<T>(pl, 0, buf, nullptr, nullptr, len, 1, CNTT_MEM_HOST, nullptr);                           \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_inv(const PLAN *pl, T *buf, size_t len) {                                     \
        if (!pl) return fail(CNTT_EINVAL, "plan is NULL");                                                          \
        if (len != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", len, pl->n);        \
        return prime_op<T>(pl, 1, buf, nullptr, nullptr, len, 1, CNTT_MEM_HOST, nullptr);                           \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_mul_assign_normalize(const PLAN *pl, T *lhs, size_t ll, const T *rhs, size_t rl) { \
        return prime_op<T>(pl, 2, lhs, rhs, nullptr, std::min(ll, rl), 0, CNTT_MEM_HOST, nullptr);                  \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_normalize(const PLAN *pl, T *v, size_t len) {                                 \
        return prime_op<T>(pl, 3, v, nullptr, nullptr, len, 0, CNTT_MEM_HOST, nullptr);                             \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_mul_accumulate(const PLAN *pl, T *acc, size_t al, const T *lhs, size_t ll,    \
                                                     const T *rhs, size_t rl) {                                     \
        return prime_op<T>(pl, 4, acc, lhs, rhs, std::min(al, std::min(ll, rl)), 0, CNTT_MEM_HOST, nullptr);        \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_fwd_batch(const PLAN *pl, T *b, size_t batch, cntt_mem_t w, void *st) {       \
        return pl ? prime_op<T>(pl, 0, b, nullptr, nullptr, batch * pl->n, batch, w, (hipStream_t)st)               \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_inv_batch(const PLAN *pl, T *b, size_t batch, cntt_mem_t w, void *st) {       \
        return pl ? prime_op<T>(pl, 1, b, nullptr, nullptr, batch * pl->n, batch, w, (hipStream_t)st)               \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_mul_assign_normalize_batch(const PLAN *pl, T *l, const T *r, size_t batch,    \
                                                                 cntt_mem_t w, void *st) {                          \
        return pl ? prime_op<T>(pl, 2, l, r, nullptr, batch * pl->n, batch, w, (hipStream_t)st)                     \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_normalize_batch(const PLAN *pl, T *v, size_t batch, cntt_mem_t w, void *st) { \
        return pl ? prime_op<T>(pl, 3, v, nullptr, nullptr, batch * pl->n, batch, w, (hipStream_t)st)               \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_mul_accumulate_batch(const PLAN *pl, T *acc, const T *l, const T *r,          \
                                                           size_t batch, cntt_mem_t w, void *st) {                  \
        return pl ? prime_op<T>(pl, 4, acc, l, r, batch * pl->n, batch, w, (hipStream_t)st)                         \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_mul_ntt_batch(const PLAN *pl, T *l, const T *r, size_t batch, cntt_mem_t w,    \
                                                    void *st) {                                                     \
        return pl ? prime_op<T>(pl, 5, l, r, nullptr, batch * pl->n, batch, w, (hipStream_t)st)                     \
                  : fail(CNTT_EINVAL, "plan is NULL");                                                              \
    }                                                                                                               \
    extern "C" int cntt_prime##BITS##_external_product_batch(const PLAN *pl, T *out, const T *terms, const T *key_ntt,  \
                                                            size_t nterms, size_t nout, size_t batch, int accumulate,  \
                                                            cntt_mem_t where, void *stream) {                          \
        return external_product<T>(pl, out, terms, key_ntt, nterms, nout, batch, accumulate, where, (hipStream_t)stream); \
    }

CNTT_PRIME_API(64, uint64_t, cntt_plan64)
CNTT_PRIME_API(32, uint32_t, cntt_plan32)

// the launchers the native and product plans call (host_common.hpp)
template int plan_new<uint32_t, cntt_plan32>(size_t, uint32_t, cntt_plan32 **);
template int plan_new<uint64_t, cntt_plan64>(size_t, uint64_t, cntt_plan64 **);
template int device_tables<uint32_t>(const PrimePlan<uint32_t> *, DeviceTables<uint32_t> *);
template int ntt_device<uint32_t>(const PrimePlan<uint32_t> *, uint32_t *, size_t, bool, hipStream_t);
template int ntt_device<uint64_t>(const PrimePlan<uint64_t> *, uint64_t *, size_t, bool, hipStream_t);
template int mul_ntt_device<uint32_t>(const PrimePlan<uint32_t> *, uint32_t *, const uint32_t *, size_t, hipStream_t);
template int mul_ntt_device<uint64_t>(const PrimePlan<uint64_t> *, uint64_t *, const uint64_t *, size_t, hipStream_t);
template int pointwise_device<uint32_t, PW_MUL_NORMALIZE>(const PrimePlan<uint32_t> *, uint32_t *, const uint32_t *, const uint32_t *, size_t, hipStream_t);
template int pointwise_device<uint64_t, PW_MUL_NORMALIZE>(const PrimePlan<uint64_t> *, uint64_t *, const uint64_t *, const uint64_t *, size_t, hipStream_t);
template int pointwise_device<uint32_t, PW_NORMALIZE>(const PrimePlan<uint32_t> *, uint32_t *, const uint32_t *, const uint32_t *, size_t, hipStream_t);
template int pointwise_device<uint64_t, PW_NORMALIZE>(const PrimePlan<uint64_t> *, uint64_t *, const uint64_t *, const uint64_t *, size_t, hipStream_t);
template int pointwise_device<uint32_t, PW_MUL_ACCUMULATE>(const PrimePlan<uint32_t> *, uint32_t *, const uint32_t *, const uint32_t *, size_t, hipStream_t);
template int pointwise_device<uint64_t, PW_MUL_ACCUMULATE>(const PrimePlan<uint64_t> *, uint64_t *, const uint64_t *, const uint64_t *, size_t, hipStream_t);
template int external_product_device<uint32_t>(const PrimePlan<uint32_t> *, uint32_t *, const uint32_t *, const uint32_t *, size_t, size_t, size_t, bool, hipStream_t);
template int external_product_device<uint64_t>(const PrimePlan<uint64_t> *, uint64_t *, const uint64_t *, const uint64_t *, size_t, size_t, size_t, bool, hipStream_t);

// the programmable bootstrap mod p around external_product_device (include/cntt_prime_pbs.h)
#include "host_prime_pbs.inc"
#include "host_prime_keyswitch.inc"
#include "host_prime_pack.inc"
// the multi-bit bootstrap mod p (include/cntt_prime_multibit.h)
#include "host_prime_multibit.inc"
// the ring automorphism, the Galois keyswitch and the trace mod p (include/cntt_prime_automorphism.h)
#include "host_prime_automorphism.inc"
// ring packing of LWE ciphertexts through automorphisms mod p (include/cntt_prime_ring_pack.h)
#include "host_prime_ring_pack.inc"
// the CMux and the CMux tree against GGSW selectors mod p (include/cntt_prime_cmux.h)
#include "host_prime_cmux.inc"
// the circuit bootstrap from LWE bits to GGSW selectors, the many-LUT bootstrap and the circuit bootstrap with one rotation per input bit
// mod p (include/cntt_prime_cbs.h, cntt_prime_manylut.h)
#include "host_prime_cbs.inc"
