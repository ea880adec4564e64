// libcntt_hip.so host side, native plans (include/cntt.h): the ten kinds with their CRT constants, residue split / CRT / fwd / inv,
// the workspace cache and negacyclic_polymul.  The per-prime transforms go through host_prime.hip.
#include <cstdlib>
#include <map>

#include "aux_kernels.hpp"
#include "host_common.hpp"

static const NativeKindInfo NATIVE_KINDS[10] = {
    {3, 4, 0, 0, 3, {0, 1, 2, 0, 0}, {-1, -1, -1, -1, -1}},   // native32::Plan32           src/native32.rs:28-56
    {5, 8, 0, 0, 3, {0, 1, 3, 0, 0}, {-1, 2, 4, -1, -1}},     // native64::Plan32           src/native64.rs:91-141
    {10, 16, 0, 0, 5, {0, 2, 4, 6, 8}, {1, 3, 5, 7, 9}},      // native128::Plan32          src/native128.rs:20-118
    {2, 4, 0, 1, 2, {0, 1, 0, 0, 0}, {-1, -1, -1, -1, -1}},   // native_binary32::Plan32    src/native_binary32.rs:22-41
    {3, 8, 0, 1, 3, {0, 1, 2, 0, 0}, {-1, -1, -1, -1, -1}},   // native_binary64::Plan32    src/native_binary64.rs:33-61
    {5, 16, 0, 1, 3, {0, 1, 3, 0, 0}, {-1, 2, 4, -1, -1}},    // native_binary128::Plan32   src/native_binary128.rs:13-63
    {2, 4, 1, 0, 2, {0, 1, 0, 0, 0}, {-1, -1, -1, -1, -1}},   // native32::Plan52           src/native32.rs:223-253
    {3, 8, 1, 0, 3, {0, 1, 2, 0, 0}, {-1, -1, -1, -1, -1}},   // native64::Plan52           src/native64.rs:770-829
    {1, 4, 1, 1, 1, {0, 0, 0, 0, 0}, {-1, -1, -1, -1, -1}},   // native_binary32::Plan52    src/native_binary32.rs:111-125
    {2, 8, 1, 1, 2, {0, 1, 0, 0, 0}, {-1, -1, -1, -1, -1}},   // native_binary64::Plan52    src/native_binary64.rs:230-260
};

// One grow-only scratch area per (plan, device) for the composed native pipeline.  Calls from several threads or on
// several streams share it safely: the plan's mutex is held while a call enqueues its launches, and a call on another
// stream first waits for the event the previous user recorded (no wait, no record while a stream is being captured
// into a hipGraph: a graph replays against the buffer it captured, as cntt_native_reserve documents).
struct Workspace {
    void *base = nullptr;
    size_t bytes = 0;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
};
struct NativeCache {
    std::mutex mu;
    std::map<int, Workspace> ws;
    // nprimes x n words psi_i^m n^-1 R^2 mod P_i, R = 2^32 (native_multibit.hpp), per device: built by the plan's first multi-bit call there
    std::map<int, uint32_t *> mono;
    ~NativeCache() {
        for (auto &kv : mono) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) continue;
            (void)hipSetDevice(kv.first);
            (void)hipFree(kv.second);
            (void)hipSetDevice(cur);
        }
        for (auto &kv : ws) {
            int cur = 0;
            if (hipGetDevice(&cur) != hipSuccess) continue;
            (void)hipSetDevice(kv.first);
            (void)hipFree(kv.second.base);
            if (kv.second.last) (void)hipEventDestroy(kv.second.last);
            (void)hipSetDevice(cur);
        }
    }
};

static void build_crt_args(cntt_native *pl) {
    CrtArgs &A = pl->crt;
    const NativeKindInfo &I = pl->info;
    std::memset(&A, 0, sizeof A);
    A.k = I.nprimes;
    A.ngroups = I.ngroups;
    for (int i = 0; i < I.nprimes; ++i) A.prime[i] = pl->prime(i);
    u128 prefix = 1;
    std::vector<uint64_t> M((size_t)I.ngroups);
    for (int g = 0; g < I.ngroups; ++g) {
        const uint64_t pa = pl->prime(I.ga[g]);
        A.ga[g] = I.ga[g];
        A.gb[g] = I.gb[g];
        uint64_t m = pa;
        if (I.gb[g] >= 0) {
            const uint64_t pb = pl->prime(I.gb[g]);
            A.pair_inv[g] = host::powmod(pa % pb, pb - 2, pb);  // P_a^-1 mod P_b (src/lib.rs:536-561)
            A.pair_inv_shoup[g] = (uint32_t)((A.pair_inv[g] << 32) / pb);
            m = pa * pb;
        }
        M[(size_t)g] = m;
        A.M[g] = m;
        // the CRT kernels rely on ascending digit moduli (digits and group residues need no reduction modulo a later
        // modulus); true for every reference plan: primes ascend within primes32 / primes52 (src/lib.rs:447-652)
        if (g > 0 && !(M[(size_t)g - 1] < m)) std::abort();
        A.prefix_lo[g] = (uint64_t)prefix;
        A.prefix_hi[g] = (uint64_t)(prefix >> 64);
        if (g > 0) {
            // inv[g] = (M_0 ... M_{g-1})^-1 mod M[g]; M[g] is a prime or a product of two primes:
            // invert through Euler's theorem like src/lib.rs:541-551
            const uint64_t phi = (I.gb[g] >= 0) ? (pl->prime(I.ga[g]) - 1) * (pl->prime(I.gb[g]) - 1) : (m - 1);
            uint64_t pm = 1;  // true product M_0 ... M_{g-1} mod m (`prefix` itself wraps mod 2^128)
            for (int h = 0; h < g; ++h) pm = host::mulmod(pm, M[(size_t)h] % m, m);
            A.inv[g] = host::powmod(pm, phi - 1, m);
            A.inv_shoup[g] = (uint64_t)((((u128)A.inv[g]) << 64) / m);
            A.inv_shoup32[g] = (m >> 32) == 0 ? (uint32_t)((A.inv[g] << 32) / m) : 0u;
            for (int h = 0; h < g; ++h) {
                A.Mmod[g][h] = M[(size_t)h] % m;
                A.Mmod_shoup[g][h] = (uint64_t)((((u128)A.Mmod[g][h]) << 64) / m);
                A.Mmod_shoup32[g][h] = (m >> 32) == 0 ? (uint32_t)((A.Mmod[g][h] << 32) / m) : 0u;
            }
        }
        prefix *= (u128)m;  // wrapping mod 2^128, as src/lib.rs:592-595
    }
    A.prefix_lo[I.ngroups] = (uint64_t)prefix;
    A.prefix_hi[I.ngroups] = (uint64_t)(prefix >> 64);
}

// Plan32 kinds: M = P_0 ... P_{k-1}, M_i = M / P_i, y_i = M_i^-1 mod P_i (Euler, like src/lib.rs:541-551)
static void build_acc_args(cntt_native *pl) {
    const int k = pl->info.nprimes;
    if (pl->info.is52) return;
    AccArgs &A = pl->acc;
    std::memset(&A, 0, sizeof A);
    u128 m = 1;  // mod 2^128
    for (int i = 0; i < k; ++i) m *= (u128)PRIMES32[i];
    A.m_lo = (uint64_t)m;
    A.m_hi = (uint64_t)(m >> 64);
    for (int i = 0; i < k; ++i) {
        const uint64_t p = PRIMES32[i];
        u128 mi = 1;         // M_i mod 2^128
        uint64_t mi_p = 1;   // M_i mod P_i
        for (int h = 0; h < k; ++h) {
            if (h == i) continue;
            mi *= (u128)PRIMES32[h];
            mi_p = host::mulmod(mi_p, PRIMES32[h] % p, p);
        }
        A.c_lo[i] = (uint64_t)mi;
        A.c_hi[i] = (uint64_t)(mi >> 64);
        A.f[i] = (uint32_t)((((uint64_t)1) << (32 + ACC_FRAC_BITS)) / p);
        A.m60[i] = (uint32_t)((((uint64_t)1) << 60) / p);
        // the lazy split folds a word 32 bits at a time with t = hi c + lo < 2^58: needs c = 2^32 mod p < 2^26 - 1
        if (((((uint64_t)1) << 32) % p) >= (((uint64_t)1) << 26) - 1) return;
        // (M / P_i)^-1 times 2^32: the kernel's pointwise product is a Montgomery product (acc_mont_lazy) and leaves a factor 2^-32
        const uint64_t y = host::mulmod(host::powmod(mi_p, p - 2, p), (((uint64_t)1) << 32) % p, p);
        const cntt_plan32 *sub = pl->p32[(size_t)i].get();
        ModParams<uint32_t> mp = sub->mp;
        if (mp.cls != CLS_LAZY) return;
        mp.n_inv = (uint32_t)host::mulmod(mp.n_inv, y, p);
        mp.n_inv_shoup = shoup_of<uint32_t>(mp.n_inv, (uint32_t)p);
        mp.last_w = (uint32_t)host::mulmod(mp.last_w, y, p);
        mp.last_w_shoup = shoup_of<uint32_t>(mp.last_w, (uint32_t)p);
        pl->mp_acc[i] = mp;
    }
    pl->has_acc = true;
}
bool cntt::native_acc_enabled() {
    return debug_switch(DBG_NATIVE_ACC) != 0;   // A/B runs, parity tests
}

// Exactness bound of the external product (cntt_ext.h): the largest T with D T inside the exact range of the kind's reconstruction,
// D = n A^2 (binary kinds: n A), A = 2^w - 1.  Unsigned big integers as little-endian 32-bit limbs: a few products and comparisons.
namespace {
using Big = std::vector<uint32_t>;
void big_trim(Big &a) {
    while (!a.empty() && a.back() == 0) a.pop_back();
}
Big big_of(uint64_t v) {
    Big a{(uint32_t)v, (uint32_t)(v >> 32)};
    big_trim(a);
    return a;
}
Big big_mul(const Big &a, const Big &b) {
    Big r(a.size() + b.size() + 1, 0);
    for (size_t i = 0; i < a.size(); ++i) {
        uint64_t carry = 0;
        for (size_t j = 0; j < b.size(); ++j) {
            const uint64_t t = (uint64_t)a[i] * b[j] + r[i + j] + carry;
            r[i + j] = (uint32_t)t;
            carry = t >> 32;
        }
        for (size_t k = i + b.size(); carry; ++k) {
            const uint64_t t = (uint64_t)r[k] + carry;
            r[k] = (uint32_t)t;
            carry = t >> 32;
        }
    }
    big_trim(r);
    return r;
}
int big_cmp(const Big &a, const Big &b) {
    if (a.size() != b.size()) return a.size() < b.size() ? -1 : 1;
    for (size_t i = a.size(); i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
Big big_add(const Big &a, const Big &b) {
    Big r(std::max(a.size(), b.size()) + 1, 0);
    uint64_t carry = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        const uint64_t t = (uint64_t)(i < a.size() ? a[i] : 0) + (i < b.size() ? b[i] : 0) + carry;
        r[i] = (uint32_t)t;
        carry = t >> 32;
    }
    big_trim(r);
    return r;
}
Big big_sub(const Big &a, const Big &b) {   // a >= b
    Big r(a);
    int64_t borrow = 0;
    for (size_t i = 0; i < r.size(); ++i) {
        int64_t t = (int64_t)r[i] - (int64_t)(i < b.size() ? b[i] : 0) - borrow;
        borrow = t < 0;
        r[i] = (uint32_t)(t + (borrow ? ((int64_t)1 << 32) : 0));
    }
    big_trim(r);
    return r;
}
Big big_shr(const Big &a, int s) {   // floor(a / 2^s)
    Big r;
    const size_t w = (size_t)s / 32;
    const int b = s % 32;
    for (size_t i = w; i < a.size(); ++i) {
        const uint64_t lo = a[i], hi = i + 1 < a.size() ? a[i + 1] : 0;
        r.push_back((uint32_t)(((hi << 32) | lo) >> b));
    }
    big_trim(r);
    return r;
}
}  // namespace
static size_t native_max_terms_of(const cntt_native *pl) {
    const NativeKindInfo &I = pl->info;
    Big M = big_of(1), Mpre = big_of(1);
    for (int i = 0; i < I.nprimes; ++i) M = big_mul(M, big_of(pl->prime(i)));
    const int top = I.ngroups - 1;   // the top mixed-radix digit: group ga / gb of the last group
    for (int i = 0; i < I.nprimes; ++i)
        if (i != I.ga[top] && i != I.gb[top]) Mpre = big_mul(Mpre, big_of(pl->prime(i)));
    // the reference's sign rule on the top digit: exact for c in [-(M - M / Mt) / 2, (M + M / Mt) / 2 - 1]
    Big lim = big_shr(big_sub(M, Mpre), 1);
    const Big up = big_sub(big_shr(big_add(M, Mpre), 1), big_of(1));
    if (big_cmp(up, lim) < 0) lim = up;
    if (!I.is52) {   // accumulating CRT (native_fused.hpp): c <= (M - 1) / 2 and -c <= floor(M (2^27 - 3 k) / 2^28)
        const Big a = big_shr(big_sub(M, big_of(1)), 1);
        const Big b = big_shr(big_mul(M, big_of(((uint64_t)1 << ACC_FRAC_BITS) - 3 * (uint64_t)I.nprimes)), ACC_FRAC_BITS + 1);
        if (big_cmp(a, lim) < 0) lim = a;
        if (big_cmp(b, lim) < 0) lim = b;
    }
    Big A(I.word / 4, 0xffffffffu);   // 2^w - 1
    Big D = big_mul(big_of(pl->n), I.binary ? A : big_mul(A, A));
    // largest T < 2^63 with D T <= lim (bisection)
    uint64_t lo = 0, hi = (uint64_t)1 << 63;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (big_cmp(big_mul(D, big_of(mid)), lim) <= 0) lo = mid;
        else hi = mid;
    }
    return lo < 1 ? 1 : (size_t)lo;
}

extern "C" int cntt_native_plan_new(cntt_native_kind_t kind, size_t n, cntt_native_t **out) {
    if (!out) return fail(CNTT_EINVAL, "out is NULL");
    *out = nullptr;
    if ((int)kind < 0 || (int)kind > 9) return fail(CNTT_EINVAL, "unknown native plan kind");
    std::unique_ptr<cntt_native> pl(new (std::nothrow) cntt_native());
    if (!pl) return fail(CNTT_ENOMEM, "out of memory");
    pl->kind = kind;
    pl->info = NATIVE_KINDS[kind];
    pl->n = n;
    for (int i = 0; i < pl->info.nprimes; ++i) {  // `?` propagation: src/native64.rs:933-942
        if (pl->info.is52) {
            cntt_plan64 *sub = nullptr;
            if (int rc = plan_new<uint64_t, cntt_plan64>(n, PRIMES52[i], &sub)) return rc;
            pl->p64.emplace_back(sub);
        } else {
            cntt_plan32 *sub = nullptr;
            if (int rc = plan_new<uint32_t, cntt_plan32>(n, PRIMES32[i], &sub)) return rc;
            pl->p32.emplace_back(sub);
        }
    }
    build_crt_args(pl.get());
    build_acc_args(pl.get());
    pl->max_terms = native_max_terms_of(pl.get());
    pl->cache = std::make_shared<NativeCache>();
    if (pl->info.is52) {
        static const cntt_native_kind_t SAME_WORDS[10] = {CNTT_NATIVE32_PLAN32, CNTT_NATIVE64_PLAN32, CNTT_NATIVE128_PLAN32,
                                                          CNTT_NATIVE_BINARY32_PLAN32, CNTT_NATIVE_BINARY64_PLAN32,
                                                          CNTT_NATIVE_BINARY128_PLAN32, CNTT_NATIVE32_PLAN32, CNTT_NATIVE64_PLAN32,
                                                          CNTT_NATIVE_BINARY32_PLAN32, CNTT_NATIVE_BINARY64_PLAN32};
        cntt_native_t *v = nullptr;
        if (cntt_native_plan_new(SAME_WORDS[kind], n, &v) == CNTT_OK) pl->via32.reset(v);   // None (n < 32 ...): composed path
    }
    *out = pl.release();
    return CNTT_OK;
}

extern "C" cntt_native_t *cntt_native_plan_clone(const cntt_native_t *pl) {
    if (!pl) return nullptr;
    cntt_native_t *out = nullptr;
    if (cntt_native_plan_new(pl->kind, pl->n, &out) != CNTT_OK) return nullptr;
    return out;
}
extern "C" void cntt_native_plan_free(cntt_native_t *pl) { delete pl; }
extern "C" size_t cntt_native_ntt_size(const cntt_native_t *pl) { return pl ? pl->n : 0; }
extern "C" int cntt_native_nprimes(const cntt_native_t *pl) { return pl ? pl->info.nprimes : 0; }
extern "C" int cntt_native_word_bytes(const cntt_native_t *pl) { return pl ? pl->info.word : 0; }
extern "C" int cntt_native_residue_bytes(const cntt_native_t *pl) { return pl ? (int)pl->rbytes() : 0; }
extern "C" const cntt_plan32_t *cntt_native_ntt32(const cntt_native_t *pl, int i) {
    if (!pl || pl->info.is52 || i < 0 || i >= pl->info.nprimes) return nullptr;
    return pl->p32[(size_t)i].get();
}
extern "C" const cntt_plan64_t *cntt_native_ntt64(const cntt_native_t *pl, int i) {
    if (!pl || !pl->info.is52 || i < 0 || i >= pl->info.nprimes) return nullptr;
    return pl->p64[(size_t)i].get();
}

template <class W, class R> static void launch_split(const void *value, const SplitArgs &A, size_t count, bool binary, hipStream_t st) {
    if (binary)
        hipLaunchKernelGGL((split_kernel<W, R, true>), dim3(ew_grid(count)), dim3(256), 0, st, (const W *)value, A, count);
    else
        hipLaunchKernelGGL((split_kernel<W, R, false>), dim3(ew_grid(count)), dim3(256), 0, st, (const W *)value, A, count);
}
// the 16-byte word of split_kernel / crt_kernel.  The same layout as Word128 (native_fused.hpp), but the kernels' symbol names carry
// this type: keep it, or every <W128, ...> kernel is renamed
struct W128 {
    uint64_t lo, hi;
};
SplitArgs native_split_args(const cntt_native *pl, void *const *res) {
    SplitArgs A{};
    A.k = pl->info.nprimes;
    for (int i = 0; i < A.k; ++i) {
        const uint64_t p = pl->prime(i);
        A.res[i] = res ? res[i] : nullptr;
        A.prime[i] = p;
        if (pl->info.is52) {
            A.barrett[i] = (uint64_t)((((u128)1) << 64) / p);
        } else {
            const uint64_t c = (((uint64_t)1) << 32) % p;
            A.c[i] = (uint32_t)c;
            A.c_shoup[i] = (uint32_t)((c << 32) / p);
            A.one_shoup[i] = (uint32_t)((((uint64_t)1) << 32) / p);
        }
    }
    return A;
}
int native_split_device(const cntt_native *pl, const void *value, void *const *res, size_t count, bool binary,
                               hipStream_t st) {
    const SplitArgs A = native_split_args(pl, res);
    // a u32 word is always below the 50-bit primes: src/native32.rs:447-452 copies it without `%`
    if (pl->info.is52) {
        if (pl->info.word == 4)
            launch_split<uint32_t, uint64_t>(value, A, count, true, st);
        else
            launch_split<uint64_t, uint64_t>(value, A, count, binary, st);
    } else {
        if (pl->info.word == 4)
            launch_split<uint32_t, uint32_t>(value, A, count, binary, st);
        else if (pl->info.word == 8)
            launch_split<uint64_t, uint32_t>(value, A, count, binary, st);
        else
            launch_split<W128, uint32_t>(value, A, count, binary, st);
    }
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}
template <class W, class R, int NG, uint32_t PAIRS>
static void launch_crt(void *value, const CrtArgs &A, size_t count, hipStream_t st) {
    hipLaunchKernelGGL((crt_kernel<W, R, NG, PAIRS>), dim3(ew_grid(count)), dim3(256), 0, st, (W *)value, A, count);
}
int native_crt_device(const cntt_native *pl, void *value, void *const *res, size_t count, hipStream_t st) {
    CrtArgs A = pl->crt;
    for (int i = 0; i < A.k; ++i) A.res[i] = res[i];
    switch (pl->kind) {  // digit structure of each reference plan (NATIVE_KINDS)
    case CNTT_NATIVE32_PLAN32: launch_crt<uint32_t, uint32_t, 3, 0u>(value, A, count, st); break;
    case CNTT_NATIVE64_PLAN32: launch_crt<uint64_t, uint32_t, 3, 0b110u>(value, A, count, st); break;
    case CNTT_NATIVE128_PLAN32: launch_crt<W128, uint32_t, 5, 0b11111u>(value, A, count, st); break;
    case CNTT_NATIVE_BINARY32_PLAN32: launch_crt<uint32_t, uint32_t, 2, 0u>(value, A, count, st); break;
    case CNTT_NATIVE_BINARY64_PLAN32: launch_crt<uint64_t, uint32_t, 3, 0u>(value, A, count, st); break;
    case CNTT_NATIVE_BINARY128_PLAN32: launch_crt<W128, uint32_t, 3, 0b110u>(value, A, count, st); break;
    case CNTT_NATIVE32_PLAN52: launch_crt<uint32_t, uint64_t, 2, 0u>(value, A, count, st); break;
    case CNTT_NATIVE64_PLAN52: launch_crt<uint64_t, uint64_t, 3, 0u>(value, A, count, st); break;
    case CNTT_NATIVE_BINARY32_PLAN52: launch_crt<uint32_t, uint64_t, 1, 0u>(value, A, count, st); break;
    case CNTT_NATIVE_BINARY64_PLAN52: launch_crt<uint64_t, uint64_t, 2, 0u>(value, A, count, st); break;
    default: return fail(CNTT_EINVAL, "unknown native plan kind");
    }
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}
// The monomial tables of the multi-bit bootstrap (include/cntt_multibit.h, native_multibit.hpp): tab[i][m] = psi_i^m n^-1 R^2 mod P_i for
// m < n, psi_i the root of sub-plan i and R = 2^32, nprimes x n words in one allocation per (plan, device).  Built on the host by the
// first multi-bit call of the plan on the device, under the cache's mutex: a synchronous allocation and copy, so that call may not sit
// inside a stream capture ("First call" in the header).  Later calls: one lock, one look-up.
int native_multibit_tables(const cntt_native *pl, const uint32_t **tab) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const size_t n = pl->n;
    const int k = pl->info.nprimes;
    std::lock_guard<std::mutex> lk(pl->cache->mu);
    uint32_t *&d = pl->cache->mono[dev];
    if (!d) {
        std::vector<uint32_t> host((size_t)k * n);
        for (int i = 0; i < k; ++i) {
            const cntt_plan32 *sub = pl->p32[(size_t)i].get();
            const uint64_t p = sub->p;
            uint64_t x = host::mulmod((uint64_t)sub->mp.r2, (uint64_t)sub->n_inv, p);
            for (size_t m = 0; m < n; ++m) {
                host[(size_t)i * n + m] = (uint32_t)x;
                x = host::mulmod(x, sub->root, p);
            }
        }
        uint32_t *fresh = nullptr;
        if (hipMalloc((void **)&fresh, host.size() * sizeof(uint32_t)) != hipSuccess)
            return fail(CNTT_ENOMEM, "hipMalloc of the monomial tables failed");
        const hipError_t c = hipMemcpy(fresh, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (c != hipSuccess) {
            (void)hipFree(fresh);
            return fail(CNTT_EDEVICE, "upload of the monomial tables failed: %s", hipGetErrorString(c));
        }
        d = fresh;
    }
    for (int i = 0; i < k; ++i) tab[i] = d + (size_t)i * n;
    return CNTT_OK;
}
// the transforms of the sub-plans on `res`; public to the other host units (host_common.hpp)
int native_ntt_device(const cntt_native *pl, void *const *res, size_t batch, bool inv, hipStream_t st) {
    for (int i = 0; i < pl->info.nprimes; ++i) {
        int rc = pl->info.is52 ? ntt_device<uint64_t>(pl->p64[(size_t)i].get(), (uint64_t *)res[i], batch, inv, st)
                               : ntt_device<uint32_t>(pl->p32[(size_t)i].get(), (uint32_t *)res[i], batch, inv, st);
        if (rc) return rc;
    }
    return CNTT_OK;
}

// op: 0 fwd, 1 fwd_binary, 2 inv   (device pointers)
static int native_op_device(const cntt_native *pl, int op, void *value, void *const *res, size_t batch, hipStream_t st) {
    const size_t count = batch * pl->n;
    if (op == 2) {
        if (int rc = native_ntt_device(pl, res, batch, true, st)) return rc;
        return native_crt_device(pl, value, res, count, st);
    }
    if (int rc = native_split_device(pl, value, res, count, op == 1, st)) return rc;
    return native_ntt_device(pl, res, batch, false, st);
}

static int native_op(const cntt_native *pl, int op, void *value, void *const *res, size_t batch, cntt_mem_t where,
                     hipStream_t st) {
    if (!pl || !value || !res) return fail(CNTT_EINVAL, "NULL argument");
    if (op == 1 && !pl->info.binary) return fail(CNTT_EINVAL, "fwd_binary exists only on native_binary* plans");
    if (batch == 0) return CNTT_OK;
    const int k = pl->info.nprimes;
    for (int i = 0; i < k; ++i)
        if (!res[i]) return fail(CNTT_EINVAL, "NULL residue buffer");
    const size_t count = batch * pl->n, vbytes = count * (size_t)pl->info.word, rb = count * pl->rbytes();
    {   // fwd writes the planes, inv the planes and the value: none of them may overlap another (include/cntt.h, "Operands")
        static const char *const PLANE[10] = {"residues[0]", "residues[1]", "residues[2]", "residues[3]", "residues[4]",
                                              "residues[5]", "residues[6]", "residues[7]", "residues[8]", "residues[9]"};
        Operand ops[11];
        ops[0] = {"value", value, vbytes, (size_t)pl->info.word, op == 2};
        for (int i = 0; i < k; ++i) ops[1 + i] = {PLANE[i], res[i], rb, pl->rbytes(), true};
        if (int rc = check_operands(ops, 1 + k)) return rc;
    }
    // fwd reads the value and writes the residues; inv reads the residues and writes the value AND the (inverse-transformed)
    // residues: src/native64.rs:1010-1014
    Staging s(where, st);
    void *dres[10];
    for (int i = 0; i < k; ++i) dres[i] = op == 2 ? s.inout(res[i], rb) : s.out(res[i], rb);
    void *dv = op == 2 ? s.out(value, vbytes) : s.in(value, vbytes);
    if (int rc = s.status()) return rc;
    if (int rc = native_op_device(pl, op, dv, dres, batch, st)) return rc;
    return s.finish();
}

extern "C" int cntt_native_fwd(const cntt_native_t *pl, const void *value, size_t len, void *const *res) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (len != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", len, pl->n);
    return native_op(pl, 0, const_cast<void *>(value), res, 1, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_native_fwd_binary(const cntt_native_t *pl, const void *value, size_t len, void *const *res) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (len != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", len, pl->n);
    return native_op(pl, 1, const_cast<void *>(value), res, 1, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_native_inv(const cntt_native_t *pl, void *value, size_t len, void *const *res) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (len != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", len, pl->n);
    return native_op(pl, 2, value, res, 1, CNTT_MEM_HOST, nullptr);
}
extern "C" int cntt_native_fwd_batch(const cntt_native_t *pl, const void *value, void *const *res, size_t batch,
                                     cntt_mem_t where, void *st) {
    return native_op(pl, 0, const_cast<void *>(value), res, batch, where, (hipStream_t)st);
}
extern "C" int cntt_native_fwd_binary_batch(const cntt_native_t *pl, const void *value, void *const *res, size_t batch,
                                            cntt_mem_t where, void *st) {
    return native_op(pl, 1, const_cast<void *>(value), res, batch, where, (hipStream_t)st);
}
extern "C" int cntt_native_inv_batch(const cntt_native_t *pl, void *value, void *const *res, size_t batch,
                                     cntt_mem_t where, void *st) {
    return native_op(pl, 2, value, res, batch, where, (hipStream_t)st);
}

// bytes of workspace a polymul of `batch` products takes: the per-workgroup parking area of the large-n whole-product
// kernel (native_fused.hpp) where that kernel runs, otherwise both operands' residue arrays of the composed pipeline
static bool native_fusable(const cntt_native *pl, size_t batch) {
    if (batch == 0 || batch >= ((size_t)1 << 32) || pl->info.is52) return false;
    return with_plan32_kind(pl->kind, [](auto) { return hipSuccess; }) == hipSuccess;
}
static size_t native_park_bytes(const cntt_native *pl, size_t batch) {
    if (!native_fusable(pl, batch)) return 0;
    return sizeof(uint32_t) * native_fused_scratch_words((int)pl->kind, pl->p32[0]->logn, pl->info.nprimes, device_num_cus(),
                                                        (uint32_t)batch);
}
static size_t native_workspace_bytes(const cntt_native *pl, size_t batch) {
    const size_t park = native_park_bytes(pl, batch);
    if (park) return park;
    // the register-resident whole-product kernel (accumulating CRT) and the LDS-parked one (32 <= n <= 4096, every fused kind but
    // native128) need no workspace at all
    if (native_fusable(pl, batch) && pl->has_acc && native_fused_acc((int)pl->kind, pl->p32[0]->logn) && native_acc_enabled()) return 0;
    if (native_fusable(pl, batch) && pl->p32[0]->logn >= 5 && pl->p32[0]->logn <= 12 && pl->kind != CNTT_NATIVE128_PLAN32) return 0;
    return 2 * (size_t)pl->info.nprimes * batch * pl->n * pl->rbytes();
}
// Plan52 kinds: does negacyclic_polymul run the Plan32 whole-product kernel of the same words?  (Measured, ns per product, through it /
// composed on the 50-bit primes, profiles/r05_plan52_via32.txt: native64 n = 4096 102 / 187, native32 n = 1024 12 / 28.5,
// native_binary64 n = 16384 384 / 572 ...; the one shape where the composed pipeline wins is native64 at n = 32768: 1816 / 1769.)
static bool plan52_via32(const cntt_native *pl) {
    if (!pl->via32 || debug_switch(DBG_PLAN52_VIA32) == 0) return false;
    return !(pl->kind == CNTT_NATIVE64_PLAN52 && pl->n >= 32768);
}
// caller holds pl->cache->mu
static int native_workspace(const cntt_native *pl, size_t need, Workspace **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    Workspace &w = pl->cache->ws[dev];
    if (w.bytes < need) {
        if (w.base) {
            HIP_TRY(hipDeviceSynchronize());  // the old workspace may still be in use by enqueued work
            (void)hipFree(w.base);
            w.base = nullptr;
            w.bytes = 0;
        }
        if (hipMalloc(&w.base, need) != hipSuccess) {
            w.base = nullptr;
            return fail(CNTT_ENOMEM, "hipMalloc(%zu) for the native workspace failed", need);
        }
        w.bytes = need;
    }
    *out = &w;
    return CNTT_OK;
}
extern "C" int cntt_native_reserve(const cntt_native_t *pl, size_t batch) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (plan52_via32(pl)) return cntt_native_reserve(pl->via32.get(), batch);
    std::lock_guard<std::mutex> lk(pl->cache->mu);
    Workspace *w = nullptr;
    return native_workspace(pl, native_workspace_bytes(pl, batch), &w);
}

// negacyclic_polymul on device memory: src/native64.rs:1042-1069 batched
// whole product in one kernel (native_fused.hpp) for the Plan32 kinds, 32 <= n <= 16384
static int native_fused_device(const cntt_native *pl, void *prod, const void *lhs, const void *rhs, size_t batch,
                               uint32_t *park, hipStream_t st) {
    return native_fused_launch(pl, "fused polymul", [&](auto kind, int &rc) {
        constexpr int KIND = decltype(kind)::value;
        FusedTables<NativeShape<KIND>::KP> F{}, Facc{};
        if ((rc = native_acc_tables<KIND>(pl, nullptr, &Facc, nullptr))) return hipErrorUnknown;
        F = Facc;
        for (int i = 0; i < NativeShape<KIND>::KP; ++i) F.P[i] = pl->p32[(size_t)i]->mp;
        const SplitArgs S = native_split_args(pl, nullptr);
        return launch_native_fused<KIND>(pl->p32[0]->logn, prod, lhs, rhs, &F, S, pl->crt, (uint32_t)batch, park, st,
                                         pl->has_acc ? &pl->acc : nullptr, pl->has_acc ? &Facc : nullptr);
    });
}

static int native_polymul_device(const cntt_native *pl, void *prod, const void *lhs, const void *rhs, size_t batch,
                                 hipStream_t st) {
    if (plan52_via32(pl)) return native_polymul_device(pl->via32.get(), prod, lhs, rhs, batch, st);
    const size_t park = native_park_bytes(pl, batch);
    if (park == 0 && native_fusable(pl, batch)) {
        const int rc = native_fused_device(pl, prod, lhs, rhs, batch, nullptr, st);
        if (rc != FUSED_NONE) return rc;
    }
    std::lock_guard<std::mutex> lk(pl->cache->mu);  // held while this call's launches are enqueued
    Workspace *ws = nullptr;
    if (int rc = native_workspace(pl, native_workspace_bytes(pl, batch), &ws)) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    const bool capturing = cap != hipStreamCaptureStatusNone;
    if (!capturing && ws->last && ws->last_stream != st) HIP_TRY(hipStreamWaitEvent(st, ws->last, 0));
    struct Release {  // records "done with the workspace" on every exit path
        Workspace *w;
        hipStream_t st;
        bool on;
        ~Release() {
            if (!on) return;
            if (!w->last && hipEventCreateWithFlags(&w->last, hipEventDisableTiming) != hipSuccess) w->last = nullptr;
            if (w->last) (void)hipEventRecord(w->last, st);
            w->last_stream = st;
        }
    } release{ws, st, !capturing};
    void *base = ws->base;
    if (park) {  // n = 8192 / 16384: the persistent whole-product kernel, its workgroups parking residue tiles in the workspace
        const int rc = native_fused_device(pl, prod, lhs, rhs, batch, (uint32_t *)base, st);
        return rc == FUSED_NONE ? fail(CNTT_EDEVICE, "no whole-product kernel for n = %zu", pl->n) : rc;
    }
    const int k = pl->info.nprimes;
    const size_t count = batch * pl->n, rb = count * pl->rbytes();
    void *L[10], *R[10];
    for (int i = 0; i < k; ++i) {
        L[i] = (char *)base + (size_t)i * rb;
        R[i] = (char *)base + (size_t)(k + i) * rb;
    }
    // rhs: split + forward transforms; lhs: split, then per prime the fused
    // inv(mul_assign_normalize(fwd(lhs_i), rhs_i^)) (one kernel for n <= 2048, three launches otherwise); CRT.
    if (int rc = native_op_device(pl, pl->info.binary ? 1 : 0, const_cast<void *>(rhs), R, batch, st)) return rc;
    if (int rc = native_split_device(pl, lhs, L, count, false, st)) return rc;
    for (int i = 0; i < k; ++i) {
        int rc = pl->info.is52 ? mul_ntt_device<uint64_t>(pl->p64[(size_t)i].get(), (uint64_t *)L[i],
                                                         (const uint64_t *)R[i], batch, st)
                               : mul_ntt_device<uint32_t>(pl->p32[(size_t)i].get(), (uint32_t *)L[i],
                                                         (const uint32_t *)R[i], batch, st);
        if (rc) return rc;
    }
    return native_crt_device(pl, prod, L, count, st);
}

extern "C" int cntt_native_negacyclic_polymul_batch(const cntt_native_t *pl, void *prod, const void *lhs,
                                                    const void *rhs, size_t batch, cntt_mem_t where, void *stream) {
    if (!pl || !prod || !lhs || !rhs) return fail(CNTT_EINVAL, "NULL argument");
    if (batch == 0) return CNTT_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t vbytes = batch * pl->n * (size_t)pl->info.word, word = (size_t)pl->info.word;
    const Operand ops[3] = {{"prod", prod, vbytes, word, true}, {"lhs", lhs, vbytes, word, false}, {"rhs", rhs, vbytes, word, false}};
    if (int rc = check_operands(ops, 3)) return rc;
    Staging s(where, st);
    void *dp = s.out(prod, vbytes);
    const void *dl = s.in(lhs, vbytes), *dr = s.in(rhs, vbytes);
    if (int rc = s.status()) return rc;
    if (int rc = native_polymul_device(pl, dp, dl, dr, batch, st)) return rc;
    return s.finish();
}
extern "C" int cntt_native_negacyclic_polymul(const cntt_native_t *pl, void *prod, size_t pn, const void *lhs, size_t ln,
                                              const void *rhs, size_t rn) {
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    // assert_eq!(n, lhs.len()); assert_eq!(n, rhs.len()) then the inner fwd asserts ntt_size: src/native64.rs:1043-1045
    if (pn != ln || pn != rn) return fail(CNTT_ELEN, "prod/lhs/rhs lengths differ");
    if (pn != pl->n) return fail(CNTT_ELEN, "assert_eq!(buf.len(), ntt_size): %zu != %zu", pn, pl->n);
    return cntt_native_negacyclic_polymul_batch(pl, prod, lhs, rhs, 1, CNTT_MEM_HOST, nullptr);
}
