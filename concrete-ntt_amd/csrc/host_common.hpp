// What the host units of libcntt_hip.so share (host_core / host_prime / host_native / host_native_ext / host_product .hip): the plan
// structs behind the C ABI, error reporting, the memory frame of the _batch calls (Staging: device pointers handed through, host slices
// staged) and the functions that cross unit borders.  Internal, never
// installed.  Every __global__ template is launched -- and so instantiated -- by exactly ONE unit; the others call the host function
// that owns the launch, declared here and explicitly instantiated there.  Nothing declared here is exported.
// pbs_host.hpp, on top of this file, is the host side of the programmable bootstrap as templates over the plan family, and lwe_host.hpp, on
// top of that, the host side of the keyswitch, keyswitch + bootstrap and packing keyswitch; multibit_host.hpp, also on top of pbs_host.hpp,
// the host side of the multi-bit blind rotation and bootstrap, and cbs_host.hpp that of the circuit bootstrap and the many-LUT calls:
// host_native_ext.hip and host_prime.hip (through its host_prime_*.inc) each
// include them and instantiate them for their plans.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/cntt.h"
#include "../../include/cntt_ext.h"
#include "host_math.hpp"
#include "native_ext.hpp"
#include "ntt_launch.hpp"

using namespace cntt;
using host::u128;

#pragma GCC visibility push(hidden)
// ---------------------------------------------------------------------------------------------
// errors (host_core.hip: the thread-local message behind cntt_last_error)
// ---------------------------------------------------------------------------------------------
int fail(int code, const char *fmt, ...);
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(CNTT_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// The aliasing and alignment contract of the _batch calls (include/cntt.h, "Operands"): every operand aligned to its word, and an
// operand the call writes disjoint from every other one; read-only operands may coincide.  Pointer comparisons only, before any device
// call.  The later headers' calls (pbs_host.hpp, lwe_host.hpp) name their pairs one by one with ranges_overlap; those of multibit_host.hpp use
// check_operands.
inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return abytes && bbytes && x < y + bbytes && y < x + abytes;
}
// whether the product of the factors reaches 2^63: taken factor by factor, so that the 128-bit product never wraps.  For the byte counts
// that are products of a call's arguments: they must fit before they are formed.
inline bool product_passes_2_63(std::initializer_list<size_t> factors) {
    u128 x = 1;
    for (size_t f : factors) {
        if (f == 0) return false;
        x *= f;
        if (x >= ((u128)1 << 63)) return true;
    }
    return false;
}
struct Operand {
    const char *name;
    const void *ptr;
    size_t bytes, align;
    bool written;
};
inline int check_operands(const Operand *ops, int count) {
    for (int i = 0; i < count; ++i)
        if (ops[i].bytes && (uintptr_t)ops[i].ptr % ops[i].align)
            return fail(CNTT_EINVAL, "%s is not %zu-byte aligned", ops[i].name, ops[i].align);
    for (int i = 0; i < count; ++i)
        for (int j = i + 1; j < count; ++j)
            if ((ops[i].written || ops[j].written) && ranges_overlap(ops[i].ptr, ops[i].bytes, ops[j].ptr, ops[j].bytes)) {
                const Operand &w = ops[i].written ? ops[i] : ops[j], &o = ops[i].written ? ops[j] : ops[i];
                return fail(CNTT_EINVAL, "%s overlaps %s", w.name, o.name);
            }
    return CNTT_OK;
}

// Grid of the element-wise kernels (grid-stride loops: any grid is correct): one 256-thread block per 256 work items, NOT capped at
// a few blocks per CU.  Measured (tools/pw_probe.py, 65536 x 1024 u64): mul_assign_normalize 0.374 -> 0.271 ms (4.3 -> 5.9 TB/s),
// normalize 0.232 -> 0.178 ms (4.6 -> 6.0 TB/s) against the 2048-block persistent form; split / CRT / Garner kernels -4 ... -7 %.
// The cap: a dispatch holds at most 2^32 - 1 work-items per dimension (grid_size_x of the AQL packet is a uint32), i.e. fewer than
// 2^24 blocks of 256 threads; beyond it (16 GiB of u32 and up -- plausible on 288 GB) the kernels' 64-bit grid-stride loops
// take over.  Exported as cntt_ew_grid (host_core.hip).
inline unsigned ew_grid(size_t work_items) {
    const size_t blocks = (work_items + 255) / 256;
    return (unsigned)std::max<size_t>(1, std::min<size_t>(blocks, ((size_t)1 << 24) - 1));
}

// Working set (bytes one call reads and writes) above which the stand-alone transforms and the pointwise kernels take the
// non-temporal policy.  384 MiB is 1.5 x the 256 MiB Infinity Cache: batches that fit the cache lost 3-17 % with the hint.
// The streaming tests restate this number (STREAM_BYTES): tests/test_gpu_multitrip_transforms.py (for test_gpu_streamed_batches.py),
// test_gpu_native_gadget.py, test_gpu_native_pbs.py, test_gpu_prime_pbs.py and tests/streaming_cases.py (for
// test_gpu_prime_streaming.py, with the byte count of every launch site that compares against it).
constexpr size_t STREAM_BYTES = (size_t)384 << 20;

// A stream-ordered device block (hipMallocAsync), released on its stream when the holder goes: after everything the call enqueued
// before that, on success and on failure alike.  Staging holds its device-mode workspace in one; so do the composed paths' scratch.
class StreamBlock {
    hipStream_t st_;
    void *p_ = nullptr;

  public:
    explicit StreamBlock(hipStream_t st) : st_(st) {}
    StreamBlock(const StreamBlock &) = delete;
    ~StreamBlock() {
        if (p_) (void)hipFreeAsync(p_, st_);
    }
    void *get() const { return p_; }
    int alloc(size_t bytes) {   // once per holder
        const hipError_t e = hipMallocAsync(&p_, bytes, st_);
        if (e == hipSuccess) return CNTT_OK;
        p_ = nullptr;
        return fail(CNTT_EDEVICE, "hipMallocAsync(%zu bytes): %s", bytes, hipGetErrorString(e));
    }
};

// The memory frame of every _batch call: where its _device function finds the operands and the workspace.  A call states each operand
// once -- in / out / inout, F::key_in, workspace -- checks status(), runs its _device function on what it got and returns finish().
// CNTT_MEM_HOST, the host-slice path: device copies of the caller's buffers, one hipMalloc each (16 bytes for an empty one), freed by the
// destructor.  in / inout enqueue their host-to-device copy on the stream when they are called; out / inout record a copy back, which
// finish() enqueues in the order of the calls before the one synchronise.  After a failed allocation or copy every later call returns
// nullptr and status() / finish() give the code.  workspace() is alloc(need): a workspace the caller brought lies in host memory, is
// checked by the call and then ignored.
// CNTT_MEM_DEVICE, the device path: in / out / inout hand back the caller's pointer (the NULL of an absent operand too) and allocate,
// copy and record nothing; finish() is status() and never synchronises.  workspace() is the caller's where there is one -- no runtime
// call at all then, which is what lets the call sit in a stream capture -- and else, if the call uses it, one hipMallocAsync on the
// stream that the destructor releases there (StreamBlock).
// host(): for the two things only the host path may do -- read the rotation exponents (check_rot_host, pbs_host.hpp) and rebuild the
// native kinds' key planes.
class Staging {
    struct Back {
        void *host, *dev;
        size_t bytes;
    };
    hipStream_t st_;
    const bool host_;
    int rc_ = CNTT_OK;
    std::vector<void *> dev_;
    std::vector<Back> back_;
    StreamBlock ws_;

  public:
    Staging(cntt_mem_t where, hipStream_t st) : st_(st), host_(where != CNTT_MEM_DEVICE), ws_(st) {}
    Staging(const Staging &) = delete;
    ~Staging() {
        for (void *p : dev_) (void)hipFree(p);
    }
    bool host() const { return host_; }
    int status() const { return rc_; }
    void *alloc(size_t bytes) {   // host mode: device scratch that lives as long as this object
        void *p = nullptr;
        if (rc_ != CNTT_OK) return nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) {
            rc_ = fail(CNTT_EDEVICE, "hipMalloc(%zu) failed (no GPU, or out of device memory)", bytes);
            return nullptr;
        }
        dev_.push_back(p);
        return p;
    }
    void *in(const void *host, size_t bytes) {
        if (!host_) return const_cast<void *>(host);
        void *p = alloc(bytes);
        const hipError_t e = p && bytes ? hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, st_) : hipSuccess;
        if (e != hipSuccess) rc_ = fail(CNTT_EDEVICE, "hipMemcpyAsync(host to device, %zu bytes): %s", bytes, hipGetErrorString(e));
        return rc_ == CNTT_OK ? p : nullptr;
    }
    void *out(void *host, size_t bytes) {
        if (!host_) return host;
        void *p = alloc(bytes);
        if (p && bytes) back_.push_back({host, p, bytes});
        return p;
    }
    void *inout(void *host, size_t bytes) {
        if (!host_) return host;
        void *p = in(host, bytes);
        if (p && bytes) back_.push_back({host, p, bytes});
        return p;
    }
    // `used`: whether the call touches its workspace at all (the device path allocates none for a call that does not)
    void *workspace(void *callers, size_t need, bool used = true) {
        if (host_) return alloc(need);
        if (callers || !used || rc_ != CNTT_OK) return callers;
        rc_ = ws_.alloc(need);
        return ws_.get();
    }
    int finish() {
        if (rc_ != CNTT_OK || !host_) return rc_;
        for (const Back &b : back_) HIP_TRY(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, st_));
        HIP_TRY(hipStreamSynchronize(st_));
        return CNTT_OK;
    }
};

#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------
// the plans behind the opaque handles of include/cntt.h: prime (host_prime.hip) ...
// ---------------------------------------------------------------------------------------------
template <class T> struct DeviceTables {
    TwPair<T> *fwd = nullptr, *inv = nullptr;
    // plans whose LDS-resident transforms run in a 64-bit-only class: the same twiddles in that class's form --
    // CLS_FP / CLS_FP51: (c, c / p) doubles, c centred in (-p/2, p/2];  CLS_PM64: plain residues;  CLS_FPW: c as one double
    TwPair<T> *fwd_fp = nullptr, *inv_fp = nullptr;
    // psi^m 2^(2B) mod p for m < n (prime_multibit.hpp): built by the plan's first multi-bit call on the device, nullptr until then
    T *mono = nullptr;
};
template <class T> struct DeviceCache;   // per-device replicas of the tables (host_prime.hip)

template <class T> struct PrimePlan {
    static constexpr int B = sizeof(T) * 8;
    size_t n = 0;
    int logn = 0;
    T p = 0;
    uint64_t root = 0;
    bool has_shoup = false;
    // reference-layout tables (src/prime64.rs:221-236)
    std::vector<T> twid, twid_shoup, inv_twid, inv_twid_shoup;
    T p_barrett = 0, n_inv = 0, n_inv_shoup = 0;
    uint32_t big_q = 0;
    ModParams<T> mp{};
    std::shared_ptr<DeviceCache<T>> cache;
};

struct cntt_plan64 : PrimePlan<uint64_t> {};
struct cntt_plan32 : PrimePlan<uint32_t> {};

// ---------------------------------------------------------------------------------------------
// ... native (host_native.hip; external product, gadget decomposition and bootstrap: host_native_ext.hip) ...
// ---------------------------------------------------------------------------------------------
// src/lib.rs:453-462 and :601-606
constexpr uint32_t PRIMES32[10] = {1062862849u, 1063059457u, 1064697857u, 1065484289u, 1068236801u,
                                   1068433409u, 1068564481u, 1069219841u, 1071513601u, 1073479681u};
constexpr uint64_t PRIMES52[6] = {1125899881086977ull, 1125899885412353ull, 1125899886395393ull,
                                  1125899899174913ull, 1125899902124033ull, 1125899903107073ull};

struct NativeKindInfo {
    int nprimes, word, is52, binary, ngroups;
    int ga[5], gb[5];  // prime indices of each mixed-radix group (gb = -1: single prime)
};
struct NativeCache;   // the workspace of the composed pipeline, per device (host_native.hip)

struct cntt_native {
    cntt_native_kind_t kind;
    NativeKindInfo info;
    size_t n = 0;
    std::vector<std::unique_ptr<cntt_plan32>> p32;
    std::vector<std::unique_ptr<cntt_plan64>> p64;
    CrtArgs crt{};
    // accumulating CRT of the whole-product kernel (native_fused.hpp, native_product_acc): constants, and the per-prime
    // parameters whose last-inverse-stage constants carry (M / P_i)^-1 / n
    AccArgs acc{};
    ModParams<uint32_t> mp_acc[10];
    bool has_acc = false;
    // Plan52 kinds (round 5): negacyclic_polymul returns the wrapping image of the EXACT integer product, which does not depend on the
    // primes it was computed with (native_fused.hpp, accumulating CRT) -- so it runs the whole-product kernel of the Plan32 kind with the
    // same words (30-bit primes: the faster arithmetic on this chip; the reference offers Plan52 for AVX-512 IFMA hosts).  fwd / inv of
    // the plan, whose 50-bit residues are visible, stay on its own primes.  Absent where the Plan32 kind does not exist (n < 32).
    std::unique_ptr<cntt_native> via32;
    std::shared_ptr<NativeCache> cache;
    size_t max_terms = 1;   // cntt_native_max_terms (cntt_ext.h)
    size_t rbytes() const { return info.is52 ? 8 : 4; }
    uint64_t prime(int i) const { return info.is52 ? PRIMES52[i] : (uint64_t)PRIMES32[i]; }
};

// ---------------------------------------------------------------------------------------------
// ... and product::Plan (host_product.hip)
// ---------------------------------------------------------------------------------------------
struct cntt_product {
    size_t n = 0;
    uint64_t modulus = 0;
    std::vector<uint64_t> primes;  // ascending, 1s removed
    std::vector<std::shared_ptr<cntt_plan32>> p32;
    std::vector<std::shared_ptr<cntt_plan64>> p64;
    std::vector<uint64_t> modular_inverses;  // src/product.rs:207-229
    ProductArgs args{};
    size_t len32() const { return (n / 2) * p32.size(); }          // ntt_domain_len_u32 src/product.rs:261-263
    size_t domain_len() const { return len32() + n * p64.size(); } // ntt_domain_len     src/product.rs:268-270
};

// ---------------------------------------------------------------------------------------------
// what crosses unit borders: the prime launchers (host_prime.hip) ...
// ---------------------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
template <class T> inline T shoup_of(T x, T p) { return (T)((((u128)x) << (sizeof(T) * 8)) / p); }
inline bool alt_tables(int cls) { return is_fp_class(cls) || cls == CLS_PM64 || cls == CLS_FPW; }
// transform class of the LDS-resident kernels for this plan (the global-stage path of larger sizes is integer-only)
template <class T> inline int transform_class(const PrimePlan<T> *pl) {
    if (pl->logn > MaxLdsLogN<T>::value) return (int)pl->mp.cls;
    if (pl->mp.fp == CLS_FPW && pl->logn > MAX_FPW_LOGN) return (int)pl->mp.cls;
    if (pl->mp.fp) return (int)pl->mp.fp;
    if (pl->mp.pm_c) return (int)CLS_PM64;
    return (int)pl->mp.cls;
}

// instantiated in host_prime.hip for (uint32_t, cntt_plan32) and (uint64_t, cntt_plan64); all on device pointers
template <class T, class PlanT> int plan_new(size_t n, T p, PlanT **out);
template <class T> int device_tables(const PrimePlan<T> *pl, DeviceTables<T> *out);
template <class T> int ntt_device(const PrimePlan<T> *pl, T *d, size_t batch, bool inv, hipStream_t st);
template <class T, int OP> int pointwise_device(const PrimePlan<T> *pl, T *a, const T *b, const T *c, size_t count, hipStream_t st);
template <class T> int mul_ntt_device(const PrimePlan<T> *pl, T *lhs, const T *rhs, size_t batch, hipStream_t st);
template <class T>
int external_product_device(const PrimePlan<T> *pl, T *out, const T *terms, const T *key, size_t nterms, size_t nout, size_t batch,
                            bool accumulate, hipStream_t st);

// ... and the native pieces (host_native.hip)
SplitArgs native_split_args(const cntt_native *pl, void *const *res);
int native_split_device(const cntt_native *pl, const void *value, void *const *res, size_t count, bool binary, hipStream_t st);
int native_crt_device(const cntt_native *pl, void *value, void *const *res, size_t count, hipStream_t st);
int native_ntt_device(const cntt_native *pl, void *const *res, size_t batch, bool inv, hipStream_t st);
// Plan32 kinds: the nprimes monomial tables of the multi-bit bootstrap on the current device (native_multibit.hpp), built on first use
int native_multibit_tables(const cntt_native *pl, const uint32_t **tab);

// CNTT_OK: enqueued; FUSED_NONE: no fused kernel for this plan / size (the caller composes)
constexpr int FUSED_NONE = -1;
// The six Plan32 kinds, the ones with fused kernels: cntt_native_kind_t -> the KIND parameter of NativeShape / launch_native_*, handed
// to f as a std::integral_constant.  hipErrorNotSupported for the Plan52 kinds.
template <class F> hipError_t with_plan32_kind(cntt_native_kind_t kind, F &&f) {
    switch (kind) {
    case CNTT_NATIVE32_PLAN32: return f(std::integral_constant<int, 0>{});
    case CNTT_NATIVE64_PLAN32: return f(std::integral_constant<int, 1>{});
    case CNTT_NATIVE128_PLAN32: return f(std::integral_constant<int, 2>{});
    case CNTT_NATIVE_BINARY32_PLAN32: return f(std::integral_constant<int, 3>{});
    case CNTT_NATIVE_BINARY64_PLAN32: return f(std::integral_constant<int, 4>{});
    case CNTT_NATIVE_BINARY128_PLAN32: return f(std::integral_constant<int, 5>{});
    default: return hipErrorNotSupported;
    }
}
// launch(kind, rc) enqueues the fused kernel `what` of the plan's kind: a CNTT_ code it stores in rc wins; its hipErrorNotSupported
// means FUSED_NONE
template <class F> int native_fused_launch(const cntt_native *pl, const char *what, F &&launch) {
    int rc = CNTT_OK;
    const hipError_t e = with_plan32_kind(pl->kind, [&](auto kind) { return launch(kind, rc); });
    if (rc != CNTT_OK) return rc;
    if (e == hipSuccess) return CNTT_OK;
    if (e != hipErrorNotSupported) return fail(CNTT_EDEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
    (void)hipGetLastError();
    return FUSED_NONE;
}
// tables of the accumulating-CRT kernels: the primes' twiddles with the parameters of build_acc_args and, with `key`, its planes
template <int KIND>
int native_acc_tables(const cntt_native *pl, const void *const *key, FusedTables<NativeShape<KIND>::KP> *Facc, KeyPlanes *K) {
    for (int i = 0; i < NativeShape<KIND>::KP; ++i) {
        DeviceTables<uint32_t> t;
        if (int rc = device_tables(pl->p32[(size_t)i].get(), &t)) return rc;
        Facc->twf[i] = t.fwd;
        Facc->twi[i] = t.inv;
        Facc->P[i] = pl->mp_acc[i];
        if (key) K->k[i] = static_cast<const uint32_t *>(key[i]);
    }
    return CNTT_OK;
}
#pragma GCC visibility pop
