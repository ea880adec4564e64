// libcntt_hip.so host side, the part every other host unit leans on: the last error, version / device count, the testing switchboard,
// the batch partition, the element-wise grid and the fill kernels.  (Plans and launch logic: host_prime / host_native /
// host_native_ext / host_product .hip; what they share: host_common.hpp.)
// There is no CPU compute path in this library: every transform runs in the HIP kernels, and every
// entry point that needs a GPU fails with CNTT_EDEVICE when none is present.
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "aux_kernels.hpp"
#include "host_common.hpp"

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char *cntt_last_error(void) { return g_err.c_str(); }
#include "build_hash.inc"  // CNTT_CSRC_HASH: sha256 of the csrc/ sources this library was built from (Makefile)
extern "C" const char *cntt_version(void) { return "cntt-hip 0.3 (gfx950) csrc:" CNTT_CSRC_HASH; }
extern "C" int cntt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---------------------------------------------------------------------------------------------
// testing only: the kernel-selection switchboard (ntt_launch.hpp DebugSwitch).  Plain atomics: set from a test or an A/B tool through
// cntt_debug_set(), read where a path is chosen (the two class switches at plan creation, the rest at the call).  Nothing here, or
// anywhere else in the library, reads the process environment.
// ---------------------------------------------------------------------------------------------
namespace {
struct SwitchDef { const char *name; int dflt; };
constexpr SwitchDef kSwitches[DBG_COUNT] = {
    {"fp", 1}, {"pm64", 1}, {"blk", 1}, {"mul32_blk", 1}, {"ext32_blk", 1}, {"ext_one", 1}, {"ext_split", -1}, {"native_acc", 1},
    {"product_fused", -1}, {"plan52_via32", 1}, {"native_ext", 1}, {"native_gadget", 0}, {"walk_split", 1}, {"autom_lds", 1}};
std::atomic<int> g_switch[DBG_COUNT] = {{1}, {1}, {1}, {1}, {1}, {1}, {-1}, {1}, {-1}, {1}, {1}, {0}, {1}, {1}};
int switch_index(const char *key) {
    if (!key) return -1;
    for (int i = 0; i < (int)DBG_COUNT; ++i)
        if (std::strcmp(key, kSwitches[i].name) == 0) return i;
    return -1;
}
}  // namespace
int cntt::debug_switch(DebugSwitch key) { return g_switch[key].load(std::memory_order_relaxed); }
extern "C" int cntt_debug_set(const char *key, int value) {
    if (key && std::strcmp(key, "reset") == 0) {
        for (int i = 0; i < (int)DBG_COUNT; ++i) g_switch[i].store(kSwitches[i].dflt);
        return CNTT_OK;
    }
    const int i = switch_index(key);
    if (i < 0) return fail(CNTT_EINVAL, "cntt_debug_set: unknown switch '%s'", key ? key : "(null)");
    if (value < -1 || value > 1) return fail(CNTT_EINVAL, "cntt_debug_set: %s takes -1 (library default), 0 or 1", key);
    g_switch[i].store(value < 0 ? kSwitches[i].dflt : value);
    return CNTT_OK;
}
extern "C" int cntt_debug_get(const char *key, int *value) {
    const int i = switch_index(key);
    if (i < 0 || !value) return fail(CNTT_EINVAL, "cntt_debug_get: unknown switch '%s'", key ? key : "(null)");
    *value = g_switch[i].load();
    return CNTT_OK;
}

// ---------------------------------------------------------------------------------------------
// batch partition over the devices of a node: contiguous shards, remainders to the low ranks -- the arithmetic of
// concrete-ntt_amd/shard.py shard_bounds(), for C / Rust callers that drive several devices themselves (examples/multi_device.cpp)
// ---------------------------------------------------------------------------------------------
extern "C" int cntt_shard_bounds(size_t batch, int world, int rank, size_t *begin, size_t *end) {
    if (world < 1 || rank < 0 || rank >= world || !begin || !end) return fail(CNTT_EINVAL, "cntt_shard_bounds: need 0 <= rank < world and non-NULL outputs");
    const size_t base = batch / (size_t)world, rem = batch % (size_t)world, r = (size_t)rank;
    *begin = r * base + (r < rem ? r : rem);
    *end = *begin + base + (r < rem ? 1 : 0);
    return CNTT_OK;
}

extern "C" unsigned cntt_ew_grid(size_t work_items) { return ew_grid(work_items); }   // host_common.hpp

// ---------------------------------------------------------------------------------------------
// fill
// ---------------------------------------------------------------------------------------------
extern "C" int cntt_fill_uniform_u64(uint64_t *dst, size_t count, uint64_t bound, uint64_t seed, void *st) {
    if (!dst && count) return fail(CNTT_EINVAL, "dst is NULL");
    if (!count) return CNTT_OK;
    hipLaunchKernelGGL((fill_uniform_kernel<uint64_t>), dim3(ew_grid(count)), dim3(256), 0, (hipStream_t)st, dst, count,
                       bound, seed);
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}
extern "C" int cntt_fill_uniform_u32(uint32_t *dst, size_t count, uint32_t bound, uint64_t seed, void *st) {
    if (!dst && count) return fail(CNTT_EINVAL, "dst is NULL");
    if (!count) return CNTT_OK;
    hipLaunchKernelGGL((fill_uniform_kernel<uint32_t>), dim3(ew_grid(count)), dim3(256), 0, (hipStream_t)st, dst, count,
                       bound, seed);
    HIP_TRY(hipGetLastError());
    return CNTT_OK;
}
