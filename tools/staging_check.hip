// Stand-alone check of Staging and StreamBlock (concrete-ntt_amd/csrc/host_common.hpp) on a machine WITHOUT a GPU, where every
// allocation of the HIP runtime fails: the failure paths of the host mode and the no-runtime-call contract of the device mode, under
// the host sanitizers.  Never loaded into Python; it brings its own fail() (the library's lives in host_core.hip).  Build and run from
// the repository root:
//     /opt/rocm/bin/hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -fsanitize=address,undefined tools/staging_check.hip -o tools/staging_check
//     tools/staging_check
// (the second -fsanitize, outside -Xarch_host, is for the link step).  Prints one line per check and "staging_check: ok"; exit status 1
// on the first check that does not hold.  On a machine with a GPU the host-mode half does not apply and the program says so.
#include <cstdarg>
#include <cstdio>

#include "../concrete-ntt_amd/csrc/host_common.hpp"

static char g_msg[256];
int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}

static int g_bad = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        const bool ok_ = (cond);                                                \
        std::printf("%s  %s\n", ok_ ? "ok  " : "FAIL", #cond);                  \
        if (!ok_) g_bad = 1;                                                    \
    } while (0)

int main() {
    char a[64] = {1}, b[64] = {2}, c[64] = {3}, w[64];
    void *probe = nullptr;
    const bool no_gpu = hipMalloc(&probe, 16) != hipSuccess;
    if (!no_gpu) (void)hipFree(probe);
    (void)hipGetLastError();

    std::printf("-- device mode: the caller's pointers, no runtime call\n");
    {
        Staging s(CNTT_MEM_DEVICE, nullptr);
        CHECK(!s.host());
        CHECK(s.in(a, sizeof a) == a);
        CHECK(s.out(b, sizeof b) == b);
        CHECK(s.inout(c, sizeof c) == c);
        CHECK(s.in(nullptr, 0) == nullptr && s.in(nullptr, 64) == nullptr);   // an absent operand stays absent
        CHECK(s.out(nullptr, 64) == nullptr && s.inout(nullptr, 64) == nullptr);
        CHECK(s.workspace(w, sizeof w) == w);
        CHECK(s.workspace(w, sizeof w, false) == w);
        CHECK(s.workspace(nullptr, 1 << 20, false) == nullptr);
        CHECK(s.status() == CNTT_OK);
        CHECK(s.finish() == CNTT_OK);   // a synchronise would fail without a GPU
        CHECK(a[0] == 1 && b[0] == 2 && c[0] == 3);
    }
    if (no_gpu) {
        std::printf("-- device mode: a workspace of its own cannot be had here\n");
        Staging s(CNTT_MEM_DEVICE, nullptr);
        g_msg[0] = 0;
        CHECK(s.workspace(nullptr, 4096) == nullptr);
        CHECK(s.status() == CNTT_EDEVICE);
        CHECK(std::strstr(g_msg, "hipMallocAsync") && std::strstr(g_msg, "4096"));
        CHECK(s.in(a, sizeof a) == a);   // still the caller's pointer: the call stops at status()
        CHECK(s.workspace(nullptr, 4096) == nullptr && s.finish() == CNTT_EDEVICE);
        StreamBlock blk(nullptr);
        CHECK(blk.alloc(256) == CNTT_EDEVICE && blk.get() == nullptr);
    }   // the destructors release nothing: no block was made
    if (no_gpu) {
        std::printf("-- host mode: the first allocation fails, everything after it is refused\n");
        for (int first = 0; first < 4; ++first) {
            Staging s(CNTT_MEM_HOST, nullptr);
            g_msg[0] = 0;
            CHECK(s.host() && s.status() == CNTT_OK);
            void *p = first == 0 ? s.in(a, sizeof a) : first == 1 ? s.out(b, sizeof b) : first == 2 ? s.inout(c, sizeof c) : s.workspace(w, sizeof w);
            CHECK(p == nullptr);
            CHECK(s.status() == CNTT_EDEVICE);
            CHECK(std::strstr(g_msg, "hipMalloc(64) failed"));
            CHECK(!s.in(a, sizeof a) && !s.out(b, sizeof b) && !s.inout(c, sizeof c) && !s.alloc(0) && !s.workspace(nullptr, 64, false));
            CHECK(s.status() == CNTT_EDEVICE && s.finish() == CNTT_EDEVICE && s.finish() == CNTT_EDEVICE);
        }   // each destructor frees nothing, and nothing twice
        CHECK(a[0] == 1 && b[0] == 2 && c[0] == 3);
    } else {
        std::printf("-- a GPU is present: the host-mode failure half does not apply\n");
    }
    std::printf(g_bad ? "staging_check: FAILED\n" : "staging_check: ok\n");
    return g_bad;
}
