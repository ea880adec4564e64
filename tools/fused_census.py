#!/usr/bin/env python3
"""Section-by-section VALU census of the tile loop of the fused prime64 product at N = 1024, mul_kernel_wp<u64, 10, lazy, 768, 3>
(gfx950 ISA as hipcc emits it; compile only, no GPU).  Next to tools/bfly_census.py, which counts ONE butterfly: this one says where
the instructions of the whole kernel go.

Boundaries come from differencing builds, not from markers in the library: a census kernel restates the tile loop of MulWp::run from the
library's own building blocks (gather / stages / scatter / mul_fused ...) with a bit mask that replaces one section at a time by an empty
asm statement which keeps the registers alive (zero instructions), and the section's cost is (nothing stubbed) - (that section stubbed).
What is left with every section stubbed is the load / unpack, the store and the loop itself.  The census kernel with nothing stubbed must
have the real kernel's counts: the tool checks that, so it cannot drift away from MulWp::run unnoticed.  Sections overlap a little where
hipcc shares an address or a move between two of them: the difference between the whole and the sum is printed as "shared / interaction".

    python tools/fused_census.py [--before DIR_OF_ANOTHER_CSRC] > profiles/r17_fused_join_census.txt

--before: the same census of another source tree (the parent commit's concrete-ntt_amd/csrc) in a second column."""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (bit, name)
SECTIONS = [(0, "forward pass 0"), (1, "forward pass 1"), (2, "forward pass 2"), (3, "rhs gather"), (4, "pointwise"),
            (5, "inverse pass 0"), (6, "inverse pass 1"), (7, "inverse pass 2 (with 1/N)"), (8, "finish"),
            (9, "exchange addressing (LDS scatter / gather)")]
ALL = (1 << 10) - 1
MASKS = [0] + [1 << b for b, _ in SECTIONS] + [ALL]

SRC = r'''
#include <type_traits>
#include "%(csrc)s/ntt_kernel.hpp"
using namespace cntt;
using T = uint64_t;
using K = MulWp<T, 10, CLS_LAZY, 768>;
// HAS_JOIN: the tree has the round-17 join (MulWp::JOIN, mul_fused_join, NORM_JOIN); the parent's does not

template <int STUB> struct Census {
    using F = K::F; using I = K::I; using FB = K::FB; using IB = K::IB;
    static constexpr int E = K::E, NPASS = K::NPASS, PPB = K::PPB, LOGN = 10, TPP = K::TPP;
    static constexpr uint32_t FULL = K::FULL, RM0 = K::RM0, RMM = K::RMM, RML = K::RML, IO_RM = K::IO_RM;
    static constexpr bool EXCH = !(STUB & (1 << 9));
#if HAS_JOIN
    static_assert(K::JOIN, "the headline shape takes the join");
    static constexpr int NORM_LAST = NORM_JOIN;
#else
    static constexpr bool NORM_LAST = true;
#endif
    template <class D> static __device__ __forceinline__ void keep(D (&r)[E]) {
#pragma unroll
        for (int j = 0; j < E; ++j) asm volatile("" : "+v"(r[j]));
    }
    // NttWp::pass, one section per pass
    template <class W, int BIT0, int KP, class D>
    static __device__ __forceinline__ void passes(D (&r)[E], D *lds, uint32_t tid, const TwPair<D> *tw, const TwPair<D> *img, const ModParams<D> &P) {
        using B = typename W::B;
        constexpr uint32_t RM = B::S::RMASK[KP], CM = FULL & ~RM;
        const uint32_t ebase = pdep<CM>(tid);
        if constexpr (KP > 0 && EXCH) B::template gather<RM>(r, (const D *)lds, ebase, true);
        if constexpr (STUB & (1 << (BIT0 + KP))) keep(r);
        else if constexpr (BIT0 == 0) B::template stages<KP, 0, true, false, 0>(r, ebase, 0u, 0u, tw, P, tid, img);
        else B::template stages<KP, 0, true, NORM_LAST, 0>(r, ebase, 0u, 0u, tw, P, tid, img);
        if constexpr (KP < NPASS - 1) {
            if constexpr (EXCH) {
                if constexpr (KP > 0) W::wsync();
                B::template scatter<RM>(r, lds, ebase, true);
                W::wsync();
            }
            passes<W, BIT0, KP + 1>(r, lds, tid, tw, img, P);
        }
    }
    static __device__ __forceinline__ void run(T *__restrict__ lhs, const T *__restrict__ rhs_ntt, const TwPair<T> *__restrict__ twf,
                                               const TwPair<T> *__restrict__ twi, const ModParams<T> &P, uint32_t nsub, const WalkArgs &W,
                                               T *lds_all, TwPair<T> *imgf, TwPair<T> *imgi) {
        FB::fill_image(imgf, twf);
        IB::fill_image(imgi, twi);
        __syncthreads();
        [[maybe_unused]] uint64_t pinv = 0;
#if HAS_JOIN
        pinv = mul_join_pinv(P);
#endif
        const ModParams<T> Pi = mul_inv_params<T, CLS_LAZY>(P);
        const uint32_t tid = threadIdx.x & (TPP - 1);
        const uint32_t pl = threadIdx.x / TPP;
        T *lds = lds_all + (size_t)pl * FB::LDS_WORDS_1;
        constexpr uint32_t CM0 = FULL & ~RM0, CMM = FULL & ~RMM, CML = FULL & ~RML, CMIO = FULL & ~IO_RM;
        const uint32_t ebase0 = pdep<CM0>(tid), ebaseM = pdep<CMM>(tid), ebaseL = pdep<CML>(tid), ebaseIO = pdep<CMIO>(tid);
        const uint32_t voffIO = ((pl << LOGN) + ebaseIO) * (uint32_t)sizeof(T);
        T r[E];
#pragma unroll
        for (int j = 0; j < E; ++j) r[j] = 0;
        uint32_t trips, lbase, step;
        F::walk_plan(W, trips, lbase, step);
        uint32_t base = W.full ? blockIdx.x * PPB : lbase;
        if (trips) {
            const uint32_t last = nsub - 1u - base;
            const uint32_t pl0 = pl < last ? pl : last;
            typename FB::AsyncVec v0[E / FB::MAXV];
            FB::template gather_async<IO_RM>(v0, (const T *)(lhs + ((size_t)base << LOGN)), ((pl0 << LOGN) + ebaseIO) * (uint32_t)sizeof(T));
            FB::template wait_async<0>(v0);
            FB::unpack_async(r, v0);
        }
        constexpr int NST = E / FB::template vec_elems<IO_RM>();
        for (uint32_t t = 0; t < trips; ++t) {
            const uint32_t sub = base + pl;
            const uint32_t bnext = t + 1u < W.full ? base + step : lbase;
            const bool more = t + 1u < trips;
            T *tbase = lhs + ((size_t)base << LOGN);
            typename FB::AsyncVec vn[E / FB::MAXV];
            if (more) {
                const uint32_t last = nsub - 1u - bnext;
                const uint32_t pln = pl < last ? pl : last;
                FB::template gather_async<IO_RM>(vn, (const T *)(lhs + ((size_t)bnext << LOGN)), ((pln << LOGN) + ebaseIO) * (uint32_t)sizeof(T));
            }
#pragma unroll
            for (int j = 0; j < E; ++j) r[j] = Bfly<T, CLS_LAZY>::load_fix(r[j], P);
            if constexpr (RM0 != IO_RM && EXCH) {
                FB::template scatter<IO_RM>(r, lds, ebaseIO, true);
                F::wsync();
                FB::template gather<RM0>(r, (const T *)lds, ebase0, true);
                F::wsync();
            }
            passes<F, 0, 0>(r, lds, tid, twf, imgf, P);
            {
                const uint32_t lastc = nsub - 1u - base;
                const uint32_t plc = pl < lastc ? pl : lastc;
                T b[E];
                if constexpr (STUB & (1 << 3)) {
#pragma unroll
                    for (int j = 0; j < E; ++j) b[j] = r[(j + 1) %% E];
                } else {
                    FB::template gather_tile<RMM>(b, rhs_ntt + ((size_t)base << LOGN), ((plc << LOGN) + ebaseM) * (uint32_t)sizeof(T));
                }
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    if constexpr (STUB & (1 << 4)) asm volatile("" : "+v"(r[j]) : "v"(b[j]));
#if HAS_JOIN
                    else r[j] = mul_fused_join(r[j], b[j], P, pinv);
#else
                    else r[j] = mul_fused<T, CLS_LAZY>(r[j], b[j], P);
#endif
                }
            }
            if constexpr (EXCH) F::wsync();
            passes<I, 5, 0>(r, lds, tid, twi, imgi, Pi);
            if constexpr (!(STUB & (1 << 8))) {
#pragma unroll
                for (int j = 0; j < E; ++j) r[j] = Bfly<T, CLS_LAZY>::finish_inv(r[j], Pi);
            }
            if constexpr (RML != IO_RM && EXCH) {
                F::wsync();
                FB::template scatter<RML>(r, lds, ebaseL, true);
                F::wsync();
                FB::template gather<IO_RM>(r, (const T *)lds, ebaseIO, true);
            }
            if (sub < nsub) FB::template scatter_tile<IO_RM>(r, tbase, voffIO);
            if constexpr (EXCH) F::wsync();
            if (more) {
                FB::template wait_async<NST>(vn);
                FB::unpack_async(r, vn);
            }
            base = bnext;
        }
    }
};
template <int STUB>
__global__ __launch_bounds__(768, 3) void census_k(T *__restrict__ lhs, const T *__restrict__ rhs_ntt, const TwPair<T> *__restrict__ twf,
                                                   const TwPair<T> *__restrict__ twi, const ModParams<T> P, uint32_t nsub, const WalkArgs W) {
    __shared__ __attribute__((aligned(16))) T lds[(size_t)K::PPB * K::FB::LDS_WORDS_1];
    __shared__ __attribute__((aligned(16))) TwPair<T> imgf[K::FB::IMG_ENTRIES];
    __shared__ __attribute__((aligned(16))) TwPair<T> imgi[K::IB::IMG_ENTRIES];
    Census<STUB>::run(lhs, rhs_ntt, twf, twi, P, nsub, W, lds, imgf, imgi);
}
%(inst)s
template __global__ void cntt::mul_kernel_wp<T, 10, CLS_LAZY, 768, 3>(T *, const T *, const TwPair<T> *, const TwPair<T> *, const ModParams<T>, uint32_t, const WalkArgs);
'''

MUL_RE = re.compile(r"v_(mad_u64_u32|mul_hi_u32|mul_lo_u32)")


def functions(text):
    """{symbol: lines} of an assembly file"""
    out, name = {}, None
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif ln.startswith(".Lfunc_end"):
            name = None
        elif name:
            out[name].append(ln)
    return out


def tile_loop(lines):
    """the longest loop (label ... last backward branch to it) that stores to global memory: the tile loop"""
    labels = {}
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = i
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and labels.get(m.group(1), i) < i:
            j = labels[m.group(1)]
            if any("global_store" in x for x in lines[j:i]) and (best is None or i - j > best[1] - best[0]):
                best = (j, i)
    assert best, "no tile loop found"
    return lines[best[0]:best[1] + 1]


def count(lines):
    c = collections.Counter()
    for ln in lines:
        ln = ln.strip()
        if not ln or ln[0] in ".;/" or ln.endswith(":"):
            continue
        c[re.sub(r"_e(32|64)$", "", ln.split()[0])] += 1
    return c


def summary(c):
    """(VALU, multiplies among them, s_nop, LDS operations, global memory operations)"""
    valu = sum(v for k, v in c.items() if k.startswith("v_"))
    mul = sum(v for k, v in c.items() if MUL_RE.match(k))
    return (valu, mul, c["s_nop"], sum(v for k, v in c.items() if k.startswith("ds_")),
            sum(v for k, v in c.items() if k.startswith("global_")))


def census(csrc):
    inst = "\n".join("template __global__ void census_k<%d>(T *, const T *, const TwPair<T> *, const TwPair<T> *, const ModParams<T>, "
                     "uint32_t, const WalkArgs);" % m for m in MASKS)
    with tempfile.TemporaryDirectory() as tmp:
        src, out = os.path.join(tmp, "c.hip"), os.path.join(tmp, "c.s")
        open(src, "w").write(SRC % {"csrc": csrc, "inst": inst})
        has_join = "mul_fused_join" in open(os.path.join(csrc, "ntt_arith.hpp")).read()
        subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-DHAS_JOIN=%d" % has_join, "-S", "--cuda-device-only", src,
                        "-o", out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    fn = functions(text)
    res, regs = {}, {}
    for sym, lines in fn.items():
        m = re.search(r"census_kILi(\d+)E", sym)
        key = int(m.group(1)) if m else ("real" if "mul_kernel_wp" in sym else None)
        if key is not None:
            res[key] = count(tile_loop(lines))
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text):
        if "mul_kernel_wp" in m.group(1):
            regs = {"vgpr": int(m.group(2)), "spill": int(m.group(3))}
    return res, regs


def rows(res):
    full, real = summary(res[0]), summary(res["real"])
    # (the s_nop padding may differ by a wait state or two: it depends on how hipcc orders independent instructions)
    assert real[:2] == full[:2] and real[3:] == full[3:], ("the census kernel no longer restates MulWp::run", real, full)
    out, tot = [], [0] * 5
    for b, name in SECTIONS:
        s = summary(res[1 << b])
        d = [f - x for f, x in zip(full, s)]
        out.append((name, d))
        tot = [a + x for a, x in zip(tot, d)]
    skel = list(summary(res[ALL]))
    out.append(("load / unpack, store, loop (all of the above stubbed)", skel))
    tot = [a + x for a, x in zip(tot, skel)]
    out.append(("shared / interaction (whole - sum)", [f - x for f, x in zip(full, tot)]))
    out.append(("whole tile loop of the census kernel", list(full)))
    out.append(("WHOLE tile loop of mul_kernel_wp itself", list(real)))
    return out


def main():
    before = None
    if "--before" in sys.argv:
        before = sys.argv[sys.argv.index("--before") + 1]
    cols = []
    if before:
        cols.append(("before", before))
    cols.append(("after" if before else "this tree", os.path.join(ROOT, "concrete-ntt_amd", "csrc")))
    print(__doc__.split("\n\n")[0])
    print("Per thread and polynomial (16 coefficients per thread, 64 threads per polynomial).  Columns: VALU instructions / multiplies among")
    print("them (v_mad_u64_u32, v_mul_hi_u32, v_mul_lo_u32) / s_nop / LDS operations / global-memory operations.\n")
    data = []
    for title, csrc in cols:
        res, regs = census(csrc)
        data.append((title, rows(res), regs, res))
    head = "%-56s" % "section" + "".join("  %-28s" % t for t, _, _, _ in data)
    print(head)
    for i in range(len(data[0][1])):
        line = "%-56s" % data[0][1][i][0]
        for _, r, _, _ in data:
            line += "  %5d /%5d /%4d /%4d /%3d " % tuple(r[i][1])
        print(line)
    print()
    for title, _, regs, res in data:
        print("%s: mul_kernel_wp<u64, 10, lazy, 768, 3>: %d VGPRs, %d spilled" % (title, regs.get("vgpr", -1), regs.get("spill", -1)))
    for title, _, _, res in data:
        print("\n%s, whole tile loop by opcode:" % title)
        for op, v in sorted(res["real"].items(), key=lambda kv: -kv[1]):
            if op.startswith("v_") or op == "s_nop":
                print("    %-24s %5d" % (op, v))


if __name__ == "__main__":
    main()
