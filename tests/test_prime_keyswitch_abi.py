"""C ABI of the prime plans' LWE keyswitch and keyswitch + bootstrap (include/cntt_prime_keyswitch.h): the header is plain C11, its six
names are declared and exported, the five existing headers keep their surface, every CNTT_EINVAL case is refused on host buffers by the
argument checks that precede any device call (outputs untouched, argument named), ks_pbs_workspace_bytes is the header's formula, the
Python wrappers panic on bad shapes, the plain-int model of the keyswitch (defined here, used by the GPU tests) satisfies the header's
phase identity, and the code object of the new kernel has no scratch and no spills.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from test_prime_pbs_model import P30, P32, P50, P62, PM64, lift, signed_digits, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEWH = os.path.join(INC, "cntt_prime_keyswitch.h")
CALLS = ["keyswitch_batch", "keyswitch_bootstrap_batch", "ks_pbs_workspace_bytes"]
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS}
SURFACE = {"cntt.h": 87, "cntt_ext.h": 2, "cntt_pbs.h": 5, "cntt_keyswitch.h": 3, "cntt_prime_pbs.h": 12}

# -- the model ----------------------------------------------------------------------------------------------------------------------
KS_ROWS = 128      # prime_keyswitch.hpp: PKS_ROWS


def chunk_words(base_log, levels):
    """mask words per chunk of the kernel: min(KS_ROWS, 2^(32 - base_log)) rows, rounded down to whole words"""
    return min(KS_ROWS, 1 << (32 - base_log)) // levels


def model_keyswitch(lwe, ksk, p, lin, lout, stride, beta, ell, batch):
    """the header's formula on Python ints: lwe batch x (lin + 1), ksk rows of `stride` words -> batch x (lout + 1) ints"""
    out = []
    for b in range(batch):
        row = lwe[b * (lin + 1):(b + 1) * (lin + 1)]
        acc = [0] * (lout + 1)
        for i in range(lin):
            for l, d in enumerate(signed_digits(int(row[i]), p, beta, ell)):
                if d:
                    base = (i * ell + l) * stride
                    for c in range(lout + 1):
                        acc[c] += d * int(ksk[base + c])
        out.extend(((int(row[lin]) if c == lout else 0) - acc[c]) % p for c in range(lout + 1))
    return out


def noiseless_ksk(rng, p, s_in, s_out, beta, ell, stride, noise=0):
    """row (i, l): a random mask and body = <mask, s_out> + s_in[i] 2^(W - beta l) + e, e uniform in [-noise, noise]"""
    W, lout = wbits(p), len(s_out)
    key = [0] * (len(s_in) * ell * stride)
    for i, si in enumerate(s_in):
        for l in range(1, ell + 1):
            base = (i * ell + l - 1) * stride
            mask = [rng.randrange(p) for _ in range(lout)]
            e = rng.randint(-noise, noise) if noise else 0
            key[base:base + lout] = mask
            key[base + lout] = (sum(m * s for m, s in zip(mask, s_out)) + si * (1 << (W - beta * l)) + e) % p
            for c in range(lout + 1, stride):
                key[base + c] = rng.randrange(p)       # padding: never read
    return key


def phase(ct, s, p):
    return (ct[-1] - sum(a * k for a, k in zip(ct[:-1], s))) % p


@pytest.mark.parametrize("p", [P62, PM64, P50, P32, P30, 12289, 97])
def test_model_satisfies_the_phase_identity_and_error_bound(p):
    rng = random.Random("ksmodel/%d" % p)
    W = wbits(p)
    for beta, ell in [(b, l) for b, l in ((1, 1), (2, 3), (3, 2), (8, 3), (16, 4), (31, 2), (W, 1)) if b * l <= W]:
        s = W - beta * ell
        lin, lout, batch = 5, 3, 3
        s_in, s_out = [rng.randrange(2) for _ in range(lin)], [rng.randrange(2) for _ in range(lout)]
        ksk = noiseless_ksk(rng, p, s_in, s_out, beta, ell, lout + 2)
        lwe = [rng.randrange(p) for _ in range(batch * (lin + 1))]
        out = model_keyswitch(lwe, ksk, p, lin, lout, lout + 2, beta, ell, batch)
        for b in range(batch):
            row = lwe[b * (lin + 1):(b + 1) * (lin + 1)]
            rs = []
            for x in row[:lin]:
                r2s = sum(d << (W - beta * (l + 1)) for l, d in enumerate(signed_digits(x, p, beta, ell)))    # r_i 2^s
                assert r2s % (1 << s) == 0 and abs(r2s - lift(x, p)) <= ((1 << s) >> 1)
                rs.append(r2s)
            want = (row[lin] - sum(si * r for si, r in zip(s_in, rs))) % p
            got = out[b * (lout + 1):(b + 1) * (lout + 1)]
            assert all(0 <= v < p for v in got) and phase(got, s_out, p) == want, (p, beta, ell, b)


# -- the surface --------------------------------------------------------------------------------------------------------------------
def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_declares_the_six():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", NEWH],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(NEW) == 6 and set(declarations(NEWH)) == NEW and len(declarations(NEWH)) == 6
    text = open(NEWH).read()
    assert re.search(r'^#include "cntt_prime_pbs.h"$', text, flags=re.M)
    assert "strict range" in text and "Barrett" in text and "2^(s-1)" in text and "never read" in text


def test_library_exports_the_six_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    for name, count in SURFACE.items():
        path = os.path.join(INC, name)
        decl = declarations(path)
        assert len(decl) == count, (name, len(decl))
        assert not (NEW & set(decl)) and "cntt_prime_keyswitch.h" not in open(path).read(), name


def test_cpp_mirror_declares_the_three_methods(tmp_path):
    """include/cntt.hpp: the three calls as members of cntt::prime32::Plan / prime64::Plan, instantiated by a translation unit"""
    src = tmp_path / "mirror.cpp"
    src.write_text("""#include "cntt.hpp"
template <class P, class T> size_t use(const P &pl, T *o, const T *i, const T *k, const T *lut, const T *bsk) {
    pl.keyswitch_batch(o, i, k, 5, 3, 4, 4, 2, 1, CNTT_MEM_HOST);
    pl.keyswitch_bootstrap_batch(o, i, k, 4, 4, 2, lut, false, bsk, 3, 1, 8, 2, 1, nullptr, 0, CNTT_MEM_HOST, nullptr);
    return pl.ks_pbs_workspace_bytes(3, 1, 2, 1);
}
template size_t use(const cntt::prime64::Plan &, uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *, const uint64_t *);
template size_t use(const cntt::prime32::Plan &, uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *, const uint32_t *);
""")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_pbs_abi.py reads its unit: the keyswitch kernel on u32 and
    u64 words, neither with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_keyswitch.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "ks.fat"), str(tmp_path / "ks.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = []
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) + int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        seen.append(name)
    assert len(seen) == 2 and sum("prime_keyswitch_kernelIjE" in s for s in seen) == 1 and sum("prime_keyswitch_kernelImE" in s for s in seen) == 1, seen


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_ks_pbs_workspace_bytes_is_the_formula_of_the_header(mod, p, wb):
    def up(x):
        return (x + 255) // 256 * 256

    for n, L, k, levels, batch in ((32, 0, 1, 1, 1), (1024, 7, 1, 3, 5), (256, 630, 2, 4, 37), (2048, 3, 0, 2, 1000)):
        plan = mod.Plan.try_new(n, p)
        want = plan.pbs_workspace_bytes(L, k, levels, batch) + up(batch * (L + 1) * wb)
        assert plan.ks_pbs_workspace_bytes(L, k, levels, batch) == want, (n, L, k, levels, batch)
    assert cntt.lib().cntt_prime64_ks_pbs_workspace_bytes(None, 5, 1, 2, 3) == 0
    assert cntt.lib().cntt_prime32_ks_pbs_workspace_bytes(None, 5, 1, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, L, K, B = 32, 3, 1, 2
BIG = K * N


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments of both calls at n = 32, L = 3, k = 1, batch = 2; outputs filled with 7."""

    def __init__(self, bits=64, p=P62, levels=2, ks_levels=3):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.levels, self.ks_levels = levels, ks_levels
        self.lut = np.arange((K + 1) * N, dtype=self.dtype)
        self.bsk = np.zeros(L * (K + 1) * levels * (K + 1) * N, dtype=self.dtype)
        self.ksk = np.zeros(BIG * ks_levels * (L + 1), dtype=self.dtype)
        self.small = np.full(B * (L + 1), 7, dtype=self.dtype)
        self.lwe_in = np.arange(B * (BIG + 1), dtype=self.dtype)
        self.lwe_out = np.full(B * (BIG + 1), 7, dtype=self.dtype)
        self.ws = np.zeros(self.plan.ks_pbs_workspace_bytes(L, K, levels, B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def keyswitch(self, plan="own", out="own", inp="own", ksk="own", lin=BIG, lout=L, stride=L + 1, base_log=4, levels=None, batch=B):
        out = self.small if isinstance(out, str) else out
        inp = self.lwe_in if isinstance(inp, str) else inp
        ksk = self.ksk if isinstance(ksk, str) else ksk
        return self.fn("keyswitch_batch")(self.plan._h if plan == "own" else None, ptr(out), ptr(inp), ptr(ksk), lin, lout, stride, base_log,
                                          self.ks_levels if levels is None else levels, batch, 0, None)

    def combined(self, plan="own", out="own", inp="own", ksk="own", stride=L + 1, ks_base_log=4, ks_levels=None, lut="own", bsk="own",
                 lwe_dim=L, glwe_dim=K, base_log=8, levels=None, batch=B, ws=None, ws_bytes=None):
        out = self.lwe_out if isinstance(out, str) else out
        inp = self.lwe_in if isinstance(inp, str) else inp
        ksk = self.ksk if isinstance(ksk, str) else ksk
        lut = self.lut if isinstance(lut, str) else lut
        bsk = self.bsk if isinstance(bsk, str) else bsk
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("keyswitch_bootstrap_batch")(self.plan._h if plan == "own" else None, ptr(out), ptr(inp), ptr(ksk), stride, ks_base_log,
                                                    self.ks_levels if ks_levels is None else ks_levels, ptr(lut), 0, ptr(bsk), lwe_dim,
                                                    glwe_dim, base_log, self.levels if levels is None else levels, batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.small == 7).all() and (self.lwe_out == 7).all())


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30)])
def test_keyswitch_refuses_every_invalid_argument(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    cases = [
        (dict(plan=None), "plan"),
        (dict(out=None), "lwe_out"),
        (dict(inp=None), "lwe_in"),
        (dict(ksk=None), "ksk"),
        (dict(base_log=0), "base_log"),
        (dict(levels=0), "levels"),
        (dict(base_log=32, levels=1), "base_log"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=1, levels=W + 1), "base_log * levels"),
        (dict(stride=L), "row_stride"),
        (dict(lin=1 << 31, levels=2, base_log=1), "2^32"),
        (dict(inp=c.small), "lwe_out overlaps lwe_in"),
        (dict(ksk=c.small), "lwe_out overlaps ksk"),
    ]
    for kw, word in cases:
        assert c.keyswitch(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched(), kw
    assert c.keyswitch(batch=0) == 0 and c.untouched()
    assert c.keyswitch(batch=0, out=None, inp=None, ksk=None) == 0


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30)])
def test_combined_call_refuses_every_invalid_argument(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    inside = c.ws[:B * (BIG + 1) * w].view(c.dtype)         # an LWE batch that lives in the workspace
    cases = [
        (dict(plan=None), "plan"),
        (dict(out=None), "lwe_out"),
        (dict(inp=None), "lwe_in"),
        (dict(ksk=None), "ksk"),
        (dict(lut=None), "lut"),
        (dict(bsk=None), "bsk_ntt"),
        (dict(ks_base_log=0), "ks_base_log"),
        (dict(ks_levels=0), "ks_levels"),
        (dict(ks_base_log=32, ks_levels=1), "ks_base_log"),
        (dict(ks_base_log=W // 3 + 1, ks_levels=3), "ks_base_log * ks_levels"),
        (dict(stride=L), "row_stride"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W, levels=2), "exceeds the bit length"),
        (dict(ws=c.ws[1:]), "workspace"),
        (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
        (dict(ws=c.ws, ws_bytes=c.plan.pbs_workspace_bytes(L, K, c.levels, B)), "workspace_bytes"),
        (dict(inp=c.lwe_out), "lwe_out overlaps lwe_in"),
        (dict(ksk=c.lwe_out), "lwe_out overlaps ksk"),
        (dict(lut=c.lwe_out[:(K + 1) * N]), "lwe_out overlaps lut"),
        (dict(out=inside, ws=c.ws), "lwe_out overlaps workspace"),
        (dict(inp=inside, ws=c.ws), "lwe_in overlaps workspace"),
        (dict(ksk=c.ws.view(c.dtype), ws=c.ws), "ksk overlaps workspace"),
        (dict(lut=inside[:(K + 1) * N], ws=c.ws), "lut overlaps workspace"),
        # glwe_dim is bounded before it is multiplied into the keyswitch's dimension, so before the keyswitch's digits too; then the rows
        (dict(glwe_dim=(1 << 32) - 1), "glwe_dim too large"),
        (dict(glwe_dim=(1 << 32) - 1, ks_base_log=0), "glwe_dim too large"),
        (dict(glwe_dim=(1 << 32) // N, ks_levels=1), "lwe_dim_in * ks_levels"),
        (dict(glwe_dim=(1 << 32) // N, ks_levels=1, stride=L), "row_stride"),
    ]
    for kw, word in cases:
        assert c.combined(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched(), kw
    assert c.combined(batch=0) == 0 and c.untouched()


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    plan = mod.Plan.try_new(N, p)
    dt = plan.dtype
    z = lambda count, t=dt: np.zeros(count, dtype=t)
    lin, lout, ell, batch = 5, 3, 2, 2
    good = dict(lwe_out=z(batch * (lout + 1)), lwe_in=z(batch * (lin + 1)), ksk=z(lin * ell * (lout + 1)), lwe_dim_in=lin, lwe_dim_out=lout,
                base_log=4, levels=ell)
    for kw in (dict(lwe_in=z(batch * (lin + 1) + 1)), dict(lwe_out=z(batch * (lout + 1) - 1)), dict(ksk=z(lin * ell * (lout + 1) - 1)),
               dict(row_stride=lout), dict(row_stride=lout + 2), dict(levels=0), dict(base_log=0), dict(lwe_dim_in=-1),
               dict(lwe_out=z(batch * (lout + 1), np.uint16))):
        with pytest.raises((Panic, TypeError)):
            plan.keyswitch_batch(**{**good, **kw})
    big = K * N
    goodc = dict(lwe_out=z(batch * (big + 1)), lwe_in=z(batch * (big + 1)), ksk=z(big * ell * (L + 1)), ks_base_log=4, ks_levels=ell,
                 lut=z((K + 1) * N), bsk_ntt=z(L * (K + 1) * 2 * (K + 1) * N), lwe_dim=L, glwe_dim=K, base_log=8, levels=2)
    for kw in (dict(lwe_out=z(batch * (big + 1) + 1)), dict(lwe_in=z(batch * (big + 1) - 1), lwe_out=z(batch * (big + 1) - 1)),
               dict(ksk=z(big * ell * (L + 1) - 1)), dict(lut=z((K + 1) * N + 1)), dict(bsk_ntt=z(7)), dict(ks_levels=0), dict(ks_base_log=0),
               dict(row_stride=L), dict(glwe_dim=-1)):
        with pytest.raises(Panic):
            plan.keyswitch_bootstrap_batch(**{**goodc, **kw})
    with pytest.raises(Panic):
        plan.ks_pbs_workspace_bytes(-1, 1, 1, 1)
