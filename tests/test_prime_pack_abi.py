"""C ABI of the prime plans' LWE-to-GLWE packing keyswitch (include/cntt_prime_pack.h): the header is plain C11, its four names are
declared and exported, the existing headers keep their surface, every CNTT_EINVAL case is refused on host buffers by the argument
checks that precede any device call (output poison intact, argument named), pack_workspace_bytes is the header's formula, the Python
wrappers panic on bad shapes, the C++ mirror forwards its arguments, the code object of the new unit has four kernels without scratch
or spills -- and the plain-int model of tests/prime_pack_model.py (matrix form against the header's formula written naively, the
phase identity, the kernel's negated digits against -digits(x) mod p) is checked against its specification.  No GPU needed."""
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
from prime_pack_model import (C, HEADER, P31, PACK_TERMS, PG64, gadget_offset, kernel_negated_digits, model_pack_batch, model_pack_literal,
                              negacyclic, noise_free_key, workspace_bytes)
from test_prime_pbs_model import P30, P32, P50, P62, P63, PM64, edge_words, lift, signed_digits, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CALLS = ["pack_keyswitch_batch", "pack_workspace_bytes"]
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS}
SURFACE = {"cntt.h": 87, "cntt_ext.h": 2, "cntt_pbs.h": 5, "cntt_keyswitch.h": 3, "cntt_pack.h": 2, "cntt_prime_pbs.h": 12,
           "cntt_prime_keyswitch.h": 6}


# -- the model against its specification --------------------------------------------------------------------------------------------
def settings(p):
    W = wbits(p)
    return sorted({(b, l) for b, l in ((1, 1), (2, 3), (5, 3), (8, 3), (16, 4), (31, 2), (W // 4, 4), (W // 2, 2), (W, 1)) if b and b * l <= W})


@pytest.mark.parametrize("p", [PM64, P32, P50])
def test_matrix_form_equals_the_headers_formula_and_the_phase_identity(p):
    """n = 16, k = 1 and 2, m = 5, n and 1: the matrix form gives the words of the header's formula written naively, and with a
    noise-free key the phase of the output under the output key is, per coefficient t, body_t - sum_i s_in[i] r_{t,i} 2^s mod p --
    zero past m."""
    W, n, lin = wbits(p), 16, 5
    rng = random.Random("packmodel/%d" % p)
    for beta, ell in settings(p):
        s = W - beta * ell
        edge = edge_words(p, beta, ell)
        for k, m in ((1, 5), (2, n), (1, 1)):
            s_in = [rng.randrange(2) for _ in range(lin)]
            S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
            key = noise_free_key(rng, p, s_in, S, k, n, beta, ell)
            lwe = []
            for t in range(m):
                lwe += [edge[(t + i) % len(edge)] if (i + t) % 2 else rng.randrange(p) for i in range(lin)] + [rng.randrange(p)]
            out = model_pack_literal(lwe, key, p, lin, m, k, n, beta, ell)
            assert all(0 <= v < p for v in out)
            assert model_pack_batch(lwe, key, p, lin, m, k, n, beta, ell, 1) == out, (p, beta, ell, k, m)
            phase = out[k * n:]
            for q in range(k):
                phase = [(x - y) % p for x, y in zip(phase, negacyclic(out[q * n:(q + 1) * n], S[q], n))]
            want = []
            for t in range(m):
                r2s = [sum(d << (W - beta * (l + 1)) for l, d in enumerate(signed_digits(x, p, beta, ell))) for x in lwe[t * (lin + 1):][:lin]]
                assert all(r % (1 << s) == 0 and abs(r - lift(x, p)) <= ((1 << s) >> 1) for r, x in zip(r2s, lwe[t * (lin + 1):]))
                want.append((lwe[t * (lin + 1) + lin] - sum(si * r for si, r in zip(s_in, r2s))) % p)
            assert phase == want + [0] * (n - m), (p, beta, ell, k, m)


def test_matrix_form_batches_and_takes_lin_zero():
    p, n, k, m = P62, 16, 1, 3
    rng = random.Random("packmodel/batch")
    lwe = [rng.randrange(p) for _ in range(2 * m * 3)]
    key = [rng.randrange(p) for _ in range(2 * 2 * (k + 1) * n)]
    both = model_pack_batch(lwe, key, p, 2, m, k, n, 4, 2, 2)
    assert both == model_pack_literal(lwe[:m * 3], key, p, 2, m, k, n, 4, 2) + model_pack_literal(lwe[m * 3:], key, p, 2, m, k, n, 4, 2)
    body = [rng.randrange(p) for _ in range(m)]
    assert model_pack_batch(body, [], p, 0, m, k, n, 4, 2, 1) == [0] * n + body + [0] * (n - m)


@pytest.mark.parametrize("p", [PM64, PG64, P63, P62, P50, P32, P31, P30])
def test_the_kernels_negated_digits_are_minus_the_digits_mod_p(p):
    """prime_pack_decompose_kernel restated (y, the two shifts, the two selects) against -digits(x) mod p on the word width the plan
    uses: 0, 1, (p-1)/2, (p+1)/2, p-1, p-off, p-off-1, the words whose rounding lands on the ends of the top digit, and random ones;
    base_log = W with one level (sh1 = 0) and base_log * levels = W included.  Where the balanced lift reaches that far -- W = the
    word width -- the top digit takes both +B/2 and -B/2."""
    W = wbits(p)
    tb = 64 if W > 32 else 32
    rng = random.Random("packdigits/%d" % p)
    pairs = settings(p) + [(b, l) for b in (1, 3, 4, 7, 8, 11, 21, 31, 32) for l in (1, 2, 3, 4, 6, 8) if b * l <= W]
    pairs += [(b, W // b) for b in range(1, W + 1) if W % b == 0]             # base_log * levels = W
    assert (W, 1) in pairs
    tops = set()
    for beta, ell in sorted(set(pairs)):
        B, off = 1 << beta, gadget_offset(p, beta, ell)
        words = {0, 1, (p - 1) // 2, (p + 1) // 2, p - 1, (p - off) % p, (p - off - 1) % p} | set(edge_words(p, beta, ell))
        words |= {rng.randrange(p) for _ in range(60)}
        for x in sorted(words):
            d = signed_digits(x, p, beta, ell)
            tops.add((d[0] == B // 2, d[0] == -(B // 2)))
            assert kernel_negated_digits(x, p, beta, ell, tb) == [(-v) % p for v in d], (p, beta, ell, tb, hex(x))
            if tb == 32:                                                       # the same rule on the wider word
                assert kernel_negated_digits(x, p, beta, ell, 64) == [(-v) % p for v in d], (p, beta, ell, 64, hex(x))
    if W == tb:
        assert (True, False) in tops and (False, True) in tops


# -- the surface --------------------------------------------------------------------------------------------------------------------
def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_declares_the_four():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(NEW) == 4 and set(declarations(HEADER)) == NEW and len(declarations(HEADER)) == 4
    text = open(HEADER).read()
    assert re.search(r'^#include "cntt_prime_keyswitch.h"$', text, flags=re.M)
    flat = re.sub(r"[\s*]+", " ", text)
    assert "C = max(1, CNTT_PRIME_PACK_TERMS / levels)" in flat and "up(batch C levels n sizeof(T))" in flat
    assert "strict range" in text and "no same-machine A/B" in text and "normalize_batch" in text and "t >= m" in text
    assert PACK_TERMS in (32, 64, 128)


def test_library_exports_the_four_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    for name, count in SURFACE.items():
        path = os.path.join(INC, name)
        decl = declarations(path)
        assert len(decl) == count, (name, len(decl))
        assert not (NEW & set(decl)) and "cntt_prime_pack.h" not in open(path).read(), name


def test_cpp_mirror_forwards_the_arguments(tmp_path):
    """include/cntt.hpp: the two calls as members of cntt::prime32::Plan / prime64::Plan.  The program defines the four C entry points
    itself (they take precedence over the library's), so what it prints is what the methods passed on."""
    src, exe = tmp_path / "mirror.cpp", tmp_path / "mirror"
    src.write_text("""#include <cstdio>
#include "cntt.hpp"
#define STUB(BITS, T, PLAN)                                                                                                     \\
    extern "C" int cntt_prime##BITS##_pack_keyswitch_batch(const PLAN *, T *o, const T *i, const T *k, size_t lin, size_t m,   \\
                                                           size_t gd, unsigned bl, unsigned lv, size_t batch, void *ws,        \\
                                                           size_t wsb, cntt_mem_t where, void *st) {                           \\
        std::printf("%d %d %d %d %zu %zu %zu %u %u %zu %d %zu %d %d\\n", BITS, (int)*o, (int)*i, (int)*k, lin, m, gd, bl, lv, batch, \\
                    (int)*(char *)ws, wsb, (int)where, (int)*(char *)st);                                                      \\
        return 0;                                                                                                               \\
    }                                                                                                                           \\
    extern "C" size_t cntt_prime##BITS##_pack_workspace_bytes(const PLAN *, size_t lin, unsigned lv, size_t batch) {           \\
        return 1000000 * lin + 1000 * lv + batch + BITS;                                                                        \\
    }
STUB(64, uint64_t, cntt_plan64_t)
STUB(32, uint32_t, cntt_plan32_t)
template <class P, class T> void use(T p) {
    auto pl = P::try_new(32, p);
    T o = 1, i = 2, k = 3;
    char ws = 4, st = 5;
    pl->pack_keyswitch_batch(&o, &i, &k, 6, 7, 8, 9, 10, 11, &ws, 12, CNTT_MEM_HOST, &st);
    std::printf("%zu\\n", pl->pack_workspace_bytes(13, 14, 15));
}
int main() {
    use<cntt::prime64::Plan, uint64_t>(4611686018427322369ull);
    use<cntt::prime32::Plan, uint32_t>(1062862849u);
}
""")
    lib = os.path.join(ROOT, "concrete-ntt_amd")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INC, str(src), "-o", str(exe), "-L", lib,
                        "-lcntt_hip", "-Wl,-rpath," + lib], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    assert out[:4] == ["64 1 2 3 6 7 8 9 10 11 4 12 %d 5" % cntt._lib.MEM_HOST, "13014079", "32 1 2 3 6 7 8 9 10 11 4 12 %d 5" % cntt._lib.MEM_HOST,
                       "13014047"], out


def test_pack_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_keyswitch_abi.py reads its unit: the decomposing transpose
    and the body kernel on u32 and u64 words, four kernels, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_pack.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "pack.fat"), str(tmp_path / "pack.co")
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
    assert len(seen) == 4, seen
    for kernel in ("prime_pack_decompose_kernel", "prime_pack_body_kernel"):
        assert sum(kernel + "IjE" in s for s in seen) == 1 and sum(kernel + "ImE" in s for s in seen) == 1, seen


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_is_the_formula_of_the_header(mod, p, wb):
    assert C(1) == PACK_TERMS and C(3) == PACK_TERMS // 3 and C(PACK_TERMS + 1) == 1
    for n, lin, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 7, 3, 5), (256, 630, 4, 37), (2048, 2048, 2, 1000), (1024, 500, 64, 2),
                                  (4096, 40, 3, 2), (64, 100, 7, 3)):
        plan = mod.Plan.try_new(n, p)
        if levels > wbits(p):
            continue
        assert plan.pack_workspace_bytes(lin, levels, batch) == workspace_bytes(n, wb, lin, levels, batch), (n, lin, levels, batch)
    plan = mod.Plan.try_new(32, p)
    fn = getattr(cntt.lib(), "cntt_prime%d_pack_workspace_bytes" % (8 * wb))
    assert fn(None, 5, 2, 3) == 0 and fn(plan._h, 5, 0, 3) == 0 and fn(plan._h, 5, 2, 3) == workspace_bytes(32, wb, 5, 2, 3)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B = 32, 1, 2
LIN, M_, LEVELS = 6, 5, 3
POISON = 7


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments at n = 32: 2 x 5 ciphertexts of dimension 6 into 2 GLWE ciphertexts with k = 1, levels = 3; the output
    filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.lwe_in = np.arange(B * M_ * (LIN + 1), dtype=self.dtype)
        self.out = np.full(B * (K + 1) * N, POISON, dtype=self.dtype)
        self.key = np.zeros(LIN * LEVELS * (K + 1) * N, dtype=self.dtype)
        self.ws = np.zeros(self.plan.pack_workspace_bytes(LIN, LEVELS, B), dtype=np.uint8)

    def call(self, plan="own", out="own", lwe_in="own", key="own", lin=LIN, m=M_, k=K, base_log=4, levels=LEVELS, batch=B, ws=None,
             ws_bytes=None):
        out = self.out if isinstance(out, str) else out
        lwe_in = self.lwe_in if isinstance(lwe_in, str) else lwe_in
        key = self.key if isinstance(key, str) else key
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        fn = getattr(cntt.lib(), "cntt_prime%d_pack_keyswitch_batch" % self.bits)
        return fn(self.plan._h if plan == "own" else None, ptr(out), ptr(lwe_in), ptr(key), lin, m, k, base_log, levels, batch, ptr(ws), wsb, 0,
                  None)

    def untouched(self):
        return bool((self.out == POISON).all())


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_every_invalid_argument_is_refused(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(8192, POISON, dtype=c.dtype)
    out_in_big = big[:B * (K + 1) * N]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    cases = [
        (dict(plan=None), "plan"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=1, levels=W + 1), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the bit length"),
        (dict(m=0), "lwe_count"),
        (dict(m=N + 1, lwe_in=np.zeros(B * (N + 1) * (LIN + 1), dtype=c.dtype)), "lwe_count"),
        (dict(out=None), "glwe_out"),
        (dict(lwe_in=None), "lwe_in"),
        (dict(key=None), "pksk_ntt"),
        (dict(out=out_in_big, lwe_in=big[8:8 + c.lwe_in.size]), "glwe_out overlaps lwe_in"),
        (dict(out=out_in_big, key=big[8:8 + c.key.size]), "glwe_out overlaps pksk_ntt"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(lwe_in=big[:c.lwe_in.size], ws=ws_in_big), "lwe_in overlaps workspace"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
        # batch * max(C * levels, k + 1) >= 2^32: C * levels = 6 * 3 here (C capped at Lin), and k + 1 with Lin = 0
        (dict(batch=(1 << 32) // (LIN * LEVELS) + 1), "2^32"),
        (dict(batch=1 << 31, lin=0, key=None), "2^32"),
        # sizes whose byte counts would wrap a size_t: refused before any of them is formed
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
        (dict(lin=1 << 32, levels=1), "2^32 key rows"),
        (dict(lin=(1 << 32) - 2, levels=1, batch=1 << 28), "2^63 bytes"),
        (dict(lin=(1 << 31) - 1, levels=2, base_log=1, k=(1 << 32) - 2, batch=1), "2^63 bytes"),
    ]
    for kw, word in cases:
        assert c.call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_lin_zero_needs_no_key(bits, p):
    c = Case(bits, p)
    fn = getattr(cntt.lib(), "cntt_prime%d_pack_keyswitch_batch" % bits)
    assert fn(c.plan._h, None, None, None, LIN, M_, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.call(batch=0) == 0 and c.untouched()
    # Lin = 0 with a NULL key passes the argument checks (what follows needs a device: any other status than CNTT_EINVAL)
    assert c.call(lin=0, key=None, lwe_in=np.arange(B * M_, dtype=c.dtype)) != EINVAL


def test_base_log_above_31_is_valid_here():
    """full-word digits, not the LWE keyswitch's 32-bit ones: base_log = 32, levels = 2 and base_log = 64, levels = 1 pass the argument
    checks on PM64"""
    c = Case(64, PM64)
    assert c.call(base_log=32, levels=2, key=np.zeros(LIN * 2 * (K + 1) * N, dtype=np.uint64)) != EINVAL
    assert c.call(base_log=64, levels=1, key=np.zeros(LIN * (K + 1) * N, dtype=np.uint64)) != EINVAL


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    bad = [
        (c.out[:-1], c.lwe_in, c.key, LIN, M_, K, 4, LEVELS),                  # glwe_out too short
        (c.out, c.lwe_in, c.key, LIN + 1, M_, K, 4, LEVELS),                   # not whole ciphertexts
        (c.out, c.lwe_in, c.key, LIN, M_ + 1, K, 4, LEVELS),                   # not whole groups of lwe_count
        (c.out, c.lwe_in, c.key, LIN, 0, K, 4, LEVELS),
        (c.out, c.lwe_in, c.key, LIN, M_, K + 1, 4, LEVELS),                   # out sized for k = 1
        (c.out, c.lwe_in, c.key[:-N], LIN, M_, K, 4, LEVELS),                  # a key polynomial missing
        (c.out, c.lwe_in, c.key, LIN, M_, K, 4, LEVELS + 1),                   # key sized for levels = 3
        (c.out, c.lwe_in, c.key, LIN, M_, K, 0, LEVELS),
        (c.out, c.lwe_in, c.key.astype(np.uint16), LIN, M_, K, 4, LEVELS),
        (c.out, c.lwe_in, c.key, LIN, M_, K, wbits(p) // 3 + 1, LEVELS),       # through the C checks
    ]
    for args in bad:
        with pytest.raises((Panic, TypeError)):
            pl.pack_keyswitch_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.pack_keyswitch_batch(c.out, c.lwe_in, c.key, LIN, M_, K, 4, LEVELS, workspace=c.ws[:-256])
    with pytest.raises(Panic):
        pl.pack_workspace_bytes(LIN, LEVELS, -1)
    with pytest.raises(Panic):
        pl.pack_workspace_bytes(LIN, 0, 1)
    assert c.untouched()
