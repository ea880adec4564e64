"""C ABI of the prime plans' ring automorphism, Galois keyswitch and trace (include/cntt_prime_automorphism.h): the header is plain C11 on
its own and includes cntt_prime_pbs.h itself, its names are the six per word width plus the grid function, none of them leaked into the
existing headers, all are exported, every CNTT_EINVAL case is refused on host buffers by the argument checks that precede any device
call (output poison intact, argument named), the workspace sizes are the header's formulas, the grid rule is what the header says, the
Python wrappers panic on bad shapes, and the code object of the new unit has its kernels without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from prime_automorphism_model import HEADER, autoks_workspace_bytes, trace_workspace_bytes
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CALLS = ["automorphism_batch", "automorphism_ntt_batch", "glwe_automorphism_keyswitch_batch", "glwe_automorphism_keyswitch_workspace_bytes",
         "glwe_trace_batch", "glwe_trace_workspace_bytes"]
GRID = "cntt_prime_automorphism_grid"
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS} | {GRID}
SURFACE = {"cntt.h": 87, "cntt_ext.h": 2, "cntt_pbs.h": 5, "cntt_keyswitch.h": 3, "cntt_pack.h": 2, "cntt_prime_pbs.h": 12,
           "cntt_prime_keyswitch.h": 6, "cntt_prime_pack.h": 4}


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert len(NEW) == 13 and set(decl) == NEW and len(decl) == 13
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_prime_pbs.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "out[j] = in[u mod n], negated mod p (0 stays 0) iff u >= n" in flat
    assert "2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n" in flat
    assert "up(batch k levels n sizeof(T))" in flat and "up(batch (k + 1) n sizeof(T))" in flat
    assert "strict range" in text and "normalize_batch" in text and "t_r = n / 2^r + 1" in text and "inverse of 2^steps mod p" in text


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    for name, count in SURFACE.items():
        path = os.path.join(INC, name)
        decl = declarations(path)
        assert len(decl) == count, (name, len(decl))
        assert not (NEW & set(decl)) and "cntt_prime_automorphism.h" not in re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S), name


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_pack_abi.py reads its unit: three kernels x two word types x
    streaming or not x staged or not, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_automorphism.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "autom.fat"), str(tmp_path / "autom.co")
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
    assert len(seen) == 24, seen
    for kernel in ("prime_automorphism_kernel", "prime_automorphism_ntt_kernel", "prime_automorphism_gadget_kernel"):
        for word in ("IjLb", "ImLb"):
            assert sum(("4cntt%d%s%s" % (len(kernel), kernel, word)) in s for s in seen) == 4, (kernel, word, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_are_the_formulas_of_the_header(mod, p, wb):
    for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
        plan = mod.Plan.try_new(n, p)
        assert plan.glwe_automorphism_keyswitch_workspace_bytes(k, levels, batch) == autoks_workspace_bytes(n, wb, k, levels, batch)
        assert plan.glwe_trace_workspace_bytes(k, levels, batch) == trace_workspace_bytes(n, wb, k, levels, batch)
    for name in ("glwe_automorphism_keyswitch_workspace_bytes", "glwe_trace_workspace_bytes"):
        assert getattr(cntt.lib(), "cntt_prime%d_%s" % (8 * wb, name))(None, 1, 2, 3) == 0


def test_grid_rule():
    """one workgroup per polynomial up to 8 per CU of a 256-CU part, fewer where the staged polynomial limits what a CU holds"""
    g = cntt.lib().cntt_prime_automorphism_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    assert g(5000, 5, 4) == 2048                       # small polynomials: the wave cap
    assert g(5000, 12, 8) == 5 * 256                   # 32 KiB staged: five per CU
    assert g(5000, 13, 8) == 2 * 256                   # 64 KiB staged: two per CU
    assert g(5000, 14, 8) == 2048                      # past the LDS limit: the global gather, the wave cap again


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, STEPS = 32, 1, 2, 3, 2
POISON = 7


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments at n = 32: 2 GLWE ciphertexts with k = 1, levels = 3, keys for two trace steps; the output filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.inp = np.arange(B * (K + 1) * N, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * N, POISON, dtype=self.dtype)
        self.key = np.zeros(STEPS * K * LEVELS * (K + 1) * N, dtype=self.dtype)
        self.ws = np.zeros(self.plan.glwe_trace_workspace_bytes(K, LEVELS, B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def pick(self, out, inp, key):
        return (self.out if isinstance(out, str) else out, self.inp if isinstance(inp, str) else inp, self.key if isinstance(key, str) else key)

    def perm(self, ntt=False, plan="own", out="own", inp="own", t=3, npolys=K + 1, batch=B):
        out, inp, _ = self.pick(out, inp, None)
        return self.fn("automorphism_ntt_batch" if ntt else "automorphism_batch")(self.plan._h if plan == "own" else None, ptr(out), ptr(inp), t,
                                                                                  npolys, batch, 0, None)

    def ks(self, plan="own", out="own", inp="own", key="own", t=3, k=K, base_log=4, levels=LEVELS, add=0, batch=B, ws=None, ws_bytes=None):
        out, inp, key = self.pick(out, inp, key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("glwe_automorphism_keyswitch_batch")(self.plan._h if plan == "own" else None, ptr(out), ptr(inp), ptr(key), t, k, base_log,
                                                            levels, add, batch, ptr(ws), wsb, 0, None)

    def trace(self, plan="own", out="own", inp="own", key="own", steps=STEPS, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        out, inp, key = self.pick(out, inp, key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("glwe_trace_batch")(self.plan._h if plan == "own" else None, ptr(out), ptr(inp), ptr(key), steps, k, base_log, levels, batch,
                                           ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all())


class Raw:
    """an array-like whose address is `addr`: what ptr() reads"""

    def __init__(self, addr):
        self.ctypes = type("C", (), {"data": addr})()


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_every_invalid_argument_is_refused(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(8192, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    skew = Raw(c.inp.ctypes.data + 1)                                          # one byte off the word's alignment
    for ntt in (False, True):
        o, i = ("out_ntt", "in_ntt") if ntt else ("out", "in")
        cases = [(dict(plan=None), "plan"), (dict(t=0), "t = 0"), (dict(t=4), "t = 4"), (dict(t=2 * N), "t = %d" % (2 * N)),
                 (dict(t=2 * N + 1), "odd exponent below 2n"), (dict(out=None), o + " is NULL"), (dict(inp=None), i + " is NULL"),
                 (dict(out=out_in_big, inp=big[8:8 + c.inp.size]), "%s overlaps %s" % (o, i)), (dict(inp=skew), i + " is not"),
                 (dict(out=Raw(c.out.ctypes.data + 1)), o + " is not"), (dict(batch=1 << 40, npolys=1 << 20), "2^63 bytes")]
        for kw, word in cases:
            assert c.perm(ntt=ntt, **kw) == EINVAL, (ntt, kw)
            assert word in err(), (kw, err())
            assert c.untouched() and (big == POISON).all(), kw
    shared = [
        (dict(plan=None), "plan"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the bit length"),
        (dict(out=None), "glwe_out is NULL"),
        (dict(inp=None), "glwe_in is NULL"),
        (dict(key=None), "ak_ntt is NULL"),
        (dict(out=out_in_big, inp=big[8:8 + c.inp.size]), "glwe_out overlaps glwe_in"),
        (dict(out=out_in_big, key=big[8:8 + c.key.size]), "glwe_out overlaps ak_ntt"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(inp=big[:c.inp.size], ws=ws_in_big), "workspace overlaps glwe_in"),
        (dict(key=big[:c.key.size], ws=ws_in_big), "workspace overlaps ak_ntt"),
        (dict(inp=skew), "glwe_in is not"),
        (dict(key=Raw(c.key.ctypes.data + w // 2)), "ak_ntt is not"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        # batch * max(k * levels, k + 1) >= 2^32: k * levels = 3 here, and k + 1 with k = 0
        (dict(batch=(1 << 32) // LEVELS + 1), "2^32"),
        (dict(batch=1 << 32, k=0, key=None), "2^32"),
        # sizes whose byte counts would wrap a size_t: refused before any of them is formed
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
        (dict(k=1 << 31, levels=1, batch=1), "2^63 bytes"),
    ]
    ks_small = c.plan.glwe_automorphism_keyswitch_workspace_bytes(K, LEVELS, B)
    for kw, word in shared + [(dict(t=0), "t = 0"), (dict(t=6), "t = 6"), (dict(t=2 * N), "below 2n"),
                              (dict(ws=c.ws, ws_bytes=ks_small - 1), "workspace_bytes")]:
        assert c.ks(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw
    for kw, word in shared + [(dict(steps=6), "steps = 6"), (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
                              (dict(ws=c.ws, ws_bytes=ks_small), "workspace_bytes")]:
        assert c.trace(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_keyless_calls_need_no_key(bits, p):
    c = Case(bits, p)
    assert c.fn("automorphism_batch")(c.plan._h, None, None, 3, 2, 0, 0, None) == 0
    assert c.fn("automorphism_ntt_batch")(c.plan._h, None, None, 3, 0, 5, 0, None) == 0
    assert c.fn("glwe_automorphism_keyswitch_batch")(c.plan._h, None, None, None, 3, K, 8, 3, 0, 0, None, 0, 0, None) == 0
    assert c.fn("glwe_trace_batch")(c.plan._h, None, None, None, 2, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.ks(batch=0) == 0 and c.trace(batch=0) == 0 and c.perm(batch=0) == 0 and c.untouched()
    # k = 0, or a trace of no steps, with a NULL key passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    body = np.arange(B * N, dtype=c.dtype)
    out = np.zeros(B * N, dtype=c.dtype)
    assert c.ks(k=0, key=None, inp=body, out=out) != EINVAL
    assert c.trace(k=0, key=None, inp=body, out=out) != EINVAL
    assert c.trace(steps=0, key=None) != EINVAL


def test_full_word_digits_are_valid():
    """base_log = 32, levels = 2 and base_log = 64, levels = 1 pass the argument checks on PM64"""
    c = Case(64, PM64)
    assert c.ks(base_log=32, levels=2, key=np.zeros(2 * (K + 1) * N, dtype=np.uint64)) != EINVAL
    assert c.ks(base_log=64, levels=1, key=np.zeros((K + 1) * N, dtype=np.uint64)) != EINVAL


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    one_key = c.key[:c.key.size // STEPS]
    for args in [(c.out[:-1], c.inp, 3), (c.out[:-N], c.inp, 3), (c.out, c.inp, 4), (c.out, c.inp, 2 * N + 1), (c.out, c.inp.astype(np.uint16), 3)]:
        for fn in (pl.automorphism_batch, pl.automorphism_ntt_batch):
            with pytest.raises((Panic, TypeError)):
                fn(*args)
    bad = [
        (c.out[:-N], c.inp, one_key, 3, K, 4, LEVELS),                         # glwe_out too short
        (c.out, c.inp, one_key, 3, K + 2, 4, LEVELS),                          # not whole ciphertexts
        (c.out, c.inp, one_key[:-N], 3, K, 4, LEVELS),                         # a key polynomial missing
        (c.out, c.inp, one_key, 3, K, 4, LEVELS + 1),                          # key sized for levels = 3
        (c.out, c.inp, one_key, 3, K, 0, LEVELS),
        (c.out, c.inp, one_key, 2, K, 4, LEVELS),                              # through the C checks: t even
        (c.out, c.inp, one_key, 3, K, wbits(p) // 3 + 1, LEVELS),              # through the C checks
    ]
    for args in bad:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_automorphism_keyswitch_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.glwe_automorphism_keyswitch_batch(c.out, c.inp, one_key, 3, K, 4, LEVELS, workspace=c.ws[:255])
    for args in [(c.out, c.inp, one_key, STEPS, K, 4, LEVELS), (c.out, c.inp, c.key, -1, K, 4, LEVELS), (c.out, c.inp, c.key, 6, K, 4, LEVELS)]:
        with pytest.raises(Panic):
            pl.glwe_trace_batch(*args)
    for fn in (pl.glwe_automorphism_keyswitch_workspace_bytes, pl.glwe_trace_workspace_bytes):
        with pytest.raises(Panic):
            fn(K, LEVELS, -1)
        with pytest.raises(Panic):
            fn(K, 0, 1)
    assert c.untouched()
