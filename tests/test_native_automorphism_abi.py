"""C ABI of the native plans' automorphism, Galois keyswitch and trace (include/cntt_automorphism.h), after tests/test_native_cmux_abi.py:
the header is plain C11 on its own and includes cntt_ext.h only, its names are the seven it declares, none of them reaches another
header, all are exported, every CNTT_EINVAL case is refused on host buffers by the argument checks that precede any device call (output
poison intact, argument named; the kind refusals and k * levels = max_terms + 1 included), the workspace sizes are the header's formulas,
the grid rule is what the header says, the Python wrappers panic on bad shapes, and the code object of the new unit has its 32 kernels
without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary32, native_binary64
from concrete_ntt_amd._lib import EINVAL, Panic
from native_automorphism_model import HEADER, autoks_workspace_bytes, grid, trace_workspace_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW = {"cntt_native_automorphism_batch", "cntt_native_automorphism_ntt_batch", "cntt_native_glwe_automorphism_keyswitch_batch",
       "cntt_native_glwe_automorphism_keyswitch_workspace_bytes", "cntt_native_glwe_trace_batch", "cntt_native_glwe_trace_workspace_bytes",
       "cntt_native_automorphism_grid"}


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def err():
    return cntt.lib().cntt_last_error().decode()


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert set(decl) == NEW and len(decl) == 7
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_ext.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "nterms = k levels, nout = k + 1, accumulate = 1" in flat and "CNTT_SRC_PLAIN, npolys = k" in flat
    assert "2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n" in flat and "AK[j][q] at index j (k + 1) + q" in flat
    assert "key r sits at residue polynomial r k levels (k + 1) of every plane" in flat
    assert "2^steps is NOT a unit mod 2^w" in flat and "headroom BELOW the message" in flat
    assert "k levels > cntt_native_max_terms(plan)" in flat and "a binary kind (calls 3 and 4)" in flat
    assert "profiles/r27_native_automorphism.txt" in flat
    for name in sorted(os.listdir(INC)):
        if name == "cntt_automorphism.h" or not name.endswith(".h"):
            continue
        raw = open(os.path.join(INC, name)).read()
        assert "cntt_automorphism.h" not in raw and not (NEW & set(declarations(os.path.join(INC, name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_native_cmux_abi.py reads its unit: the signed gather and the
    gather with digits on three word types, the slot permutation on two residue types, each streaming or not and staged or not -- 32
    kernels, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_automorphism.o")
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
    assert len(seen) == 32, seen
    for kernel, words in (("26native_automorphism_kernel", ("Ij", "Im", "INS_7Word128E")), ("30native_automorphism_ntt_kernel", ("Ij", "Im")),
                          ("33native_automorphism_gadget_kernel", ("Ij", "Im", "INS_7Word128E"))):
        for word in words:
            for stream in "01":
                for lds in "01":
                    tag = "4cntt%s%sLb%sELb%sE" % (kernel, word, stream, lds)
                    assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("mod", [native32, native64, native128, native_binary64])
def test_workspace_bytes_are_the_formulas_of_the_header(mod):
    for P in (mod.Plan32, getattr(mod, "Plan52", None)):
        if P is None:
            continue
        for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
            plan = P.try_new(n)
            wb = plan.WORD
            assert plan.glwe_automorphism_keyswitch_workspace_bytes(k, levels, batch) == autoks_workspace_bytes(n, wb, k, levels, batch)
            assert plan.glwe_trace_workspace_bytes(k, levels, batch) == trace_workspace_bytes(n, wb, k, levels, batch)
    wb = mod.Plan32.WORD
    assert mod.Plan32.try_new(32).glwe_trace_workspace_bytes(1, 3, 8) == 8 * 3 * 32 * wb + 8 * 2 * 32 * wb
    L = cntt.lib()
    assert L.cntt_native_glwe_automorphism_keyswitch_workspace_bytes(None, 1, 2, 3) == 0 and L.cntt_native_glwe_trace_workspace_bytes(None, 1, 2, 3) == 0


def test_grid_rule():
    g = cntt.lib().cntt_native_automorphism_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(5000, 10, 8) == 2048
    assert g(5000, 12, 16) == 512 and g(5000, 13, 16) == 2048                   # 64 KiB is staged, two per CU; 128 KiB is not
    for polys in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 11, 12, 13, 14, 15):
            for w in (4, 8, 16):
                assert g(polys, logn, w) == grid(polys, logn, w), (polys, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, STEPS = 32, 1, 2, 3, 2
POISON = 7
KEY = K * LEVELS * (K + 1) * N


class Raw:
    """a bare address standing for a buffer"""

    def __init__(self, address):
        self.address = address


def ptr(a):
    if a is None:
        return None
    return ctypes.c_void_p(a.address if isinstance(a, Raw) else a.ctypes.data)


class Case:
    """Valid host arguments at n = 32: k = 1, levels = 3, 2 GLWE ciphertexts, two automorphism keys as residue planes; the outputs
    filled with 7."""

    def __init__(self, P):
        self.plan = P.try_new(N)
        self.dtype, self.pe = self.plan.word_dtype, N * (2 if self.plan.WORD == 16 else 1)
        self.inp = np.arange(B * (K + 1) * self.pe, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * self.pe, POISON, dtype=self.dtype)
        self.key = [np.zeros(STEPS * KEY, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.pin = [np.arange(B * N, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.pout = [np.full(B * N, POISON, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.ws = np.zeros(self.plan.glwe_trace_workspace_bytes(K, LEVELS, B), dtype=np.uint8)

    def planes(self, sel):
        if sel is None:
            return None
        return (ctypes.c_void_p * self.plan.NPRIMES)(*[None if p is None else ptr(p) for p in sel])

    def pick(self, **kw):
        return {k: (getattr(self, k) if isinstance(v, str) else v) for k, v in kw.items()}

    def autom(self, plan="own", out="own", inp="own", t=3, npolys=K + 1, batch=B):
        a = self.pick(out=out, inp=inp)
        return cntt.lib().cntt_native_automorphism_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["inp"]), t, npolys, batch, 0, None)

    def ntt(self, plan="own", pout="own", pin="own", t=3, npolys=1, batch=B):
        a = self.pick(pout=pout, pin=pin)
        return cntt.lib().cntt_native_automorphism_ntt_batch(self.plan._h if plan == "own" else None, self.planes(a["pout"]), self.planes(a["pin"]), t,
                                                             npolys, batch, 0, None)

    def autoks(self, plan="own", out="own", inp="own", key="own", t=3, k=K, base_log=4, levels=LEVELS, add=0, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, inp=inp, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_glwe_automorphism_keyswitch_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["inp"]),
                                                                        self.planes(a["key"]), t, k, base_log, levels, add, batch, ptr(ws), wsb, 0, None)

    def trace(self, plan="own", out="own", inp="own", key="own", steps=STEPS, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, inp=inp, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_glwe_trace_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["inp"]), self.planes(a["key"]),
                                                       steps, k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all()) and all(bool((p == POISON).all()) for p in self.pout)


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_every_invalid_argument_is_refused(P):
    c = Case(P)
    W, w, rb = 8 * c.plan.WORD, c.plan.WORD, c.plan.RES
    big = np.full(16384, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    plane_in_big = big.view(c.plan.res_dtype)[8 * w // rb:8 * w // rb + c.key[0].size]     # starts 8 words into `big`
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    ks_ws = c.plan.glwe_automorphism_keyswitch_workspace_bytes(K, LEVELS, B)
    tr_ws = c.plan.glwe_trace_workspace_bytes(K, LEVELS, B)
    last = c.plan.NPRIMES - 1

    def refused(call, kw, word):
        assert call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw

    def with_plane(planes, i, p):
        return planes[:i] + [p] + planes[i + 1:]

    # calls 1 and 2
    for kw, word in [(dict(plan=None), "plan is NULL"), (dict(t=0), "t = 0"), (dict(t=4), "t = 4"), (dict(t=2 * N), "t = 64"), (dict(t=2 * N + 1), "t = 65"),
                     (dict(out=None), "out is NULL"), (dict(inp=None), "in is NULL"), (dict(out=out_in_big, inp=big[8:8 + c.inp.size]), "out overlaps in"),
                     (dict(out=Raw(c.out.ctypes.data + w // 2)), "out is not"), (dict(inp=Raw(c.inp.ctypes.data + 1)), "in is not"),
                     (dict(batch=1 << 62, npolys=1 << 10), "2^63 bytes")]:
        refused(c.autom, kw, word)
    assert c.autom(out=c.inp) == EINVAL and "out overlaps in" in err()               # no call runs in place
    pbig = big.view(c.plan.res_dtype)
    for kw, word in [(dict(plan=None), "plan is NULL"), (dict(t=2), "t = 2"), (dict(t=2 * N + 3), "t = 67"),
                     (dict(pout=None), "out_planes is NULL"), (dict(pin=None), "in_planes is NULL"),
                     (dict(pout=with_plane(c.pout, last, None)), "NULL residue plane (out_planes[%d])" % last),
                     (dict(pin=with_plane(c.pin, 0, None)), "NULL residue plane (in_planes[0])"),
                     (dict(pout=with_plane(c.pout, 0, pbig[:B * N]), pin=with_plane(c.pin, last, pbig[8:8 + B * N])), "out_planes[0] overlaps in_planes[%d]" % last),
                     (dict(pout=with_plane(c.pout, 0, Raw(c.pout[0].ctypes.data + rb // 2))), "out_planes[0] is not"),
                     (dict(pin=with_plane(c.pin, last, Raw(c.pin[last].ctypes.data + 1))), "in_planes[%d] is not" % last),
                     (dict(batch=1 << 62, npolys=1 << 10), "2^63 bytes")]:
        refused(c.ntt, kw, word)
    if c.plan.NPRIMES > 1:
        refused(c.ntt, dict(pout=with_plane(with_plane(c.pout, 0, pbig[:B * N]), 1, pbig[8:8 + B * N])), "out_planes[0] overlaps out_planes[1]")
    assert c.ntt(pout=c.pin) == EINVAL and "overlaps" in err()
    # calls 3 and 4
    shared = [
        (dict(plan=None), "plan is NULL"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the word width %d" % W),
        (dict(out=None), "glwe_out is NULL"),
        (dict(inp=None), "glwe_in is NULL"),
        (dict(key=None), "ak_ntt is NULL"),
        (dict(key=with_plane(c.key, last, None)), "NULL key residue plane (ak_ntt[%d])" % last),
        (dict(out=out_in_big, inp=big[8:8 + c.inp.size]), "glwe_out overlaps glwe_in"),
        (dict(out=out_in_big, key=with_plane(c.key, 0, plane_in_big)), "glwe_out overlaps ak_ntt[0]"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(inp=big[:c.inp.size], ws=ws_in_big), "workspace overlaps glwe_in"),
        (dict(key=with_plane(c.key, last, plane_in_big), ws=ws_in_big), "workspace overlaps ak_ntt[%d]" % last),
        (dict(key=with_plane(c.key, 1 % c.plan.NPRIMES, Raw(c.key[0].ctypes.data + rb // 2))), "ak_ntt[%d] is not" % (1 % c.plan.NPRIMES)),
        (dict(out=Raw(c.out.ctypes.data + w // 2)), "glwe_out is not"),
        (dict(inp=Raw(c.inp.ctypes.data + 1)), "glwe_in is not"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "workspace is not 16-byte aligned"),
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
        # batch * max(k * levels, k + 1) >= 2^32
        (dict(batch=(1 << 32) // (K * LEVELS) + 1), "2^32"), (dict(batch=1 << 32, k=0, levels=1), "2^32"), (dict(batch=1 << 63), "2^32"),
    ]
    for kw, word in shared + [(dict(t=0), "t = 0"), (dict(t=6), "t = 6"), (dict(t=2 * N), "t = 64"), (dict(t=(1 << 64) - 1), "t = "),
                              (dict(ws=c.ws, ws_bytes=ks_ws - 1), "workspace_bytes")]:
        refused(c.autoks, kw, word)
    assert c.autoks(out=c.inp) == EINVAL and "glwe_out overlaps glwe_in" in err()
    for kw, word in shared + [(dict(steps=6), "steps = 6 exceeds log2(ntt_size) = 5"), (dict(steps=(1 << 32) - 1), "steps"),
                              (dict(ws=c.ws, ws_bytes=tr_ws - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=ks_ws), "workspace_bytes")]:
        refused(c.trace, kw, word)


@pytest.mark.parametrize("P", [native_binary64.Plan32, native_binary32.Plan52])
def test_binary_kinds_are_refused_by_calls_3_and_4_and_served_by_1_and_2(P):
    c = Case(P)
    assert c.autoks() == EINVAL and "native_binary kind" in err() and c.untouched()
    assert c.trace() == EINVAL and "native_binary kind" in err() and c.untouched()
    assert c.autom(t=4) == EINVAL and c.ntt(t=4) == EINVAL                       # ... past the kind, at the exponent
    assert c.autom() != EINVAL and c.ntt() != EINVAL                             # (what follows needs a device: any status but CNTT_EINVAL)


def test_max_terms_bound_counts_k_times_levels():
    """native64 Plan32 at n = 32768 holds 61 terms: k = 1, base_log = 1, levels = 62 fits the word (62 <= 64) and not the exact range;
    levels = 61 passes, and so does k = 0 with any levels, which sums nothing"""
    plan = native64.Plan32.try_new(32768)
    assert plan.max_terms() == 61
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * 5)(*[16] * 5)
    assert L.cntt_native_glwe_automorphism_keyswitch_batch(plan._h, p(16), p(16), dummy, 3, 1, 1, 62, 0, 1, None, 0, 0, None) == EINVAL
    assert "glwe_dim * levels = 62 exceeds cntt_native_max_terms() = 61" in err()
    assert L.cntt_native_glwe_trace_batch(plan._h, p(16), p(16), dummy, 2, 1, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "glwe_dim * levels = 62 exceeds cntt_native_max_terms() = 61" in err()
    assert L.cntt_native_glwe_automorphism_keyswitch_batch(plan._h, None, p(16), dummy, 3, 1, 1, 61, 0, 1, None, 0, 0, None) == EINVAL
    assert "glwe_out is NULL" in err()                                          # 61 terms got past the size checks
    assert L.cntt_native_glwe_automorphism_keyswitch_batch(plan._h, None, p(16), None, 3, 0, 1, 62, 0, 1, None, 0, 0, None) == EINVAL
    assert "glwe_out is NULL" in err()


def test_byte_counts_past_2_63_are_refused_before_they_are_formed():
    plan = native32.Plan52.try_new(16)
    assert plan.max_terms() > 1 << 30
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * plan.NPRIMES)(*[16] * plan.NPRIMES)
    assert L.cntt_native_glwe_automorphism_keyswitch_batch(plan._h, p(16), p(16), dummy, 3, (1 << 30) - 1, 1, 1, 0, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()
    assert L.cntt_native_glwe_trace_batch(plan._h, p(16), p(16), dummy, 4, (1 << 30) - 1, 1, 1, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32])
def test_empty_calls_do_nothing_and_k_zero_needs_no_key(P):
    c = Case(P)
    L = cntt.lib()
    assert L.cntt_native_automorphism_batch(c.plan._h, None, None, 3, 1, 0, 0, None) == 0
    assert L.cntt_native_automorphism_ntt_batch(c.plan._h, None, None, 3, 0, 1, 0, None) == 0
    assert L.cntt_native_glwe_automorphism_keyswitch_batch(c.plan._h, None, None, None, 3, K, 8, 3, 0, 0, None, 0, 0, None) == 0
    assert L.cntt_native_glwe_trace_batch(c.plan._h, None, None, None, STEPS, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.autoks(batch=0) == 0 and c.trace(batch=0) == 0 and c.autom(batch=0) == 0 and c.ntt(npolys=0) == 0 and c.untouched()
    # k = 0 with a NULL key, and the trace of no steps, pass the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    body, out = np.arange(B * N, dtype=c.dtype), np.zeros(B * N, dtype=c.dtype)
    assert c.autoks(k=0, key=None, inp=body, out=out) != EINVAL
    assert c.trace(k=0, key=None, inp=body, out=out) != EINVAL
    assert c.trace(steps=0, key=None, out=np.zeros_like(c.inp)) != EINVAL
    W = 8 * c.plan.WORD
    one = [np.zeros(K * 1 * (K + 1) * N, dtype=c.plan.res_dtype) for _ in range(c.plan.NPRIMES)]
    assert c.autoks(base_log=W, levels=1, key=one, out=np.zeros_like(c.inp)) != EINVAL          # full-word digits are valid


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32])
def test_python_wrappers_panic_on_bad_shapes(P):
    c = Case(P)
    pl, pe = c.plan, c.pe
    one = [p[:KEY] for p in c.key]
    for args in [(c.out[:-pe], c.inp, 3), (c.out, c.inp[:-2], 3), (c.out, c.inp, -1)]:
        with pytest.raises((Panic, TypeError)):
            pl.automorphism_batch(*args)
    for args in [(c.pout[:-1], c.pin, 3), (c.pout, c.pin[:-1], 3), (c.pout, [p[:-N] for p in c.pin], 3), ([p[:-2] for p in c.pout], c.pin, 3), (c.pout, c.pin, -1)]:
        with pytest.raises((Panic, TypeError)):
            pl.automorphism_ntt_batch(*args)
    for args in [(c.out[:-pe], c.inp, one, 3, K, 4, LEVELS), (c.out, c.inp[:-2], one, 3, K, 4, LEVELS), (c.out, c.inp, [p[:-N] for p in one], 3, K, 4, LEVELS),
                 (c.out, c.inp, one, 3, K, 4, LEVELS + 1), (c.out, c.inp, c.key, 3, K, 4, LEVELS), (c.out, c.inp, one[:-1], 3, K, 4, LEVELS),
                 (c.out, c.inp, None, 3, K, 4, LEVELS), (c.out, c.inp, one, 3, -1, 4, LEVELS), (c.out, c.inp, one, 3, K, 0, LEVELS),
                 (c.out, c.inp, one, 3, K, 4, 0), (c.out, c.inp, one, -3, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_automorphism_keyswitch_batch(*args)
    for args in [(c.out[:-pe], c.inp, c.key, STEPS, K, 4, LEVELS), (c.out, c.inp, one, STEPS, K, 4, LEVELS), (c.out, c.inp, c.key, STEPS + 1, K, 4, LEVELS),
                 (c.out, c.inp, None, STEPS, K, 4, LEVELS), (c.out, c.inp, c.key, -1, K, 4, LEVELS), (c.out, c.inp, c.key, STEPS, K, 0, LEVELS),
                 (c.out, c.inp, c.key[:-1], STEPS, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_trace_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.glwe_trace_batch(c.out, c.inp, c.key, STEPS, K, 4, LEVELS, workspace=c.ws[:255])
    with pytest.raises(Panic):                                                 # ... and an even exponent
        pl.glwe_automorphism_keyswitch_batch(c.out, c.inp, one, 4, K, 4, LEVELS)
    for fn, args in ((pl.glwe_automorphism_keyswitch_workspace_bytes, (K, LEVELS, -1)), (pl.glwe_automorphism_keyswitch_workspace_bytes, (K, 0, 1)),
                     (pl.glwe_trace_workspace_bytes, (-1, LEVELS, 1)), (pl.glwe_trace_workspace_bytes, (K, 0, 1))):
        with pytest.raises(Panic):
            fn(*args)
    assert c.untouched()
