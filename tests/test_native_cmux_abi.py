"""C ABI of the native plans' CMux and CMux tree (include/cntt_cmux.h): the header is plain C11 on its own and includes cntt_ext.h only,
its names are the five it declares, none of them reaches cntt.h or cntt_ext.h, all are exported, every CNTT_EINVAL case is refused on
host buffers by the argument checks that precede any device call (output poison intact, argument named), the workspace sizes are the
header's formulas, the grid rule is what the header says, the Python wrappers panic on bad shapes, and the code object of the new unit
has its twelve kernels without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary64
from concrete_ntt_amd._lib import EINVAL, Panic
from native_cmux_model import HEADER, cmux_tree_workspace_bytes, cmux_workspace_bytes, grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW = {"cntt_native_glwe_cmux_batch", "cntt_native_glwe_cmux_workspace_bytes", "cntt_native_cmux_tree_batch",
       "cntt_native_cmux_tree_workspace_bytes", "cntt_native_cmux_grid"}


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
    assert set(decl) == NEW and len(decl) == 5
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_ext.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "nterms = (k + 1) levels, nout = k + 1, accumulate = 1" in flat and "CNTT_SRC_PLAIN, npolys = k + 1" in flat
    assert "c_s[j] = cmux(sel = selector depth - s, c0 = c_(s-1)[j], c1 = c_(s-1)[j + h])" in flat
    assert "every plane pointer is advanced by k levels (k + 1) residue polynomials" in flat
    assert "the leaf form EQUALS call 1 on the trivial ciphertexts, word for word, for every kind" in flat
    assert "row j = q levels + (l - 1) sits at polynomial j (k + 1) + o" in flat
    assert "rot_t[i batch + b] = 2n - 2^i" in flat and "lut_per_element = 1" in flat and "sample_extract_batch(index = 0)" in flat
    assert "(k + 1) levels > cntt_native_max_terms(plan)" in flat and "not a measured optimum" in flat
    assert "profiles/r25_native_cmux.txt" in flat
    for name in ("cntt.h", "cntt_ext.h", "cntt_gadget.h", "cntt_pbs.h", "cntt_multibit.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, name)).read(), flags=re.S)
        assert "cntt_cmux.h" not in other and not (NEW & set(declarations(os.path.join(INC, name)))), name
    for name in ("cntt.h", "cntt_ext.h"):                                        # ... not even in a comment
        assert "cntt_cmux.h" not in open(os.path.join(INC, name)).read(), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_cmux_abi.py reads its unit: the one kernel x three word
    types x streaming or not x ciphertext sources or table leaves, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_cmux.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "cmux.fat"), str(tmp_path / "cmux.co")
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
    assert len(seen) == 12, seen
    for word in ("Ij", "Im", "INS_7Word128E"):
        for stream in "01":
            for leaf in "01":
                tag = "4cntt23native_cmux_diff_kernel%sLb%sELb%sE" % (word, stream, leaf)
                assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("mod", [native32, native64, native128, native_binary64])
def test_workspace_bytes_are_the_formulas_of_the_header(mod):
    for P in (mod.Plan32, getattr(mod, "Plan52", None)):
        if P is None:
            continue
        for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
            plan = P.try_new(n)
            wb = plan.WORD
            assert plan.glwe_cmux_workspace_bytes(k, levels, batch) == cmux_workspace_bytes(n, wb, k, levels, batch)
            for m in (1, 2, 4, 8, 64, 4096):
                assert plan.cmux_tree_workspace_bytes(m, k, levels, batch) == cmux_tree_workspace_bytes(n, wb, m, k, levels, batch), (n, m, k)
    # the three parts, spelled out once: M = 8 at n = 32, k = 1, levels = 3, batch = 5 -> H = 4, Q = 2
    wb = mod.Plan32.WORD
    assert mod.Plan32.try_new(32).cmux_tree_workspace_bytes(8, 1, 3, 5) == 5 * 4 * 3 * 32 * wb + 5 * 4 * 2 * 32 * wb + 5 * 2 * 2 * 32 * wb
    assert mod.Plan32.try_new(32).cmux_tree_workspace_bytes(1, 1, 3, 5) == 0
    L = cntt.lib()
    assert L.cntt_native_glwe_cmux_workspace_bytes(None, 1, 2, 3) == 0 and L.cntt_native_cmux_tree_workspace_bytes(None, 4, 1, 2, 3) == 0


def test_grid_rule():
    """one workgroup per output polynomial up to 8 per CU of a 256-CU part; nothing is staged, so neither the size nor the word enters"""
    g = cntt.lib().cntt_native_cmux_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    for polys in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 11, 12, 13, 14):
            for w in (4, 8, 16):
                assert g(polys, logn, w) == grid(polys, logn, w), (polys, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, M = 32, 1, 2, 3, 4
DEPTH = 2
POISON = 7
SEL = (K + 1) * LEVELS * (K + 1) * N


class Raw:
    """a bare address standing for a buffer"""

    def __init__(self, address):
        self.address = address


def ptr(a):
    if a is None:
        return None
    return ctypes.c_void_p(a.address if isinstance(a, Raw) else a.ctypes.data)


class Case:
    """Valid host arguments at n = 32: k = 1, levels = 3, 2 pairs of GLWE ciphertexts, 2 tables of 4 polynomials, two selectors as
    residue planes; the output filled with 7."""

    def __init__(self, P):
        self.plan = P.try_new(N)
        self.dtype, self.pe = self.plan.word_dtype, N * (2 if self.plan.WORD == 16 else 1)
        self.c0 = np.arange(B * (K + 1) * self.pe, dtype=self.dtype)
        self.c1 = np.arange(B * (K + 1) * self.pe, dtype=self.dtype) + 3
        self.lut = np.arange(B * M * self.pe, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * self.pe, POISON, dtype=self.dtype)
        self.sel = [np.zeros(DEPTH * SEL, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.ws = np.zeros(max(self.plan.cmux_tree_workspace_bytes(M, K, LEVELS, B), self.plan.glwe_cmux_workspace_bytes(K, LEVELS, B)), dtype=np.uint8)

    def planes(self, sel):
        if sel is None:
            return None
        return (ctypes.c_void_p * self.plan.NPRIMES)(*[None if p is None else ptr(p) for p in sel])

    def pick(self, **kw):
        return {k: (getattr(self, k) if isinstance(v, str) else v) for k, v in kw.items()}

    def cmux(self, plan="own", out="own", c0="own", c1="own", sel="own", k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, c0=c0, c1=c1, sel=sel)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_glwe_cmux_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["c0"]), ptr(a["c1"]),
                                                      self.planes(a["sel"]), k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def tree(self, plan="own", out="own", lut="own", sel="own", m=M, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, lut=lut, sel=sel)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_cmux_tree_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lut"]), self.planes(a["sel"]),
                                                      m, k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all())


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_every_invalid_argument_is_refused(P):
    c = Case(P)
    W, w, rb = 8 * c.plan.WORD, c.plan.WORD, c.plan.RES
    big = np.full(16384, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    plane_in_big = big.view(c.plan.res_dtype)[8 * w // rb:8 * w // rb + c.sel[0].size]     # starts 8 words into `big`
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    cmux_ws = c.plan.glwe_cmux_workspace_bytes(K, LEVELS, B)
    tree_ws = c.plan.cmux_tree_workspace_bytes(M, K, LEVELS, B)

    def refused(call, kw, word):
        assert call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw

    def with_plane(i, p):
        return c.sel[:i] + [p] + c.sel[i + 1:]

    last = c.plan.NPRIMES - 1
    shared = [
        (dict(plan=None), "plan is NULL"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the word width %d" % W),
        (dict(out=None), "glwe_out is NULL"),
        (dict(sel=None), "ggsw_ntt is NULL"),
        (dict(sel=with_plane(last, None)), "NULL key residue plane (ggsw_ntt[%d])" % last),
        (dict(out=out_in_big, sel=with_plane(0, plane_in_big)), "glwe_out overlaps ggsw_ntt[0]"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(sel=with_plane(last, plane_in_big), ws=ws_in_big), "workspace overlaps ggsw_ntt[%d]" % last),
        (dict(sel=with_plane(1 % c.plan.NPRIMES, Raw(c.sel[0].ctypes.data + rb // 2))), "ggsw_ntt[%d] is not" % (1 % c.plan.NPRIMES)),
        (dict(out=Raw(c.out.ctypes.data + w // 2)), "glwe_out is not"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "workspace is not 16-byte aligned"),
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
    ]
    # call 1
    for kw, word in shared + [
            (dict(c0=None), "glwe0 is NULL"), (dict(c1=None), "glwe1 is NULL"),
            (dict(out=out_in_big, c0=big[8:8 + c.c0.size]), "glwe_out overlaps glwe0"),
            (dict(out=out_in_big, c1=big[8:8 + c.c1.size]), "glwe_out overlaps glwe1"),
            (dict(c0=big[:c.c0.size], ws=ws_in_big), "workspace overlaps glwe0"),
            (dict(c1=big[:c.c1.size], ws=ws_in_big), "workspace overlaps glwe1"),
            (dict(c0=Raw(c.c0.ctypes.data + 1)), "glwe0 is not"), (dict(c1=Raw(c.c1.ctypes.data + 1)), "glwe1 is not"),
            (dict(ws=c.ws, ws_bytes=cmux_ws - 1), "workspace_bytes"),
            # batch * (k + 1) * levels >= 2^32
            (dict(batch=(1 << 32) // ((K + 1) * LEVELS) + 1), "2^32"), (dict(batch=1 << 32, k=0, levels=1), "2^32"), (dict(batch=1 << 63), "2^32")]:
        refused(c.cmux, kw, word)
    assert c.cmux(out=c.c0) == EINVAL and "glwe_out overlaps glwe0" in err()          # no call runs in place
    # call 2
    for kw, word in shared + [
            (dict(m=0), "lut_count = 0"), (dict(m=3), "lut_count = 3"), (dict(m=12), "lut_count = 12"), (dict(m=(1 << 63) + 1), "lut_count"),
            (dict(lut=None), "lut_in is NULL"),
            (dict(out=out_in_big, lut=big[8:8 + c.lut.size]), "glwe_out overlaps lut_in"),
            (dict(lut=big[:c.lut.size], ws=ws_in_big), "workspace overlaps lut_in"),
            (dict(lut=Raw(c.lut.ctypes.data + 1)), "lut_in is not"),
            (dict(ws=c.ws, ws_bytes=tree_ws - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=256), "workspace_bytes"),
            # batch * max(H, 1) * (k + 1) * levels >= 2^32 with H = M / 2 = 2: half the batch of call 1 is refused already
            (dict(batch=(1 << 32) // (2 * (K + 1) * LEVELS) + 1), "2^32"), (dict(batch=1 << 31, k=0, levels=1), "2^32"),
            (dict(batch=(1 << 32) // ((K + 1) * LEVELS) + 1, m=1), "2^32"), (dict(m=1 << 40, batch=1), "2^32"),
            (dict(m=1 << 62, batch=4), "2^32")]:
        refused(c.tree, kw, word)


def test_max_terms_is_one_rule_for_both_calls():
    """native64 Plan32 at n = 32768 holds 61 terms: k = 0, base_log = 1, levels = 62 fits the word (62 <= 64) and not the exact range.
    Refused by call 1 and by every tree with M >= 2 -- the leaf stage alone (M = 2) included -- and not by M = 1, which sums nothing."""
    plan = native64.Plan32.try_new(32768)
    assert plan.max_terms() == 61
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * 5)(*[16] * 5)
    assert L.cntt_native_glwe_cmux_batch(plan._h, p(16), p(16), p(16), dummy, 0, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "(glwe_dim + 1) * levels = 62 exceeds cntt_native_max_terms() = 61" in err()
    for m in (2, 4, 1 << 20):
        assert L.cntt_native_cmux_tree_batch(plan._h, p(16), p(16), dummy, m, 0, 1, 62, 1, None, 0, 0, None) == EINVAL, m
        assert "(glwe_dim + 1) * levels = 62 exceeds cntt_native_max_terms() = 61" in err(), m
    assert L.cntt_native_cmux_tree_batch(plan._h, None, p(16), None, 1, 0, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "glwe_out is NULL" in err()                                          # M = 1 got past the size checks
    assert L.cntt_native_glwe_cmux_batch(plan._h, None, p(16), p(16), dummy, 0, 1, 61, 1, None, 0, 0, None) == EINVAL and "glwe_out is NULL" in err()


def test_byte_counts_past_2_63_are_refused_before_they_are_formed():
    """native32 Plan52 at n = 16 holds 2^31 - 89 terms, so glwe_dim + 1 = 2^30 passes the term and the launch bounds, and its selector
    of 2^60 polynomials does not fit"""
    plan = native32.Plan52.try_new(16)
    assert plan.max_terms() > 1 << 30
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * plan.NPRIMES)(*[16] * plan.NPRIMES)
    assert L.cntt_native_glwe_cmux_batch(plan._h, p(16), p(16), p(16), dummy, (1 << 30) - 1, 1, 1, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()
    assert L.cntt_native_cmux_tree_batch(plan._h, p(16), p(16), dummy, 2, (1 << 30) - 1, 1, 1, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32])
def test_batch_zero_does_nothing_and_one_entry_needs_no_selector(P):
    c = Case(P)
    L = cntt.lib()
    assert L.cntt_native_glwe_cmux_batch(c.plan._h, None, None, None, None, K, 8, 3, 0, None, 0, 0, None) == 0
    assert L.cntt_native_cmux_tree_batch(c.plan._h, None, None, None, M, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.cmux(batch=0) == 0 and c.tree(batch=0) == 0 and c.untouched()
    # lut_count = 1 with a NULL selector passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    out = np.zeros(B * (K + 1) * N, dtype=c.dtype)
    assert c.tree(m=1, sel=None, lut=c.lut[:B * N], out=out) != EINVAL
    # k = 0 is valid, and every valid lut_count passes with the workspace of its own formula
    body = np.arange(B * N, dtype=c.dtype)
    planes = [np.zeros(LEVELS * N, dtype=c.plan.res_dtype) for _ in range(c.plan.NPRIMES)]
    assert c.cmux(k=0, c0=body, c1=body + 1, out=np.zeros(B * N, dtype=c.dtype), sel=planes) != EINVAL
    for m in (1, 2, 4, 8, 16):
        ws = np.zeros(c.plan.cmux_tree_workspace_bytes(m, K, LEVELS, 1), dtype=np.uint8)
        depth = m.bit_length() - 1
        planes = [np.zeros(max(depth, 1) * SEL, dtype=c.plan.res_dtype) for _ in range(c.plan.NPRIMES)]
        assert c.tree(m=m, batch=1, lut=np.zeros(m * N, dtype=c.dtype), out=np.zeros((K + 1) * N, dtype=c.dtype), sel=planes,
                      ws=ws if ws.size else None) != EINVAL, m


def test_full_word_digits_are_valid():
    """base_log * levels = w exactly, base_log = w included"""
    for P in (native64.Plan32, native32.Plan32, native128.Plan32):
        c = Case(P)
        W = 8 * c.plan.WORD
        one = [np.zeros((K + 1) * (K + 1) * N, dtype=c.plan.res_dtype) for _ in range(c.plan.NPRIMES)]
        two = [np.zeros(DEPTH * (K + 1) * 2 * (K + 1) * N, dtype=c.plan.res_dtype) for _ in range(c.plan.NPRIMES)]
        assert c.cmux(base_log=W, levels=1, sel=one) != EINVAL
        assert c.tree(base_log=W // 2, levels=2, sel=two) != EINVAL


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32])
def test_python_wrappers_panic_on_bad_shapes(P):
    c = Case(P)
    pl, pe = c.plan, c.pe
    one = [p[:SEL] for p in c.sel]
    for args in [(c.out[:-pe], c.c0, c.c1, one, K, 4, LEVELS), (c.out, c.c0, c.c1[:-pe], one, K, 4, LEVELS), (c.out, c.c0[:-2], c.c1, one, K, 4, LEVELS),
                 (c.out, c.c0, c.c1, [p[:-N] for p in one], K, 4, LEVELS), (c.out, c.c0, c.c1, one, K, 4, LEVELS + 1), (c.out, c.c0, c.c1, c.sel, K, 4, LEVELS),
                 (c.out, c.c0, c.c1, one[:-1], K, 4, LEVELS), (c.out, c.c0, c.c1, one, -1, 4, LEVELS), (c.out, c.c0, c.c1, one, K, 0, LEVELS),
                 (c.out, c.c0, c.c1, one, K, 4, 0)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_cmux_batch(*args)
    for args in [(c.out[:-pe], c.lut, c.sel, M, K, 4, LEVELS), (c.out, c.lut[:-2], c.sel, M, K, 4, LEVELS), (c.out, c.lut, one, M, K, 4, LEVELS),
                 (c.out, c.lut, c.sel, 0, K, 4, LEVELS), (c.out, c.lut[:B * 3 * pe], c.sel, 3, K, 4, LEVELS), (c.out, c.lut, c.sel, M, K, 0, LEVELS),
                 (c.out, c.lut, c.sel, M, K, 4, 0), (c.out, c.lut, None, M, K, 4, LEVELS), (c.out, c.lut, c.sel, M, -1, 4, LEVELS),
                 (c.out, c.lut, c.sel[:-1], M, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.cmux_tree_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.cmux_tree_batch(c.out, c.lut, c.sel, M, K, 4, LEVELS, workspace=c.ws[:255])
    with pytest.raises(Panic):
        pl.glwe_cmux_batch(c.out, c.c0, c.c1, one, K, 4, LEVELS, workspace=c.ws[:255])
    for fn, args in ((pl.glwe_cmux_workspace_bytes, (K, LEVELS, -1)), (pl.glwe_cmux_workspace_bytes, (K, 0, 1)),
                     (pl.cmux_tree_workspace_bytes, (0, K, LEVELS, 1)), (pl.cmux_tree_workspace_bytes, (M, K, LEVELS, -1))):
        with pytest.raises(Panic):
            fn(*args)
    assert c.untouched()
