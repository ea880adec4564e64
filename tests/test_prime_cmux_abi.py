"""C ABI of the prime plans' CMux and CMux tree (include/cntt_prime_cmux.h): the header is plain C11 on its own and includes
cntt_prime_pbs.h only, its names are the four per word width plus the grid function, all are exported, every CNTT_EINVAL case is refused
on host buffers by the argument checks that precede any device call (output poison intact, argument named), the workspace sizes are the
header's formulas, the grid rule is what the header says, the Python wrappers panic on bad shapes, and the code object of the new unit
has its eight kernels without scratch or spills.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from prime_cmux_model import HEADER, cmux_tree_workspace_bytes, cmux_workspace_bytes, grid
from test_prime_automorphism_abi import Raw, declarations, err, ptr
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["glwe_cmux_batch", "glwe_cmux_workspace_bytes", "cmux_tree_batch", "cmux_tree_workspace_bytes"]
GRID = "cntt_prime_cmux_grid"
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS} | {GRID}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert len(NEW) == 9 and set(decl) == NEW and len(decl) == 9
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_prime_pbs.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "the digits are NOT negated" in flat and "nterms = (k + 1) levels, nout = k + 1, accumulate = 1" in flat
    assert "c_s[j] = cmux(sel = selector depth - s, c0 = c_(s-1)[j], c1 = c_(s-1)[j + h])" in flat
    assert "the key pointer is advanced by k levels (k + 1) polynomials" in flat and "strict-range caveat" in flat
    assert "up(batch (k + 1) levels n sizeof(T))" in flat
    assert ("up(max(batch H levels, batch Q (k + 1) levels) n sizeof(T)) + up(batch H (k + 1) n sizeof(T)) + up(batch Q (k + 1) n sizeof(T))"
            in flat)
    assert "rot_t[i batch + b] = 2n - 2^i" in flat and "lut_per_element = 1" in flat and "sample_extract_batch(index = 0)" in flat
    assert "profiles/r23_prime_cmux.txt" in flat
    for name in ("cntt.h", "cntt_ext.h", "cntt_prime_pbs.h", "cntt_prime_ring_pack.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert "cntt_prime_cmux.h" not in other and not (NEW & set(declarations(os.path.join(ROOT, "include", name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_ring_pack_abi.py reads its unit: the one kernel x two word
    types x streaming or not x ciphertext sources or table leaves, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_cmux.o")
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
    assert len(seen) == 8, seen
    for word in ("Ij", "Im"):
        for stream in "01":
            for leaf in "01":
                tag = "4cntt22prime_cmux_diff_kernel%sLb%sELb%sE" % (word, stream, leaf)
                assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_are_the_formulas_of_the_header(mod, p, wb):
    for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
        plan = mod.Plan.try_new(n, p)
        assert plan.glwe_cmux_workspace_bytes(k, levels, batch) == cmux_workspace_bytes(n, wb, k, levels, batch)
        for m in (1, 2, 4, 8, 64, 4096):
            assert plan.cmux_tree_workspace_bytes(m, k, levels, batch) == cmux_tree_workspace_bytes(n, wb, m, k, levels, batch), (n, m, k)
    # the three parts, spelled out once: M = 8 at n = 32, k = 1, levels = 3, batch = 5 on 8-byte words -> H = 4, Q = 2
    if wb == 8:
        assert mod.Plan.try_new(32, p).cmux_tree_workspace_bytes(8, 1, 3, 5) == 5 * 4 * 3 * 32 * 8 + 5 * 4 * 2 * 32 * 8 + 5 * 2 * 2 * 32 * 8
        assert mod.Plan.try_new(32, p).cmux_tree_workspace_bytes(1, 1, 3, 5) == 0
    L = cntt.lib()
    assert getattr(L, "cntt_prime%d_glwe_cmux_workspace_bytes" % (8 * wb))(None, 1, 2, 3) == 0
    assert getattr(L, "cntt_prime%d_cmux_tree_workspace_bytes" % (8 * wb))(None, 4, 1, 2, 3) == 0


def test_grid_rule():
    """one workgroup per output polynomial up to 8 per CU of a 256-CU part; nothing is staged, so neither the size nor the word enters"""
    g = cntt.lib().cntt_prime_cmux_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    for polys in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 11, 12, 13, 14):
            for w in (4, 8):
                assert g(polys, logn, w) == grid(polys, logn, w), (polys, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, M = 32, 1, 2, 3, 4
DEPTH = 2
POISON = 7
SEL = (K + 1) * LEVELS * (K + 1) * N


class Case:
    """Valid host arguments at n = 32: k = 1, levels = 3, 2 pairs of GLWE ciphertexts, 2 tables of 4 polynomials, two selectors; the
    output filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.c0 = np.arange(B * (K + 1) * N, dtype=self.dtype)
        self.c1 = np.arange(B * (K + 1) * N, dtype=self.dtype) + 3
        self.lut = np.arange(B * M * N, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * N, POISON, dtype=self.dtype)
        self.sel = np.zeros(DEPTH * SEL, dtype=self.dtype)
        self.ws = np.zeros(max(self.plan.cmux_tree_workspace_bytes(M, K, LEVELS, B), self.plan.glwe_cmux_workspace_bytes(K, LEVELS, B)), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def pick(self, **kw):
        return {k: (getattr(self, k) if isinstance(v, str) else v) for k, v in kw.items()}

    def cmux(self, plan="own", out="own", c0="own", c1="own", sel="own", k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, c0=c0, c1=c1, sel=sel)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("glwe_cmux_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["c0"]), ptr(a["c1"]), ptr(a["sel"]), k, base_log,
                                          levels, batch, ptr(ws), wsb, 0, None)

    def tree(self, plan="own", out="own", lut="own", sel="own", m=M, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, lut=lut, sel=sel)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("cmux_tree_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lut"]), ptr(a["sel"]), m, k, base_log, levels,
                                          batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all())


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
    cmux_ws = c.plan.glwe_cmux_workspace_bytes(K, LEVELS, B)
    tree_ws = c.plan.cmux_tree_workspace_bytes(M, K, LEVELS, B)

    def refused(call, kw, word):
        assert call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw

    shared = [
        (dict(plan=None), "plan"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the bit length"),
        (dict(out=None), "glwe_out is NULL"),
        (dict(sel=None), "ggsw_ntt is NULL"),
        (dict(out=out_in_big, sel=big[8:8 + c.sel.size]), "glwe_out overlaps ggsw_ntt"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(sel=big[:c.sel.size], ws=ws_in_big), "workspace overlaps ggsw_ntt"),
        (dict(sel=Raw(c.sel.ctypes.data + w // 2)), "ggsw_ntt is not"),
        (dict(out=Raw(c.out.ctypes.data + w // 2)), "glwe_out is not"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
    ]
    # call 1
    for kw, word in shared + [
            (dict(k=1 << 31, levels=1, batch=1), "2^63 bytes"),                       # the launch bound passes, the selector does not fit
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
            (dict(k=1 << 31, levels=1, batch=1, m=2), "2^63 bytes"),
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


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_one_entry_needs_no_selector(bits, p):
    c = Case(bits, p)
    assert c.fn("glwe_cmux_batch")(c.plan._h, None, None, None, None, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.fn("cmux_tree_batch")(c.plan._h, None, None, None, M, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.cmux(batch=0) == 0 and c.tree(batch=0) == 0 and c.untouched()
    # lut_count = 1 with a NULL selector passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    out = np.zeros(B * (K + 1) * N, dtype=c.dtype)
    assert c.tree(m=1, sel=None, lut=c.lut[:B * N], out=out) != EINVAL
    # k = 0 is valid, and every valid lut_count passes with the workspace of its own formula
    body = np.arange(B * N, dtype=c.dtype)
    assert c.cmux(k=0, c0=body, c1=body + 1, out=np.zeros(B * N, dtype=c.dtype), sel=np.zeros(LEVELS * N, dtype=c.dtype)) != EINVAL
    for m in (1, 2, 4, 8, 16):
        ws = np.zeros(c.plan.cmux_tree_workspace_bytes(m, K, LEVELS, 1), dtype=np.uint8)
        depth = m.bit_length() - 1
        assert c.tree(m=m, batch=1, lut=np.zeros(m * N, dtype=c.dtype), out=np.zeros((K + 1) * N, dtype=c.dtype),
                      sel=np.zeros(max(depth, 1) * SEL, dtype=c.dtype), ws=ws if ws.size else None) != EINVAL, m


def test_full_word_digits_are_valid():
    """base_log * levels = W exactly, base_log = W included"""
    for bits, p in ((64, PM64), (32, P32), (64, P62)):
        c = Case(bits, p)
        W = wbits(p)
        assert c.cmux(base_log=W, levels=1, sel=np.zeros((K + 1) * (K + 1) * N, dtype=c.dtype)) != EINVAL
        assert c.tree(base_log=W // 2, levels=2, sel=np.zeros(DEPTH * (K + 1) * 2 * (K + 1) * N, dtype=c.dtype)) != EINVAL


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    one = c.sel[:SEL]
    for args in [(c.out[:-N], c.c0, c.c1, one, K, 4, LEVELS), (c.out, c.c0, c.c1[:-N], one, K, 4, LEVELS), (c.out, c.c0[:-1], c.c1, one, K, 4, LEVELS),
                 (c.out, c.c0, c.c1, one[:-N], K, 4, LEVELS), (c.out, c.c0, c.c1, one, K, 4, LEVELS + 1), (c.out, c.c0, c.c1, c.sel, K, 4, LEVELS),
                 (c.out, c.c0, c.c1, one, -1, 4, LEVELS), (c.out, c.c0, c.c1, one, K, 0, LEVELS), (c.out, c.c0, c.c1, one, K, 4, 0)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_cmux_batch(*args)
    for args in [(c.out[:-N], c.lut, c.sel, M, K, 4, LEVELS), (c.out, c.lut[:-1], c.sel, M, K, 4, LEVELS), (c.out, c.lut, one, M, K, 4, LEVELS),
                 (c.out, c.lut, c.sel, 0, K, 4, LEVELS), (c.out, c.lut[:B * 3 * N], c.sel, 3, K, 4, LEVELS), (c.out, c.lut, c.sel, M, K, 0, LEVELS),
                 (c.out, c.lut, c.sel, M, K, 4, 0), (c.out, c.lut, None, M, K, 4, LEVELS), (c.out, c.lut, c.sel, M, -1, 4, LEVELS)]:
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
