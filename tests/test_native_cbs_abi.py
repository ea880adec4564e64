"""C ABI of the native plans' circuit bootstrap (include/cntt_cbs.h): the header is plain C11 on its own and includes cntt_cmux.h only, its
names are the three it declares, all are exported, every CNTT_EINVAL case is refused on host buffers by the argument checks that precede
any device call (output poison intact, argument named), the workspace size is the header's formula, the grid rule is what the header says,
the Python wrappers panic on bad shapes, and the code object of the new unit has its twelve kernels without scratch or spills.  No GPU
needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary32, native_binary64, native_binary128
from concrete_ntt_amd._lib import EINVAL, Panic
from native_cbs_model import HEADER, cbs_workspace_bytes, grid
from test_native_cmux_abi import Raw, declarations, err, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW = {"cntt_native_circuit_bootstrap_batch", "cntt_native_circuit_bootstrap_workspace_bytes", "cntt_native_cbs_grid"}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert set(decl) == NEW and len(decl) == 3
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_cmux.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "PLAIN WORDS IN THE COEFFICIENT DOMAIN" in flat and "2 has no inverse mod 2^w" in flat and "NOT checked here" in flat
    assert "lwe_dim_in = Lin + 1, lwe_count = 1, the body word 0" in flat and "profiles/r26_native_cbs.txt" in flat
    for name in ("cntt.h", "cntt_ext.h", "cntt_pbs.h", "cntt_cmux.h", "cntt_prime_cbs.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, name)).read(), flags=re.S)
        assert "cntt_cbs.h" not in other and not (NEW & set(declarations(os.path.join(INC, name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_native_cmux_abi.py reads its unit: four kernels x three word types,
    none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_cbs.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "cbs.fat"), str(tmp_path / "cbs.co")
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
        for kernel in ("23native_cbs_setup_kernel", "25native_cbs_extract_kernel", "20native_cbs_ks_kernel", "21native_cbs_sum_kernel"):
            tag = "4cntt%s%sE" % (kernel, word)
            assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("P", [native32.Plan32, native64.Plan32, native128.Plan32, native32.Plan52, native64.Plan52])
def test_workspace_bytes_are_the_formula_of_the_header(P):
    for n, k in ((32, 1), (1024, 1), (256, 3), (2048, 2), (64, 0)):
        plan = P.try_new(n)
        for L, pl, Lk, Lc, batch in ((0, 1, 1, 1, 1), (3, 2, 3, 2, 3), (630, 3, 1, 2, 10), (700, 1, 2, 4, 64), (5, 2, 1, 1, 8195), (1, 1, 1, 1, 0)):
            assert plan.circuit_bootstrap_workspace_bytes(L, k, pl, Lk, Lc, batch) == cbs_workspace_bytes(n, plan.WORD, L, k, pl, Lk, Lc, batch), (n, k, L, batch)
    assert cntt.lib().cntt_native_circuit_bootstrap_workspace_bytes(None, 3, 1, 2, 2, 2, 3) == 0


def test_grid_rule():
    """one workgroup per work item up to 8 per CU of a 256-CU part; neither the size nor the word enters"""
    g = cntt.lib().cntt_native_cbs_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    for items in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 14):
            for w in (4, 8, 16):
                assert g(items, logn, w) == grid(items, logn, w), (items, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, L = 32, 1, 2, 3
PBS, KS, CBS = (4, 2), (5, 3), (6, 2)
POISON = 7
R = (K * N + 1) * KS[1]


class Case:
    """Valid host arguments at n = 32: k = 1, L = 3, 2 bits, gadgets (4, 2), (5, 3), (6, 2); the output planes filled with 7."""

    def __init__(self, P):
        self.plan = P.try_new(N)
        self.dtype, self.pe = self.plan.word_dtype, N * (2 if self.plan.WORD == 16 else 1)
        self.np = self.plan.NPRIMES
        self.lwe = np.arange(B * (L + 1) * self.pe // N, dtype=self.dtype)
        self.bsk = [np.zeros(L * (K + 1) * PBS[1] * (K + 1) * N, dtype=self.plan.res_dtype) for _ in range(self.np)]
        self.fk = np.zeros((K + 1) * R * (K + 1) * self.pe, dtype=self.dtype)
        self.out = [np.full(B * (K + 1) * CBS[1] * (K + 1) * N, POISON, dtype=self.plan.res_dtype) for _ in range(self.np)]
        self.ws = np.zeros(self.plan.circuit_bootstrap_workspace_bytes(L, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)

    def planes(self, ps):
        if ps is None:
            return None
        return (ctypes.c_void_p * self.np)(*[None if p is None else ptr(p) for p in ps])

    def call(self, plan="own", out="own", lwe="own", bsk="own", fk="own", lwe_dim=L, k=K, pbs=PBS, ks=KS, cbs=CBS, batch=B, ws=None, ws_bytes=None):
        a = {name: (getattr(self, name) if isinstance(v, str) else v) for name, v in dict(out=out, lwe=lwe, bsk=bsk, fk=fk).items()}
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_circuit_bootstrap_batch(self.plan._h if plan == "own" else None, self.planes(a["out"]), ptr(a["lwe"]),
                                                              self.planes(a["bsk"]), ptr(a["fk"]), lwe_dim, k, pbs[0], pbs[1], ks[0], ks[1], cbs[0],
                                                              cbs[1], batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return all(bool((o == POISON).all()) for o in self.out)


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_every_invalid_argument_is_refused(P):
    c = Case(P)
    W, w, rb = 8 * c.plan.WORD, c.plan.WORD, c.plan.RES
    big = np.full(1 << 16, POISON, dtype=np.uint64)
    bigr, bigw = big.view(c.plan.res_dtype), big.view(c.dtype)
    out_in_big = bigr[:c.out[0].size]
    ws_in_big = big.view(np.uint8)[256:256 + c.ws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16

    def with_plane(planes, i, p):
        return [p if j == i else x for j, x in enumerate(planes)]

    last = c.np - 1
    for kw, word in [
            (dict(plan=None), "plan"),
            (dict(pbs=(0, 2)), "pbs_base_log is 0"), (dict(pbs=(4, 0)), "pbs_levels is 0"), (dict(pbs=(W, 2)), "pbs_base_log * pbs_levels"),
            (dict(ks=(0, 2)), "ks_base_log is 0"), (dict(ks=(4, 0)), "ks_levels is 0"), (dict(ks=(W // 3 + 1, 3)), "ks_base_log * ks_levels"),
            (dict(ks=(32, 1)), "ks_base_log = 32 is above 31"),
            (dict(cbs=(0, 2)), "cbs_base_log is 0"), (dict(cbs=(4, 0)), "cbs_levels is 0"), (dict(cbs=(W // 2 + 1, 2)), "cbs_base_log * cbs_levels"),
            (dict(cbs=(W // 2, 2)), "2 has no inverse mod 2^w"), (dict(cbs=(W, 1)), "2 has no inverse mod 2^w"),
            (dict(k=(1 << 32) - 1), "glwe_dim"), (dict(k=(1 << 64) - 1), "glwe_dim"),
            (dict(k=1 << 27, pbs=(4, 1), cbs=(6, 1), batch=1), "cntt_native_max_terms" if (1 << 27) + 1 > c.plan.max_terms() else "2^32 key rows"),
            (dict(ks=(1, 30), k=0, batch=1 << 40, cbs=(6, 1), pbs=(4, 1)), "2^32"), (dict(batch=1 << 63), "2^32"),
            (dict(batch=(1 << 32) // (CBS[1] * (K + 1) * PBS[1]) + 1), "2^32"),
            (dict(lwe_dim=1 << 60), "2^63 bytes"),
            (dict(out=None), "ggsw_ntt_out is NULL"), (dict(out=with_plane(c.out, last, None)), "ggsw_ntt_out[%d]" % last),
            (dict(lwe=None), "lwe_in is NULL"), (dict(bsk=None), "bsk_ntt is NULL"), (dict(bsk=with_plane(c.bsk, 0, None)), "bsk_ntt[0]"),
            (dict(fk=None), "fpksk is NULL"),
            (dict(out=with_plane(c.out, 0, out_in_big), lwe=bigw[8 * c.pe // N:8 * c.pe // N + c.lwe.size]), "ggsw_ntt_out[0] overlaps lwe_in"),
            (dict(out=with_plane(c.out, last, out_in_big), bsk=with_plane(c.bsk, 0, bigr[16:16 + c.bsk[0].size])), "ggsw_ntt_out[%d] overlaps bsk_ntt[0]" % last),
            (dict(out=with_plane(c.out, 0, out_in_big), fk=bigw[:c.fk.size]), "ggsw_ntt_out[0] overlaps fpksk"),
            (dict(out=with_plane(c.out, 0, out_in_big), ws=ws_in_big), "ggsw_ntt_out[0] overlaps workspace"),
            (dict(out=with_plane(c.out, 0, c.out[1])), "ggsw_ntt_out[0] overlaps ggsw_ntt_out[1]") if c.np > 1 else (dict(out=None), "NULL"),
            (dict(lwe=bigw[64 * c.pe // N:64 * c.pe // N + c.lwe.size], ws=ws_in_big), "workspace overlaps lwe_in"),
            (dict(bsk=with_plane(c.bsk, last, bigr[:c.bsk[0].size]), ws=ws_in_big), "workspace overlaps bsk_ntt[%d]" % last),
            (dict(fk=bigw[:c.fk.size], ws=ws_in_big), "workspace overlaps fpksk"),
            (dict(out=with_plane(c.out, 0, Raw(c.out[0].ctypes.data + rb // 2))), "ggsw_ntt_out[0] is not"),
            (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"), (dict(bsk=with_plane(c.bsk, 0, Raw(c.bsk[0].ctypes.data + 1))), "bsk_ntt[0] is not"),
            (dict(fk=Raw(c.fk.ctypes.data + 8)), "fpksk is not 16-byte aligned"),
            (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
            (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=256), "workspace_bytes")]:
        assert c.call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw


def test_key_rows_and_byte_counts_are_bounded():
    c = Case(native64.Plan32)
    for kw, word in [(dict(ks=(1, 30), k=1 << 23, pbs=(4, 1)), "2^32 key rows"), (dict(batch=1, k=1 << 20, pbs=(4, 1)), "2^63 bytes"),
                     (dict(batch=1 << 29, k=7, pbs=(4, 1), cbs=(6, 1)), "2^46")]:
        if c.plan.max_terms() < (kw["k"] + 1):
            continue                                                              # the term rule comes first and refuses it already
        assert c.call(**kw) == EINVAL and word in err(), (kw, err())
        assert c.untouched()


@pytest.mark.parametrize("P", [native_binary32.Plan32, native_binary64.Plan32, native_binary128.Plan32, native_binary32.Plan52, native_binary64.Plan52],
                         ids=["binary32", "binary64", "binary128", "binary32_plan52", "binary64_plan52"])
def test_the_binary_kinds_are_refused(P):
    c = Case(P)
    assert c.call() == EINVAL and "native_binary" in err() and "0/1 key words" in err(), err()
    assert c.call(batch=0) == EINVAL and c.untouched()
    with pytest.raises(Panic):
        c.plan.circuit_bootstrap_batch(c.out, c.lwe, c.bsk, c.fk, L, K, *PBS, *KS, *CBS)


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan52, native128.Plan32], ids=["native64", "native32_plan52", "native128"])
def test_batch_zero_does_nothing_and_lwe_dim_zero_is_valid(P):
    c = Case(P)
    W = 8 * c.plan.WORD
    fn = cntt.lib().cntt_native_circuit_bootstrap_batch
    assert fn(c.plan._h, None, None, None, None, L, K, 4, 2, 5, 3, 6, 2, 0, None, 0, 0, None) == 0
    assert c.call(batch=0) == 0 and c.untouched()
    # lwe_dim = 0 with a NULL bootstrapping key passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    ws = np.zeros(c.plan.circuit_bootstrap_workspace_bytes(0, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)
    out = [np.zeros(c.out[0].size, dtype=c.plan.res_dtype) for _ in range(c.np)]
    assert c.call(lwe_dim=0, bsk=None, lwe=c.lwe[:B * c.pe // N], out=out, ws=ws) != EINVAL
    # the gadgets at their edges: pbs and ks at the whole word, ks_base_log at 31, cbs_base_log * Lc = w - 1, k = 0
    out = [np.zeros(B * N, dtype=c.plan.res_dtype) for _ in range(c.np)]
    assert c.call(k=0, pbs=(W, 1), ks=(31, W // 31), cbs=(W - 1, 1), bsk=[np.zeros(L * N, dtype=c.plan.res_dtype) for _ in range(c.np)],
                  fk=np.zeros(W // 31 * c.pe, dtype=c.dtype), out=out) != EINVAL


@pytest.mark.parametrize("P", [native64.Plan32, native128.Plan32], ids=["native64", "native128"])
def test_python_wrappers_panic_on_bad_shapes(P):
    c = Case(P)
    pl = c.plan
    good = (c.out, c.lwe, c.bsk, c.fk, L, K) + PBS + KS + CBS
    for i, bad in [(0, c.out[:-1]), (0, [o[:-N] for o in c.out]), (1, c.lwe[:-1]), (2, [b[:-N] for b in c.bsk]), (3, c.fk[:-c.pe]), (2, None), (4, -1),
                   (5, -1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0), (11, 3)]:
        args = list(good)
        args[i] = bad
        with pytest.raises((Panic, TypeError)):
            pl.circuit_bootstrap_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.circuit_bootstrap_batch(*good, workspace=c.ws[:255])
    for args in ((L, K, 2, 3, 2, -1), (L, K, 0, 3, 2, 1), (L, K, 2, 0, 2, 1), (L, K, 2, 3, 0, 1), (-1, K, 2, 3, 2, 1)):
        with pytest.raises(Panic):
            pl.circuit_bootstrap_workspace_bytes(*args)
    assert c.untouched()


# -- the order of the refusals: of two wrong arguments the earlier check answers ---------------------------------------------------
@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_of_two_wrong_arguments_the_earlier_check_answers(P):
    c = Case(P)
    W = 8 * c.plan.WORD
    big = np.full(1 << 16, POISON, dtype=np.uint64)
    out_in_big = [big.view(c.plan.res_dtype)[:c.out[0].size]] + c.out[1:]
    ws_in_big = big.view(np.uint8)[256:256 + c.ws.nbytes]
    for kw, word in [
            (dict(plan=None, pbs=(0, 2)), "plan is NULL"),
            (dict(pbs=(0, 2), ks=(0, 2)), "pbs_base_log is 0"), (dict(pbs=(4, 0), cbs=(0, 2)), "pbs_levels is 0"),
            (dict(ks=(W // 3 + 1, 3), cbs=(4, 0)), "ks_base_log * ks_levels"),
            (dict(ks=(32, 1), cbs=(4, 0)), "ks_base_log = 32 is above 31"),
            (dict(cbs=(W // 2, 2), k=(1 << 32) - 1), "2 has no inverse mod 2^w"),
            (dict(k=(1 << 32) - 1, batch=1 << 63), "glwe_dim too large"),
            (dict(batch=1 << 32, lwe_dim=1 << 60), "too large for one launch"),
            (dict(lwe_dim=1 << 60, out=None), "2^63 bytes"),
            (dict(out=None, lwe=None), "ggsw_ntt_out is NULL"),
            (dict(lwe=None, fk=None), "lwe_in is NULL"), (dict(bsk=None, fk=None), "bsk_ntt is NULL"),
            (dict(fk=None, ws=c.ws, ws_bytes=c.ws.nbytes - 1), "fpksk is NULL"),
            (dict(out=out_in_big, ws=ws_in_big, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
            (dict(lwe=Raw(c.lwe.ctypes.data + 1), out=out_in_big, ws=ws_in_big), "lwe_in is not")]:
        assert c.call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw


def test_the_binary_kinds_are_refused_before_the_gadgets():
    c = Case(native_binary64.Plan32)
    assert c.call(pbs=(0, 2)) == EINVAL and "native_binary" in err(), err()
    assert c.call(pbs=(4, 0), cbs=(0, 0), ks=(32, 1)) == EINVAL and "native_binary" in err(), err()
    assert c.untouched()
