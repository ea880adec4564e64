"""C ABI of the prime plans' circuit bootstrap (include/cntt_prime_cbs.h): the header is plain C11 on its own and includes
cntt_prime_cmux.h only, its names are the two per word width plus the grid function, all are exported, every CNTT_EINVAL case is refused
on host buffers by the argument checks that precede any device call (output poison intact, argument named), the workspace size is the
header's formula, the grid rule is what the header says, the Python wrappers panic on bad shapes, and the code object of the new unit
has its eight kernels without scratch or spills.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from prime_cbs_model import HEADER, cbs_workspace_bytes, grid
from test_prime_automorphism_abi import Raw, declarations, err, ptr
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["circuit_bootstrap_batch", "circuit_bootstrap_workspace_bytes"]
GRID = "cntt_prime_cbs_grid"
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS} | {GRID}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert len(NEW) == 5 and set(decl) == NEW and len(decl) == 5
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_prime_cmux.h"]
    for name in ("cntt.h", "cntt_ext.h", "cntt_prime_pbs.h", "cntt_prime_cmux.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert "cntt_prime_cbs.h" not in other and not (NEW & set(declarations(os.path.join(ROOT, "include", name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_cmux_abi.py reads its unit: four kernels x two word types,
    none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_cbs.o")
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
    assert len(seen) == 8, seen
    for word in ("Ij", "Im"):
        for kernel in ("22prime_cbs_setup_kernel", "24prime_cbs_extract_kernel", "19prime_cbs_ks_kernel", "20prime_cbs_sum_kernel"):
            tag = "4cntt%s%sE" % (kernel, word)
            assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_are_the_formula_of_the_header(mod, p, wb):
    for n, k in ((32, 1), (1024, 1), (256, 3), (2048, 2), (64, 0)):
        plan = mod.Plan.try_new(n, p)
        for L, pl, Lk, Lc, batch in ((0, 1, 1, 1, 1), (3, 2, 3, 2, 3), (630, 3, 1, 2, 10), (700, 1, 2, 4, 64), (5, 2, 1, 1, 8195), (1, 1, 1, 1, 0)):
            assert plan.circuit_bootstrap_workspace_bytes(L, k, pl, Lk, Lc, batch) == cbs_workspace_bytes(n, wb, L, k, pl, Lk, Lc, batch), (n, k, L, batch)
    assert getattr(cntt.lib(), "cntt_prime%d_circuit_bootstrap_workspace_bytes" % (8 * wb))(None, 3, 1, 2, 2, 2, 3) == 0


def test_grid_rule():
    """one workgroup per work item up to 8 per CU of a 256-CU part; neither the size nor the word enters"""
    g = cntt.lib().cntt_prime_cbs_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    for items in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 14):
            for w in (4, 8):
                assert g(items, logn, w) == grid(items, logn, w), (items, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, L = 32, 1, 2, 3
PBS, KS, CBS = (4, 2), (5, 3), (6, 2)
POISON = 7
LIN = K * N
R = (LIN + 1) * KS[1]


class Case:
    """Valid host arguments at n = 32: k = 1, L = 3, 2 bits, gadgets (4, 2), (5, 3), (6, 2); the output filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.lwe = np.arange(B * (L + 1), dtype=self.dtype)
        self.bsk = np.zeros(L * (K + 1) * PBS[1] * (K + 1) * N, dtype=self.dtype)
        self.fk = np.zeros((K + 1) * R * (K + 1) * N, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * CBS[1] * (K + 1) * N, POISON, dtype=self.dtype)
        self.ws = np.zeros(self.plan.circuit_bootstrap_workspace_bytes(L, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)

    def call(self, plan="own", out="own", lwe="own", bsk="own", fk="own", lwe_dim=L, k=K, pbs=PBS, ks=KS, cbs=CBS, batch=B, ws=None, ws_bytes=None):
        a = {name: (getattr(self, name) if isinstance(v, str) else v) for name, v in dict(out=out, lwe=lwe, bsk=bsk, fk=fk).items()}
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        fn = getattr(cntt.lib(), "cntt_prime%d_circuit_bootstrap_batch" % self.bits)
        return fn(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), ptr(a["bsk"]), ptr(a["fk"]), lwe_dim, k, pbs[0], pbs[1],
                  ks[0], ks[1], cbs[0], cbs[1], batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all())


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_every_invalid_argument_is_refused(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(1 << 16, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    for kw, word in [
            (dict(plan=None), "plan"),
            (dict(pbs=(0, 2)), "pbs_base_log is 0"), (dict(pbs=(4, 0)), "pbs_levels is 0"), (dict(pbs=(W, 2)), "pbs_base_log * pbs_levels"),
            (dict(ks=(0, 2)), "ks_base_log is 0"), (dict(ks=(4, 0)), "ks_levels is 0"), (dict(ks=(W // 3 + 1, 3)), "ks_base_log * ks_levels"),
            (dict(ks=(32, 1)), "ks_base_log = 32 is above 31") if W >= 32 else (dict(ks=(W + 1, 1)), "exceeds the bit length"),
            (dict(cbs=(0, 2)), "cbs_base_log is 0"), (dict(cbs=(4, 0)), "cbs_levels is 0"), (dict(cbs=(W // 2 + 1, 2)), "cbs_base_log * cbs_levels"),
            (dict(k=(1 << 32) - 1), "glwe_dim"), (dict(k=(1 << 64) - 1), "glwe_dim"),
            (dict(k=1 << 27), "2^32 key rows"), (dict(ks=(1, 30), k=1 << 23), "2^32 key rows"),
            (dict(batch=(1 << 32) // (CBS[1] * (K + 1) * PBS[1]) + 1), "2^32"), (dict(batch=1 << 63), "2^32"),
            (dict(lwe_dim=1 << 60), "2^63 bytes"), (dict(batch=1, k=1 << 20), "2^63 bytes"),     # the launch bounds pass, the keys do not fit
            (dict(out=None), "ggsw_ntt_out is NULL"), (dict(lwe=None), "lwe_in is NULL"), (dict(bsk=None), "bsk_ntt is NULL"),
            (dict(fk=None), "fpksk_ntt is NULL"),
            (dict(out=out_in_big, lwe=big[8:8 + c.lwe.size]), "ggsw_ntt_out overlaps lwe_in"),
            (dict(out=out_in_big, bsk=big[8:8 + c.bsk.size]), "ggsw_ntt_out overlaps bsk_ntt"),
            (dict(out=out_in_big, fk=big[8:8 + c.fk.size]), "ggsw_ntt_out overlaps fpksk_ntt"),
            (dict(out=out_in_big, ws=ws_in_big), "ggsw_ntt_out overlaps workspace"),
            (dict(lwe=big[16:16 + c.lwe.size], ws=ws_in_big), "workspace overlaps lwe_in"),
            (dict(bsk=big[:c.bsk.size], ws=ws_in_big), "workspace overlaps bsk_ntt"),
            (dict(fk=big[:c.fk.size], ws=ws_in_big), "workspace overlaps fpksk_ntt"),
            (dict(out=Raw(c.out.ctypes.data + w // 2)), "ggsw_ntt_out is not"), (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"),
            (dict(bsk=Raw(c.bsk.ctypes.data + 1)), "bsk_ntt is not"), (dict(fk=Raw(c.fk.ctypes.data + w // 2)), "fpksk_ntt is not"),
            (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
            (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=256), "workspace_bytes")]:
        assert c.call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_lwe_dim_zero_is_valid(bits, p):
    c = Case(bits, p)
    fn = getattr(cntt.lib(), "cntt_prime%d_circuit_bootstrap_batch" % bits)
    assert fn(c.plan._h, None, None, None, None, L, K, 4, 2, 5, 3, 6, 2, 0, None, 0, 0, None) == 0
    assert c.call(batch=0) == 0 and c.untouched()
    # lwe_dim = 0 with a NULL bootstrapping key passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    ws = np.zeros(c.plan.circuit_bootstrap_workspace_bytes(0, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)
    assert c.call(lwe_dim=0, bsk=None, lwe=c.lwe[:B], out=np.zeros(c.out.size, dtype=c.dtype), ws=ws) != EINVAL
    # every gadget at the whole bit length, ks_base_log at 31, k = 0
    W = wbits(p)
    out = np.zeros(B * 1 * N, dtype=c.dtype)
    assert c.call(k=0, pbs=(W, 1), ks=(min(31, W), 1), cbs=(W, 1), bsk=np.zeros(L * N, dtype=c.dtype), fk=np.zeros(N, dtype=c.dtype), out=out) != EINVAL


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    good = (c.out, c.lwe, c.bsk, c.fk, L, K) + PBS + KS + CBS
    for i, bad in [(0, c.out[:-N]), (1, c.lwe[:-1]), (2, c.bsk[:-N]), (3, c.fk[:-N]), (2, None), (4, -1), (5, -1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0),
                   (11, 0), (11, 3)]:
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
@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_of_two_wrong_arguments_the_earlier_check_answers(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(1 << 16, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    for kw, word in [
            (dict(plan=None, pbs=(0, 2)), "plan is NULL"),
            (dict(pbs=(0, 2), ks=(0, 2)), "pbs_base_log is 0"), (dict(pbs=(4, 0), cbs=(0, 2)), "pbs_levels is 0"),
            (dict(ks=(W // 3 + 1, 3), cbs=(4, 0)), "ks_base_log * ks_levels"),
            (dict(ks=(32, 1), cbs=(4, 0)), "ks_base_log = 32 is above 31") if W >= 32 else (dict(ks=(W + 1, 1), cbs=(4, 0)), "exceeds the bit length"),
            (dict(cbs=(W // 2 + 1, 2), k=(1 << 32) - 1), "cbs_base_log * cbs_levels"),
            (dict(k=(1 << 32) - 1, batch=1 << 63), "glwe_dim too large"),
            (dict(k=1 << 27, batch=1 << 63), "2^32 key rows"),
            (dict(batch=1 << 32, lwe_dim=1 << 60), "too large for one launch"),
            (dict(lwe_dim=1 << 60, out=None), "2^63 bytes"),
            (dict(out=None, lwe=None), "ggsw_ntt_out is NULL"),
            (dict(lwe=None, fk=None), "lwe_in is NULL"), (dict(bsk=None, fk=None), "bsk_ntt is NULL"),
            (dict(fk=None, ws=c.ws, ws_bytes=c.ws.nbytes - 1), "fpksk_ntt is NULL"),
            (dict(out=out_in_big, ws=ws_in_big, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
            (dict(lwe=Raw(c.lwe.ctypes.data + 1), out=out_in_big, ws=ws_in_big), "lwe_in is not")]:
        assert c.call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw
