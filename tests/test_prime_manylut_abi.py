"""C ABI of the prime plans' many-LUT bootstrap and one-rotation circuit bootstrap (include/cntt_prime_manylut.h): the header is plain
C11 on its own and includes cntt_prime_cbs.h only, its names are the five per word width, none of them leaks into the older headers,
all are exported, every CNTT_EINVAL case is refused on host buffers by the argument checks that precede any device call (output poison
intact, argument named), the workspace size is the header's formula, the Python wrappers panic on bad shapes, and the code object of the
new unit has its ten kernels without scratch or spills.  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from prime_manylut_model import HEADER, cbs_manylut_workspace_bytes
from test_prime_automorphism_abi import Raw, declarations, err, ptr
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["lwe_modswitch_manylut_batch", "sample_extract_many_batch", "bootstrap_manylut_batch", "circuit_bootstrap_manylut_batch",
         "circuit_bootstrap_manylut_workspace_bytes"]
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert len(NEW) == 10 and set(decl) == NEW and len(decl) == 10
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_prime_cbs.h"]
    for name in ("cntt.h", "cntt_ext.h", "cntt_prime_pbs.h", "cntt_prime_cmux.h", "cntt_prime_cbs.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert "cntt_prime_manylut.h" not in other and not (NEW & set(declarations(os.path.join(ROOT, "include", name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_prime_cbs_abi.py reads its unit: the modulus switch with and without
    the circuit bootstrap's set-up, the extraction of several indices with and without streaming stores, the extraction + digits of the
    circuit bootstrap, each on two word types: ten kernels, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_manylut.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "ml.fat"), str(tmp_path / "ml.co")
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
    assert len(seen) == 10, seen
    for word in ("Ij", "Im"):
        for kernel, variants in (("30prime_modswitch_manylut_kernel", ("Lb0E", "Lb1E")), ("32prime_sample_extract_many_kernel", ("Lb0E", "Lb1E")),
                                 ("32prime_cbs_manylut_extract_kernel", ("",))):
            for v in variants:
                tag = "4cntt%s%s%sE" % (kernel, word, v)
                assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_are_the_formula_of_the_header(mod, p, wb):
    """the shape list of tests/test_prime_cbs_abi.py"""
    for n, k in ((32, 1), (1024, 1), (256, 3), (2048, 2), (64, 0)):
        plan = mod.Plan.try_new(n, p)
        for L, pl, Lk, Lc, batch in ((0, 1, 1, 1, 1), (3, 2, 3, 2, 3), (630, 3, 1, 2, 10), (700, 1, 2, 4, 64), (5, 2, 1, 1, 8195), (1, 1, 1, 1, 0)):
            assert plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pl, Lk, Lc, batch) == \
                cbs_manylut_workspace_bytes(n, wb, L, k, pl, Lk, Lc, batch), (n, k, L, batch)
    assert getattr(cntt.lib(), "cntt_prime%d_circuit_bootstrap_manylut_workspace_bytes" % (8 * wb))(None, 3, 1, 2, 2, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, LOGN, K, B, L = 32, 5, 1, 2, 3
PBS, KS, CBS, T = (4, 2), (5, 3), (6, 2), 2
POISON = 7
R = (K * N + 1) * KS[1]


class Case:
    """Valid host arguments at n = 32: k = 1, L = 3, 2 elements, gadgets (4, 2), (5, 3), (6, 2), t = 2, 3 tables; every output filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.lwe = np.arange(B * (L + 1), dtype=self.dtype)
        self.bsk = np.zeros(L * (K + 1) * PBS[1] * (K + 1) * N, dtype=self.dtype)
        self.fk = np.zeros((K + 1) * R * (K + 1) * N, dtype=self.dtype)
        self.lut = np.zeros((K + 1) * N, dtype=self.dtype)
        self.glwe = np.zeros(B * (K + 1) * N, dtype=self.dtype)
        self.rot = np.full(B * (L + 1), POISON, dtype=np.uint32)
        self.ext = np.full(B * 3 * (K * N + 1), POISON, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * CBS[1] * (K + 1) * N, POISON, dtype=self.dtype)
        self.ws = np.zeros(self.plan.circuit_bootstrap_manylut_workspace_bytes(L, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)
        self.pws = np.zeros(self.plan.pbs_workspace_bytes(L, K, PBS[1], B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def own(self, **kw):
        return {name: (getattr(self, name) if isinstance(v, str) else v) for name, v in kw.items()}

    def modswitch(self, plan="own", rot="own", lwe="own", lwe_dim=L, t=T, batch=B):
        a = self.own(rot=rot, lwe=lwe)
        return self.fn("lwe_modswitch_manylut_batch")(self.plan._h if plan == "own" else None, ptr(a["rot"]), ptr(a["lwe"]), lwe_dim, t, batch, 0, None)

    def extract(self, plan="own", ext="own", glwe="own", k=K, count=3, batch=B):
        a = self.own(ext=ext, glwe=glwe)
        return self.fn("sample_extract_many_batch")(self.plan._h if plan == "own" else None, ptr(a["ext"]), ptr(a["glwe"]), k, count, batch, 0, None)

    def boot(self, plan="own", ext="own", lwe="own", lut="own", bsk="own", lwe_dim=L, k=K, pbs=PBS, t=T, count=3, batch=B, ws=None, ws_bytes=None):
        a = self.own(ext=ext, lwe=lwe, lut=lut, bsk=bsk)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("bootstrap_manylut_batch")(self.plan._h if plan == "own" else None, ptr(a["ext"]), ptr(a["lwe"]), ptr(a["lut"]), 0, ptr(a["bsk"]),
                                                  lwe_dim, k, pbs[0], pbs[1], t, count, batch, ptr(ws), wsb, 0, None)

    def cbs(self, plan="own", out="own", lwe="own", bsk="own", fk="own", lwe_dim=L, k=K, pbs=PBS, ks=KS, cbs=CBS, t=T, batch=B, ws=None, ws_bytes=None):
        a = self.own(out=out, lwe=lwe, bsk=bsk, fk=fk)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("circuit_bootstrap_manylut_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), ptr(a["bsk"]),
                                                          ptr(a["fk"]), lwe_dim, k, pbs[0], pbs[1], ks[0], ks[1], cbs[0], cbs[1], t, batch, ptr(ws), wsb,
                                                          0, None)

    def untouched(self):
        return bool((self.out == POISON).all() and (self.ext == POISON).all() and (self.rot == POISON).all())


@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_every_invalid_argument_is_refused(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(1 << 16, POISON, dtype=c.dtype)
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    pws_in_big = big.view(np.uint8)[16 * w:16 * w + c.pws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    cases = [
        # the coarse modulus switch
        (c.modswitch, dict(plan=None), "plan"), (c.modswitch, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"),
        (c.modswitch, dict(rot=None), "rot_t is NULL"), (c.modswitch, dict(lwe=None), "lwe is NULL"),
        (c.modswitch, dict(rot=big.view(np.uint32)[:c.rot.size], lwe=big[:c.lwe.size]), "rot_t overlaps lwe"),
        (c.modswitch, dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe is not"),
        # the extraction of several indices
        (c.extract, dict(plan=None), "plan"), (c.extract, dict(count=0), "count = 0"), (c.extract, dict(count=N + 1), "count = 33"),
        (c.extract, dict(ext=None), "lwe_out is NULL"), (c.extract, dict(glwe=None), "glwe is NULL"),
        (c.extract, dict(ext=big[:c.ext.size], glwe=big[8:8 + c.glwe.size]), "lwe_out overlaps glwe"),
        (c.extract, dict(k=1 << 62), "2^63 bytes"),
        # the many-LUT bootstrap
        (c.boot, dict(plan=None), "plan"), (c.boot, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"),
        (c.boot, dict(count=0), "lut_count = 0"), (c.boot, dict(count=5), "lut_count = 5"), (c.boot, dict(t=0, count=2), "lut_count = 2"),
        (c.boot, dict(pbs=(0, 2)), "base_log is 0"), (c.boot, dict(pbs=(4, 0)), "levels is 0"), (c.boot, dict(pbs=(W, 2)), "base_log * levels"),
        (c.boot, dict(ext=None), "lwe_out is NULL"), (c.boot, dict(lwe=None), "lwe_in is NULL"), (c.boot, dict(lut=None), "lut is NULL"),
        (c.boot, dict(bsk=None), "bsk_ntt is NULL"),
        (c.boot, dict(ext=big[:c.ext.size], lwe=big[8:8 + c.lwe.size]), "lwe_out overlaps lwe_in"),
        (c.boot, dict(ext=big[:c.ext.size], lut=big[8:8 + c.lut.size]), "lwe_out overlaps lut"),
        (c.boot, dict(ext=big[:c.ext.size], ws=pws_in_big), "lwe_out overlaps workspace"),
        (c.boot, dict(lut=big[16:16 + c.lut.size], ws=pws_in_big), "workspace overlaps lut"),
        (c.boot, dict(ws=c.pws, ws_bytes=c.pws.nbytes - 1), "workspace_bytes"),
        (c.boot, dict(lwe_dim=1 << 60), "2^63 bytes"),
        # the one-rotation circuit bootstrap: its own cases, then the inherited ones
        (c.cbs, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"), (c.cbs, dict(t=LOGN), "exceeds ntt_size / 2"),
        (c.cbs, dict(cbs=(6, 5)), "cbs_levels = 5 exceeds 2^log_lut_count = 4"), (c.cbs, dict(t=0), "cbs_levels = 2 exceeds 2^log_lut_count = 1"),
        (c.cbs, dict(plan=None), "plan"),
        (c.cbs, dict(pbs=(0, 2)), "pbs_base_log is 0"), (c.cbs, dict(pbs=(4, 0)), "pbs_levels is 0"), (c.cbs, dict(pbs=(W, 2)), "pbs_base_log * pbs_levels"),
        (c.cbs, dict(ks=(0, 2)), "ks_base_log is 0"), (c.cbs, dict(ks=(4, 0)), "ks_levels is 0"), (c.cbs, dict(ks=(W // 3 + 1, 3)), "ks_base_log * ks_levels"),
        (c.cbs, dict(ks=(32, 1)), "ks_base_log = 32 is above 31") if W >= 32 else (c.cbs, dict(ks=(W + 1, 1)), "exceeds the bit length"),
        (c.cbs, dict(cbs=(0, 2)), "cbs_base_log is 0"), (c.cbs, dict(cbs=(4, 0)), "cbs_levels is 0"), (c.cbs, dict(cbs=(W // 2 + 1, 2)), "cbs_base_log * cbs_levels"),
        (c.cbs, dict(k=(1 << 32) - 1), "glwe_dim"), (c.cbs, dict(k=1 << 27), "2^32 key rows"),
        (c.cbs, dict(batch=(1 << 32) // ((K + 1) * PBS[1])), "batch * (glwe_dim + 1) * pbs_levels"), (c.cbs, dict(batch=1 << 63), "2^32"),
        (c.cbs, dict(lwe_dim=1 << 60), "2^63 bytes"), (c.cbs, dict(batch=1, k=1 << 20), "2^63 bytes"),
        (c.cbs, dict(out=None), "ggsw_ntt_out is NULL"), (c.cbs, dict(lwe=None), "lwe_in is NULL"), (c.cbs, dict(bsk=None), "bsk_ntt is NULL"),
        (c.cbs, dict(fk=None), "fpksk_ntt is NULL"),
        (c.cbs, dict(out=big[:c.out.size], lwe=big[8:8 + c.lwe.size]), "ggsw_ntt_out overlaps lwe_in"),
        (c.cbs, dict(out=big[:c.out.size], fk=big[8:8 + c.fk.size]), "ggsw_ntt_out overlaps fpksk_ntt"),
        (c.cbs, dict(out=big[:c.out.size], ws=ws_in_big), "ggsw_ntt_out overlaps workspace"),
        (c.cbs, dict(bsk=big[:c.bsk.size], ws=ws_in_big), "workspace overlaps bsk_ntt"),
        (c.cbs, dict(out=Raw(c.out.ctypes.data + w // 2)), "ggsw_ntt_out is not"), (c.cbs, dict(fk=Raw(c.fk.ctypes.data + w // 2)), "fpksk_ntt is not"),
        (c.cbs, dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        (c.cbs, dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (c.cbs, dict(ws=c.ws, ws_bytes=256), "workspace_bytes")]
    for call, kw, word in cases:
        assert call(**kw) == EINVAL, (call.__name__, kw)
        assert word in err(), (call.__name__, kw, err())
        assert c.untouched() and (big == POISON).all(), (call.__name__, kw)


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_the_edges_of_the_ranges_are_valid(bits, p):
    c = Case(bits, p)
    assert c.modswitch(batch=0) == 0 and c.extract(batch=0) == 0 and c.boot(batch=0) == 0 and c.cbs(batch=0) == 0 and c.untouched()
    # what passes the argument checks needs a device: any status but CNTT_EINVAL
    assert c.modswitch(t=LOGN, rot=np.zeros(c.rot.size, dtype=np.uint32)) != EINVAL
    assert c.extract(count=N, ext=np.zeros(B * N * (K * N + 1), dtype=c.dtype)) != EINVAL
    assert c.boot(t=LOGN, count=N, ext=np.zeros(B * N * (K * N + 1), dtype=c.dtype)) != EINVAL
    assert c.cbs(t=LOGN - 1, cbs=(1, N // 2), out=np.zeros(B * (K + 1) * (N // 2) * (K + 1) * N, dtype=c.dtype)) != EINVAL
    assert c.cbs(t=1, out=np.zeros(c.out.size, dtype=c.dtype), ws=c.ws) != EINVAL


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    for args in ((c.rot[:-1], c.lwe, L, T), (c.rot, c.lwe, L, -1), (c.rot, c.lwe, 4, T), (c.rot.astype(np.uint64), c.lwe, L, T)):
        with pytest.raises((Panic, TypeError)):
            pl.lwe_modswitch_manylut_batch(*args)
    for args in ((c.ext[:-1], c.glwe, K, 3), (c.ext, c.glwe, K, 0), (c.ext, c.glwe[:-1], K, 3), (c.ext, c.glwe, K, 2)):
        with pytest.raises((Panic, TypeError)):
            pl.sample_extract_many_batch(*args)
    good = (c.ext, c.lwe, c.lut, c.bsk, L, K) + PBS + (T, 3)
    for i, bad in [(0, c.ext[:-1]), (1, c.lwe[:-1]), (2, c.lut[:-1]), (3, c.bsk[:-N]), (4, -1), (6, 0), (7, 0), (8, -1), (9, 0), (9, 2)]:
        args = list(good)
        args[i] = bad
        with pytest.raises((Panic, TypeError)):
            pl.bootstrap_manylut_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: lut_count above 2^t
        pl.bootstrap_manylut_batch(np.zeros(B * 5 * (K * N + 1), dtype=c.dtype), c.lwe, c.lut, c.bsk, L, K, *PBS, T, 5)
    good = (c.out, c.lwe, c.bsk, c.fk, L, K) + PBS + KS + CBS + (T,)
    for i, bad in [(0, c.out[:-N]), (1, c.lwe[:-1]), (2, c.bsk[:-N]), (3, c.fk[:-N]), (2, None), (4, -1), (5, -1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0),
                   (11, 0), (11, 3), (12, -1)]:
        args = list(good)
        args[i] = bad
        with pytest.raises((Panic, TypeError)):
            pl.circuit_bootstrap_manylut_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.circuit_bootstrap_manylut_batch(*good, workspace=c.ws[:255])
    with pytest.raises(Panic):                                                 # through the C checks: the levels do not fit the table
        pl.circuit_bootstrap_manylut_batch(*good[:-1], 0)
    for args in ((L, K, 2, 3, 2, -1), (L, K, 0, 3, 2, 1), (L, K, 2, 0, 2, 1), (L, K, 2, 3, 0, 1), (-1, K, 2, 3, 2, 1)):
        with pytest.raises(Panic):
            pl.circuit_bootstrap_manylut_workspace_bytes(*args)
    assert c.untouched()


# -- the order of the refusals: of two wrong arguments the earlier check answers ---------------------------------------------------
@pytest.mark.parametrize("bits,p", [(64, P62), (64, PM64), (32, P30), (32, P32)])
def test_of_two_wrong_arguments_the_earlier_check_answers(bits, p):
    c = Case(bits, p)
    W = wbits(p)
    w = c.dtype().itemsize
    big = np.full(1 << 16, POISON, dtype=c.dtype)
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    pws_in_big = big.view(np.uint8)[16 * w:16 * w + c.pws.nbytes]
    cases = [
        (c.modswitch, dict(t=LOGN + 1, lwe_dim=1 << 61), "log_lut_count = 6 exceeds"), (c.modswitch, dict(lwe_dim=1 << 61, rot=None), "2^63 bytes"),
        (c.modswitch, dict(rot=None, lwe=None), "rot_t is NULL"),
        (c.extract, dict(count=0, k=1 << 62), "count = 0"), (c.extract, dict(k=1 << 62, ext=None), "2^63 bytes"),
        (c.extract, dict(ext=None, glwe=None), "lwe_out is NULL"),
        # the many-LUT bootstrap
        (c.boot, dict(t=LOGN + 1, count=0), "log_lut_count = 6 exceeds"),
        (c.boot, dict(count=5, pbs=(0, 2)), "lut_count = 5"), (c.boot, dict(count=0, pbs=(0, 2)), "lut_count = 0"),
        (c.boot, dict(count=5, lwe_dim=1 << 60), "lut_count = 5"), (c.boot, dict(lwe_dim=1 << 60, pbs=(0, 2)), "2^63 bytes"),
        (c.boot, dict(pbs=(4, 0), bsk=None), "levels is 0"), (c.boot, dict(bsk=None, ext=None), "bsk_ntt is NULL"),
        (c.boot, dict(ws=c.pws, ws_bytes=c.pws.nbytes - 1, ext=None), "workspace_bytes"), (c.boot, dict(ext=None, lwe=None), "lwe_out is NULL"),
        (c.boot, dict(lut=None, ext=big[:c.ext.size], ws=pws_in_big), "lut is NULL"),
        # the one-rotation circuit bootstrap
        (c.cbs, dict(plan=None, pbs=(0, 2)), "plan is NULL"),
        (c.cbs, dict(pbs=(0, 2), ks=(0, 2)), "pbs_base_log is 0"),
        (c.cbs, dict(ks=(32, 1), cbs=(4, 0)), "ks_base_log = 32 is above 31") if W >= 32 else (c.cbs, dict(ks=(W + 1, 1), cbs=(4, 0)), "exceeds the bit length"),
        (c.cbs, dict(cbs=(W // 2 + 1, 2), t=LOGN + 1), "cbs_base_log * cbs_levels"),
        (c.cbs, dict(t=LOGN + 1, cbs=(1, W)), "log_lut_count = 6 exceeds"),
        (c.cbs, dict(t=LOGN, cbs=(1, 33)), "exceeds ntt_size / 2") if W >= 33 else (c.cbs, dict(t=LOGN, k=(1 << 32) - 1), "exceeds ntt_size / 2"),
        (c.cbs, dict(t=0, k=(1 << 32) - 1), "cbs_levels = 2 exceeds 2^log_lut_count = 1"),
        (c.cbs, dict(k=(1 << 32) - 1, batch=1 << 63), "glwe_dim too large"),
        (c.cbs, dict(k=1 << 27, batch=1 << 63), "2^32 key rows"),
        (c.cbs, dict(batch=1 << 32, lwe_dim=1 << 60), "too large for one launch"),
        (c.cbs, dict(lwe_dim=1 << 60, out=None), "2^63 bytes"),
        (c.cbs, dict(out=None, lwe=None), "ggsw_ntt_out is NULL"),
        (c.cbs, dict(lwe=None, fk=None), "lwe_in is NULL"), (c.cbs, dict(bsk=None, fk=None), "bsk_ntt is NULL"),
        (c.cbs, dict(fk=None, ws=c.ws, ws_bytes=c.ws.nbytes - 1), "fpksk_ntt is NULL"),
        (c.cbs, dict(out=big[:c.out.size], ws=ws_in_big, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
        (c.cbs, dict(lwe=Raw(c.lwe.ctypes.data + 1), out=big[:c.out.size], ws=ws_in_big), "lwe_in is not")]
    for call, kw, word in cases:
        assert call(**kw) == EINVAL, (call.__name__, kw)
        assert word in err(), (call.__name__, kw, err())
        assert c.untouched() and (big == POISON).all(), (call.__name__, kw)
