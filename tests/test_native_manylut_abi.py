"""C ABI of the native plans' many-LUT bootstrap and one-rotation circuit bootstrap (include/cntt_manylut.h): the header is plain C11 on
its own and includes cntt_cbs.h only, its names are the five it declares, all are exported, every CNTT_EINVAL case is refused on host
buffers by the argument checks that precede any device call (output poison intact, argument named), the binary kinds are refused by the
circuit bootstrap and accepted by the other three calls, the workspace size is the header's formula, the Python wrappers panic on bad
shapes, and the code object of the new unit has its fifteen kernels without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary32, native_binary64, native_binary128
from concrete_ntt_amd._lib import EINVAL, Panic
from native_manylut_model import HEADER, cbs_manylut_workspace_bytes
from test_native_cmux_abi import Raw, declarations, err, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CALLS = ["lwe_modswitch_manylut_batch", "sample_extract_many_batch", "bootstrap_manylut_batch", "circuit_bootstrap_manylut_batch",
         "circuit_bootstrap_manylut_workspace_bytes"]
NEW = {"cntt_native_" + c for c in CALLS}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert set(decl) == NEW and len(decl) == 5
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_cbs.h"]
    older = sorted(f for f in os.listdir(INC) if f.endswith(".h") and f != "cntt_manylut.h")
    assert "cntt.h" in older and "cntt_ext.h" in older and "cntt_cbs.h" in older and "cntt_prime_manylut.h" in older
    for name in older:
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, name)).read(), flags=re.S)
        assert "cntt_manylut.h" not in other, name
        if name.startswith("cntt") and "hpp" not in name:
            assert not (NEW & set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", other))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_native_cbs_abi.py reads its unit: 2 + 2 + 1 kernels x three word
    types, none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_manylut.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "manylut.fat"), str(tmp_path / "manylut.co")
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
    assert len(seen) == 15, seen
    for word in ("Ij", "Im", "INS_7Word128E"):
        for kernel in ("31native_modswitch_manylut_kernel", "33native_sample_extract_many_kernel"):
            for flag in ("Lb0E", "Lb1E"):
                tag = "4cntt%s%s%sE" % (kernel, word, flag)
                assert sum(tag in s for s in seen) == 1, (tag, seen)
        tag = "4cntt33native_cbs_manylut_extract_kernel%sE" % word
        assert sum(tag in s for s in seen) == 1, (tag, seen)


@pytest.mark.parametrize("P", [native32.Plan32, native64.Plan32, native128.Plan32, native32.Plan52, native64.Plan52])
def test_workspace_bytes_are_the_formula_of_the_header(P):
    for n, k in ((32, 1), (1024, 1), (256, 3), (2048, 2), (64, 0)):
        plan = P.try_new(n)
        for L, pl, Lk, Lc, batch in ((0, 1, 1, 1, 1), (3, 2, 3, 2, 3), (630, 3, 1, 2, 10), (700, 1, 2, 4, 64), (5, 2, 1, 1, 8195), (1, 1, 1, 1, 0)):
            assert plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pl, Lk, Lc, batch) == \
                cbs_manylut_workspace_bytes(n, plan.WORD, L, k, pl, Lk, Lc, batch), (n, k, L, batch)
    assert cntt.lib().cntt_native_circuit_bootstrap_manylut_workspace_bytes(None, 3, 1, 2, 2, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, LOGN, K, B, L = 32, 5, 1, 2, 3
PBS, KS, CBS, T = (4, 2), (5, 3), (6, 2), 2
POISON = 7
R = (K * N + 1) * KS[1]


class Case:
    """Valid host arguments at n = 32: k = 1, L = 3, 2 elements, gadgets (4, 2), (5, 3), (6, 2), t = 2, 3 tables; every output filled
    with 7."""

    def __init__(self, P):
        self.plan = P.try_new(N)
        self.dtype, self.pw = self.plan.word_dtype, (2 if self.plan.WORD == 16 else 1)       # array items per word
        self.pe = N * self.pw
        self.np = self.plan.NPRIMES
        self.lwe = np.arange(B * (L + 1) * self.pw, dtype=self.dtype)
        self.bsk = [np.zeros(L * (K + 1) * PBS[1] * (K + 1) * N, dtype=self.plan.res_dtype) for _ in range(self.np)]
        self.fk = np.zeros((K + 1) * R * (K + 1) * self.pe, dtype=self.dtype)
        self.lut = np.zeros((K + 1) * self.pe, dtype=self.dtype)
        self.glwe = np.zeros(B * (K + 1) * self.pe, dtype=self.dtype)
        self.rot = np.full(B * (L + 1), POISON, dtype=np.uint32)
        self.ext = np.full(B * 3 * (K * N + 1) * self.pw, POISON, dtype=self.dtype)
        self.out = [np.full(B * (K + 1) * CBS[1] * (K + 1) * N, POISON, dtype=self.plan.res_dtype) for _ in range(self.np)]
        self.ws = np.zeros(self.plan.circuit_bootstrap_manylut_workspace_bytes(L, K, PBS[1], KS[1], CBS[1], B), dtype=np.uint8)
        self.pws = np.zeros(self.plan.pbs_workspace_bytes(L, K, PBS[1], B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_native_" + name)

    def planes(self, ps):
        if ps is None:
            return None
        return (ctypes.c_void_p * self.np)(*[None if p is None else ptr(p) for p in ps])

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
        return self.fn("bootstrap_manylut_batch")(self.plan._h if plan == "own" else None, ptr(a["ext"]), ptr(a["lwe"]), ptr(a["lut"]), 0,
                                                  self.planes(a["bsk"]), lwe_dim, k, pbs[0], pbs[1], t, count, batch, ptr(ws), wsb, 0, None)

    def cbs(self, plan="own", out="own", lwe="own", bsk="own", fk="own", lwe_dim=L, k=K, pbs=PBS, ks=KS, cbs=CBS, t=T, batch=B, ws=None, ws_bytes=None):
        a = self.own(out=out, lwe=lwe, bsk=bsk, fk=fk)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("circuit_bootstrap_manylut_batch")(self.plan._h if plan == "own" else None, self.planes(a["out"]), ptr(a["lwe"]),
                                                          self.planes(a["bsk"]), ptr(a["fk"]), lwe_dim, k, pbs[0], pbs[1], ks[0], ks[1], cbs[0],
                                                          cbs[1], t, batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool(all((o == POISON).all() for o in self.out) and (self.ext == POISON).all() and (self.rot == POISON).all())


def with_plane(planes, i, p):
    return [p if j == i else x for j, x in enumerate(planes)]


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_every_invalid_argument_is_refused(P):
    c = Case(P)
    W, rb, pw = 8 * c.plan.WORD, c.plan.RES, c.pw
    big = np.full(1 << 16, POISON, dtype=np.uint64)
    bigr, bigw = big.view(c.plan.res_dtype), big.view(c.dtype)
    out_in_big = bigr[:c.out[0].size]
    ws_in_big = big.view(np.uint8)[256:256 + c.ws.nbytes]
    pws_in_big = big.view(np.uint8)[256:256 + c.pws.nbytes]
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                           # an address that is 4 mod 16
    last = c.np - 1
    cases = [
        # the coarse modulus switch
        (c.modswitch, dict(plan=None), "plan"), (c.modswitch, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"),
        (c.modswitch, dict(rot=None), "rot_t is NULL"), (c.modswitch, dict(lwe=None), "lwe is NULL"),
        (c.modswitch, dict(rot=big.view(np.uint32)[:c.rot.size], lwe=bigw[:c.lwe.size]), "rot_t overlaps lwe"),
        (c.modswitch, dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe is not"), (c.modswitch, dict(lwe_dim=1 << 61), "2^63 bytes"),
        # the extraction of several indices
        (c.extract, dict(plan=None), "plan"), (c.extract, dict(count=0), "count = 0"), (c.extract, dict(count=N + 1), "count = 33"),
        (c.extract, dict(ext=None), "lwe_out is NULL"), (c.extract, dict(glwe=None), "glwe is NULL"),
        (c.extract, dict(ext=bigw[:c.ext.size], glwe=bigw[8 * pw:8 * pw + c.glwe.size]), "lwe_out overlaps glwe"),
        (c.extract, dict(k=1 << 62), "2^63 bytes"), (c.extract, dict(glwe=Raw(c.glwe.ctypes.data + 1)), "glwe is not"),
        # the many-LUT bootstrap
        (c.boot, dict(plan=None), "plan"), (c.boot, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"),
        (c.boot, dict(count=0), "lut_count = 0"), (c.boot, dict(count=5), "lut_count = 5"), (c.boot, dict(t=0, count=2), "lut_count = 2"),
        (c.boot, dict(pbs=(0, 2)), "base_log is 0"), (c.boot, dict(pbs=(4, 0)), "levels is 0"), (c.boot, dict(pbs=(W, 2)), "base_log * levels"),
        (c.boot, dict(k=(1 << 32) - 1), "glwe_dim"), (c.boot, dict(k=c.plan.max_terms(), pbs=(4, 1)), "cntt_native_max_terms" if c.plan.max_terms() + 1 < 1 << 32 else "glwe_dim"),
        (c.boot, dict(ext=None), "lwe_out is NULL"), (c.boot, dict(lwe=None), "lwe_in is NULL"), (c.boot, dict(lut=None), "lut is NULL"),
        (c.boot, dict(bsk=None), "bsk_ntt is NULL"), (c.boot, dict(bsk=with_plane(c.bsk, last, None)), "bsk_ntt"),
        (c.boot, dict(ext=bigw[:c.ext.size], lwe=bigw[8 * pw:8 * pw + c.lwe.size]), "lwe_out overlaps lwe_in"),
        (c.boot, dict(ext=bigw[:c.ext.size], lut=bigw[8 * pw:8 * pw + c.lut.size]), "lwe_out overlaps lut"),
        (c.boot, dict(ext=bigw[:c.ext.size], bsk=with_plane(c.bsk, 0, bigr[16:16 + c.bsk[0].size])), "lwe_out overlaps bsk_ntt[0]"),
        (c.boot, dict(ext=bigw[:c.ext.size], ws=pws_in_big), "lwe_out overlaps workspace"),
        (c.boot, dict(lut=bigw[64 * pw:64 * pw + c.lut.size], ws=pws_in_big), "workspace overlaps lut"),
        (c.boot, dict(ws=c.pws, ws_bytes=c.pws.nbytes - 1), "workspace_bytes"),
        (c.boot, dict(lwe_dim=1 << 60), "2^63 bytes"),
        # the one-rotation circuit bootstrap: its own cases, then the inherited ones
        (c.cbs, dict(t=LOGN + 1), "log_lut_count = 6 exceeds"), (c.cbs, dict(t=LOGN), "exceeds ntt_size / 2"),
        (c.cbs, dict(cbs=(6, 5)), "cbs_levels = 5 exceeds 2^log_lut_count = 4"), (c.cbs, dict(t=0), "cbs_levels = 2 exceeds 2^log_lut_count = 1"),
        (c.cbs, dict(plan=None), "plan"),
        (c.cbs, dict(pbs=(0, 2)), "pbs_base_log is 0"), (c.cbs, dict(pbs=(4, 0)), "pbs_levels is 0"), (c.cbs, dict(pbs=(W, 2)), "pbs_base_log * pbs_levels"),
        (c.cbs, dict(ks=(0, 2)), "ks_base_log is 0"), (c.cbs, dict(ks=(4, 0)), "ks_levels is 0"), (c.cbs, dict(ks=(W // 3 + 1, 3)), "ks_base_log * ks_levels"),
        (c.cbs, dict(ks=(32, 1)), "ks_base_log = 32 is above 31"),
        (c.cbs, dict(cbs=(0, 2)), "cbs_base_log is 0"), (c.cbs, dict(cbs=(4, 0)), "cbs_levels is 0"), (c.cbs, dict(cbs=(W // 2 + 1, 2)), "cbs_base_log * cbs_levels"),
        (c.cbs, dict(cbs=(W // 2, 2)), "2 has no inverse mod 2^w"), (c.cbs, dict(cbs=(W, 1)), "2 has no inverse mod 2^w"),
        (c.cbs, dict(k=(1 << 32) - 1), "glwe_dim"), (c.cbs, dict(k=(1 << 64) - 1), "glwe_dim"),
        (c.cbs, dict(k=1 << 27, pbs=(4, 1), cbs=(6, 1), batch=1), "cntt_native_max_terms" if (1 << 27) + 1 > c.plan.max_terms() else "2^32 key rows"),
        (c.cbs, dict(batch=(1 << 32) // ((K + 1) * PBS[1])), "batch * (glwe_dim + 1) * pbs_levels"), (c.cbs, dict(batch=1 << 63), "2^32"),
        (c.cbs, dict(batch=1 << 29, k=7, pbs=(4, 1), cbs=(6, 1)), "2^46" if c.plan.max_terms() >= 8 else "cntt_native_max_terms"),
        (c.cbs, dict(lwe_dim=1 << 60), "2^63 bytes"),
        (c.cbs, dict(out=None), "ggsw_ntt_out is NULL"), (c.cbs, dict(out=with_plane(c.out, last, None)), "ggsw_ntt_out[%d]" % last),
        (c.cbs, dict(lwe=None), "lwe_in is NULL"), (c.cbs, dict(bsk=None), "bsk_ntt is NULL"), (c.cbs, dict(bsk=with_plane(c.bsk, 0, None)), "bsk_ntt[0]"),
        (c.cbs, dict(fk=None), "fpksk is NULL"),
        (c.cbs, dict(out=with_plane(c.out, 0, out_in_big), lwe=bigw[8 * pw:8 * pw + c.lwe.size]), "ggsw_ntt_out[0] overlaps lwe_in"),
        (c.cbs, dict(out=with_plane(c.out, last, out_in_big), bsk=with_plane(c.bsk, 0, bigr[16:16 + c.bsk[0].size])), "ggsw_ntt_out[%d] overlaps bsk_ntt[0]" % last),
        (c.cbs, dict(out=with_plane(c.out, 0, out_in_big), fk=bigw[:c.fk.size]), "ggsw_ntt_out[0] overlaps fpksk"),
        (c.cbs, dict(out=with_plane(c.out, 0, out_in_big), ws=ws_in_big), "ggsw_ntt_out[0] overlaps workspace"),
        (c.cbs, dict(fk=bigw[:c.fk.size], ws=ws_in_big), "workspace overlaps fpksk"),
        (c.cbs, dict(out=with_plane(c.out, 0, Raw(c.out[0].ctypes.data + rb // 2))), "ggsw_ntt_out[0] is not"),
        (c.cbs, dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"),
        (c.cbs, dict(fk=Raw(c.fk.ctypes.data + 8)), "fpksk is not 16-byte aligned"),
        (c.cbs, dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        (c.cbs, dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (c.cbs, dict(ws=c.ws, ws_bytes=256), "workspace_bytes")]
    for call, kw, word in cases:
        assert call(**kw) == EINVAL, (call.__name__, kw)
        assert word in err(), (call.__name__, kw, err())
        assert c.untouched() and (big == POISON).all(), (call.__name__, kw)


@pytest.mark.parametrize("P", [native_binary32.Plan32, native_binary64.Plan32, native_binary128.Plan32, native_binary32.Plan52, native_binary64.Plan52],
                         ids=["binary32", "binary64", "binary128", "binary32_plan52", "binary64_plan52"])
def test_the_binary_kinds_are_refused_by_the_circuit_bootstrap_and_accepted_elsewhere(P):
    c = Case(P)
    assert c.cbs() == EINVAL and "native_binary" in err() and "0/1 key words" in err(), err()
    assert c.cbs(batch=0) == EINVAL and c.untouched()
    with pytest.raises(Panic):
        c.plan.circuit_bootstrap_manylut_batch(c.out, c.lwe, c.bsk, c.fk, L, K, *PBS, *KS, *CBS, T)
    # the other three pass the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    assert c.modswitch(rot=np.zeros(c.rot.size, dtype=np.uint32)) != EINVAL
    assert c.extract(ext=np.zeros(c.ext.size, dtype=c.dtype)) != EINVAL
    assert c.boot(ext=np.zeros(c.ext.size, dtype=c.dtype)) != EINVAL
    assert c.untouched()


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan52, native128.Plan32], ids=["native64", "native32_plan52", "native128"])
def test_batch_zero_does_nothing_and_the_edges_of_the_ranges_are_valid(P):
    c = Case(P)
    assert c.modswitch(batch=0) == 0 and c.extract(batch=0) == 0 and c.boot(batch=0) == 0 and c.cbs(batch=0) == 0 and c.untouched()
    assert c.fn("circuit_bootstrap_manylut_batch")(c.plan._h, None, None, None, None, L, K, 4, 2, 5, 3, 6, 2, T, 0, None, 0, 0, None) == 0
    # what passes the argument checks needs a device: any status but CNTT_EINVAL
    assert c.modswitch(t=LOGN, rot=np.zeros(c.rot.size, dtype=np.uint32)) != EINVAL
    assert c.extract(count=N, ext=np.zeros(B * N * (K * N + 1) * c.pw, dtype=c.dtype)) != EINVAL
    assert c.boot(t=LOGN, count=N, ext=np.zeros(B * N * (K * N + 1) * c.pw, dtype=c.dtype)) != EINVAL
    assert c.cbs(t=LOGN - 1, cbs=(1, N // 2), out=[np.zeros(B * (K + 1) * (N // 2) * (K + 1) * N, dtype=c.plan.res_dtype) for _ in range(c.np)]) != EINVAL
    assert c.cbs(t=1, out=[np.zeros(c.out[0].size, dtype=c.plan.res_dtype) for _ in range(c.np)], ws=c.ws) != EINVAL
    # lwe_dim = 0 with a NULL bootstrapping key
    assert c.cbs(lwe_dim=0, bsk=None, lwe=c.lwe[:B * c.pw], out=[np.zeros(c.out[0].size, dtype=c.plan.res_dtype) for _ in range(c.np)]) != EINVAL


@pytest.mark.parametrize("P", [native64.Plan32, native128.Plan32], ids=["native64", "native128"])
def test_python_wrappers_panic_on_bad_shapes(P):
    c = Case(P)
    pl = c.plan
    for args in ((c.rot[:-1], c.lwe, L, T), (c.rot, c.lwe, L, -1), (c.rot, c.lwe, 4, T), (c.rot.astype(np.uint64), c.lwe, L, T)):
        with pytest.raises((Panic, TypeError)):
            pl.lwe_modswitch_manylut_batch(*args)
    for args in ((c.ext[:-c.pw], c.glwe, K, 3), (c.ext, c.glwe, K, 0), (c.ext, c.glwe[:-c.pw], K, 3), (c.ext, c.glwe, K, 2)):
        with pytest.raises((Panic, TypeError)):
            pl.sample_extract_many_batch(*args)
    good = (c.ext, c.lwe, c.lut, c.bsk, L, K) + PBS + (T, 3)
    for i, bad in [(0, c.ext[:-c.pw]), (1, c.lwe[:-c.pw]), (2, c.lut[:-c.pw]), (3, [b[:-N] for b in c.bsk]), (3, c.bsk[:-1]), (4, -1), (6, 0), (7, 0),
                   (8, -1), (9, 0), (9, 2)]:
        args = list(good)
        args[i] = bad
        with pytest.raises((Panic, TypeError)):
            pl.bootstrap_manylut_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: lut_count above 2^t
        pl.bootstrap_manylut_batch(np.zeros(B * 5 * (K * N + 1) * c.pw, dtype=c.dtype), c.lwe, c.lut, c.bsk, L, K, *PBS, T, 5)
    good = (c.out, c.lwe, c.bsk, c.fk, L, K) + PBS + KS + CBS + (T,)
    for i, bad in [(0, c.out[:-1]), (0, [o[:-N] for o in c.out]), (1, c.lwe[:-c.pw]), (2, [b[:-N] for b in c.bsk]), (3, c.fk[:-c.pe]), (2, None), (4, -1),
                   (5, -1), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0), (11, 3), (12, -1)]:
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
@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_of_two_wrong_arguments_the_earlier_check_answers(P):
    c = Case(P)
    W = 8 * c.plan.WORD
    big = np.full(1 << 16, POISON, dtype=np.uint64)
    bigw = big.view(c.dtype)
    out_in_big = with_plane(c.out, 0, big.view(c.plan.res_dtype)[:c.out[0].size])
    ws_in_big = big.view(np.uint8)[256:256 + c.ws.nbytes]
    pws_in_big = big.view(np.uint8)[256:256 + c.pws.nbytes]
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
        (c.boot, dict(lut=None, ext=bigw[:c.ext.size], ws=pws_in_big), "lut is NULL"),
        # the one-rotation circuit bootstrap
        (c.cbs, dict(plan=None, pbs=(0, 2)), "plan is NULL"),
        (c.cbs, dict(pbs=(0, 2), ks=(0, 2)), "pbs_base_log is 0"), (c.cbs, dict(ks=(32, 1), cbs=(4, 0)), "ks_base_log = 32 is above 31"),
        (c.cbs, dict(cbs=(W // 2, 2), t=LOGN + 1), "2 has no inverse mod 2^w"), (c.cbs, dict(cbs=(W, 1), t=LOGN + 1), "2 has no inverse mod 2^w"),
        (c.cbs, dict(t=LOGN + 1, cbs=(1, W - 1)), "log_lut_count = 6 exceeds"),
        (c.cbs, dict(t=LOGN, cbs=(1, 33)), "exceeds ntt_size / 2") if W - 1 >= 33 else (c.cbs, dict(t=LOGN, k=(1 << 32) - 1), "exceeds ntt_size / 2"),
        (c.cbs, dict(t=0, k=(1 << 32) - 1), "cbs_levels = 2 exceeds 2^log_lut_count = 1"),
        (c.cbs, dict(k=(1 << 32) - 1, batch=1 << 63), "glwe_dim too large"),
        (c.cbs, dict(batch=1 << 32, lwe_dim=1 << 60), "too large for one launch"),
        (c.cbs, dict(lwe_dim=1 << 60, out=None), "2^63 bytes"),
        (c.cbs, dict(out=None, lwe=None), "ggsw_ntt_out is NULL"),
        (c.cbs, dict(lwe=None, fk=None), "lwe_in is NULL"), (c.cbs, dict(bsk=None, fk=None), "bsk_ntt is NULL"),
        (c.cbs, dict(fk=None, ws=c.ws, ws_bytes=c.ws.nbytes - 1), "fpksk is NULL"),
        (c.cbs, dict(out=out_in_big, ws=ws_in_big, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"),
        (c.cbs, dict(lwe=Raw(c.lwe.ctypes.data + 1), out=out_in_big, ws=ws_in_big), "lwe_in is not")]
    for call, kw, word in cases:
        assert call(**kw) == EINVAL, (call.__name__, kw)
        assert word in err(), (call.__name__, kw, err())
        assert c.untouched() and (big == POISON).all(), (call.__name__, kw)


def test_the_binary_kinds_are_refused_before_the_gadgets():
    c = Case(native_binary64.Plan32)
    assert c.cbs(pbs=(0, 2)) == EINVAL and "native_binary" in err(), err()
    assert c.cbs(t=LOGN + 1, cbs=(0, 0), ks=(32, 1)) == EINVAL and "native_binary" in err(), err()
    assert c.untouched()
