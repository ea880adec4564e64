"""C ABI of the prime plans' programmable bootstrap (include/cntt_prime_pbs.h): the header is plain C11, its twelve names are declared
and exported, cntt.h keeps its 87 entry points and cntt_ext.h is not touched, every CNTT_EINVAL case is refused on host buffers by the
argument checks that precede any device call (outputs untouched, argument named), pbs_workspace_bytes is the header's formula, the
Python wrappers panic on bad shapes, and the code object of the new kernels has no scratch and no spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEWH = os.path.join(ROOT, "include", "cntt_prime_pbs.h")
EXT = os.path.join(ROOT, "include", "cntt_ext.h")
HEADER = os.path.join(ROOT, "include", "cntt.h")
CALLS = ["gadget_decompose_batch", "lwe_modswitch_batch", "blind_rotate_batch", "sample_extract_batch", "bootstrap_batch",
         "pbs_workspace_bytes"]
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS}
P62, PM64, P30 = 4611686018427322369, 18446744069414584321, 1062862849


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_declares_the_twelve():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", NEWH],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(NEW) == 12 and set(declarations(NEWH)) == NEW and len(declarations(NEWH)) == 12
    text = open(NEWH).read()
    assert re.search(r'^#include "cntt_gadget.h"$', text, flags=re.M)          # cntt_src_mode_t comes from there
    assert "NOT claimed" in text and "n^-1" in text and "strict range" in text


def test_library_exports_the_twelve_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    base = declarations(HEADER)
    assert len(base) == 87, len(base)
    assert not (NEW & set(base))
    assert sorted(declarations(EXT)) == ["cntt_native_external_product_batch", "cntt_native_max_terms"]
    assert "cntt_prime_pbs.h" not in open(EXT).read() and "cntt_prime_pbs.h" not in open(HEADER).read()


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_native_pbs_abi.py reads its unit: four kernels on u32 / u64 words
    (decomposition and set-up also in their streaming form), none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_pbs.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "pbs.fat"), str(tmp_path / "pbs.co")
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
    for kernel, count in (("prime_gadget_kernel", 4), ("prime_lwe_modswitch_kernel", 2), ("prime_pbs_init_kernel", 4),
                          ("prime_sample_extract_kernel", 2)):
        assert sum(kernel in s for s in seen) == count, (kernel, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_is_the_formula_of_the_header(mod, p, wb):
    def up(x):
        return (x + 255) // 256 * 256

    for n, L, k, levels, batch in ((32, 0, 1, 1, 1), (1024, 7, 1, 3, 5), (256, 630, 2, 4, 37), (2048, 3, 0, 2, 1000)):
        plan = mod.Plan.try_new(n, p)
        want = up(batch * (k + 1) * levels * n * wb) + up((L + 1) * batch * 4) + up(batch * (k + 1) * n * wb)
        assert plan.pbs_workspace_bytes(L, k, levels, batch) == want, (n, L, k, levels, batch)
        assert want >= batch * (k + 1) * levels * n * wb          # at least what blind_rotate needs
    assert cntt.lib().cntt_prime64_pbs_workspace_bytes(None, 5, 1, 2, 3) == 0
    assert cntt.lib().cntt_prime32_pbs_workspace_bytes(None, 5, 1, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, L, K, B = 32, 3, 1, 2


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments of every call at n = 32, L = 3, k = 1, batch = 2; outputs filled with 7."""

    def __init__(self, bits=64, p=P62, levels=2):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.levels = levels
        self.acc = np.full(B * (K + 1) * N, 7, dtype=self.dtype)
        self.lut = np.arange((K + 1) * N, dtype=self.dtype)
        self.rot = np.zeros((L + 1) * B, dtype=np.uint32)
        self.key = np.zeros(L * (K + 1) * levels * (K + 1) * N, dtype=self.dtype)
        self.lwe_in = np.arange(B * (L + 1), dtype=self.dtype)
        self.lwe_out = np.full(B * (K * N + 1), 7, dtype=self.dtype)
        self.terms = np.full(B * (K + 1) * N * levels, 7, dtype=self.dtype)
        self.ws = np.zeros(self.plan.pbs_workspace_bytes(L, K, levels, B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def decompose(self, base_log=8, levels=None, terms=None, polys=None, rot="own", mode=2):
        terms = self.terms if terms is None else terms
        polys = self.acc if polys is None else polys
        rot = self.rot if isinstance(rot, str) else rot
        return self.fn("gadget_decompose_batch")(self.plan._h, ptr(terms), ptr(polys), ptr(rot), K + 1, base_log,
                                                 self.levels if levels is None else levels, mode, B, 0, None)

    def rotate(self, base_log=8, levels=None, acc=None, lut=None, rot="own", key="own", ws=None, ws_bytes=None, glwe_dim=K):
        acc = self.acc if acc is None else acc
        lut = self.lut if lut is None else lut
        rot = self.rot if isinstance(rot, str) else rot
        key = self.key if isinstance(key, str) else key
        return self.fn("blind_rotate_batch")(
            self.plan._h, ptr(acc), ptr(lut), 0, ptr(rot), ptr(key), L, glwe_dim, base_log, self.levels if levels is None else levels, B,
            ptr(ws), (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes, 0, None)

    def bootstrap(self, base_log=8, levels=None, out=None, lwe_in=None, lut=None, key="own", ws=None, ws_bytes=None, glwe_dim=K):
        out = self.lwe_out if out is None else out
        lwe_in = self.lwe_in if lwe_in is None else lwe_in
        lut = self.lut if lut is None else lut
        key = self.key if isinstance(key, str) else key
        return self.fn("bootstrap_batch")(
            self.plan._h, ptr(out), ptr(lwe_in), ptr(lut), 0, ptr(key), L, glwe_dim, base_log, self.levels if levels is None else levels, B,
            ptr(ws), (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes, 0, None)

    def untouched(self):
        return (self.acc == 7).all() and (self.lwe_out == 7).all() and (self.terms == 7).all()


# the bound is W, the bit length of the modulus: 62 for P62 (so 8 * 8 = 64 is refused although it fits the word), 64, 30
BAD = [(64, P62, 0, 2, "base_log"), (64, P62, 8, 0, "levels"), (64, P62, 32, 2, "base_log * levels"), (64, P62, 63, 1, "base_log * levels"),
       (64, PM64, 33, 2, "base_log * levels"), (64, PM64, 1, 65, "base_log * levels"), (32, P30, 31, 1, "base_log * levels"),
       (32, P30, 16, 2, "base_log * levels")]


@pytest.mark.parametrize("bits,p,base_log,levels,word", BAD)
def test_the_decomposition_cases_are_refused(bits, p, base_log, levels, word):
    c = Case(bits, p)
    assert c.decompose(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.rotate(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.bootstrap(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.untouched()


def test_the_bound_is_the_bit_length_of_the_modulus_and_there_is_no_term_bound():
    """base_log * levels = W itself passes the check (the next refusal names another argument), and a huge glwe_dim * levels is not
    refused for the number of terms: a prime plan's accumulation is modular"""
    for bits, p, base_log, levels in ((64, P62, 31, 2), (64, PM64, 16, 4), (64, PM64, 64, 1), (32, P30, 30, 1)):
        c = Case(bits, p)
        assert c.decompose(base_log=base_log, levels=levels, terms=c.acc[:1]) == EINVAL and "terms overlaps polys" in err()
    c = Case()
    assert c.rotate(glwe_dim=1 << 20, levels=1, rot=None) == EINVAL and "rot_t" in err()
    assert c.bootstrap(glwe_dim=1 << 20, levels=1, out=c.lwe_in) == EINVAL and "max_terms" not in err()
    assert c.untouched()


def test_unknown_mode_null_rot_and_overlap_are_refused_by_the_decomposition():
    c = Case()
    assert c.decompose(mode=3) == EINVAL and "src_mode" in err()
    assert c.decompose(rot=None) == EINVAL and "rot" in err()
    assert c.decompose(rot=None, mode=0, terms=c.acc[N:]) == EINVAL and "terms overlaps polys" in err()
    assert c.fn("gadget_decompose_batch")(None, ptr(c.terms), ptr(c.acc), ptr(c.rot), K + 1, 8, 2, 2, B, 0, None) == EINVAL and "plan" in err()
    c.rot[1] = 2 * N          # host path: an exponent that is not below 2n
    assert c.decompose() == EINVAL and "rot[1]" in err()
    assert c.untouched()


def test_null_arguments_are_refused():
    c = Case()
    assert c.rotate(rot=None) == EINVAL and "rot_t" in err()
    for call in (c.rotate, c.bootstrap):
        assert call(key=None) == EINVAL and "bsk_ntt" in err()
    z = np.zeros(0, dtype=np.uint64)
    assert c.fn("blind_rotate_batch")(c.plan._h, None, ptr(c.lut), 0, ptr(c.rot), ptr(c.key), L, K, 8, 2, B, None, 0, 0, None) == EINVAL
    assert "acc" in err()
    assert c.fn("blind_rotate_batch")(c.plan._h, ptr(c.acc), None, 0, ptr(c.rot), ptr(c.key), L, K, 8, 2, B, None, 0, 0, None) == EINVAL
    assert "lut" in err()
    assert c.fn("bootstrap_batch")(c.plan._h, None, ptr(c.lwe_in), ptr(c.lut), 0, ptr(c.key), L, K, 8, 2, B, None, 0, 0, None) == EINVAL
    assert "lwe_out" in err()
    assert c.fn("bootstrap_batch")(c.plan._h, ptr(c.lwe_out), None, ptr(c.lut), 0, ptr(c.key), L, K, 8, 2, B, None, 0, 0, None) == EINVAL
    assert "lwe_in" in err()
    assert c.fn("bootstrap_batch")(None, ptr(c.lwe_out), ptr(c.lwe_in), ptr(c.lut), 0, ptr(c.key), L, K, 8, 2, B, None, 0, 0, None) == EINVAL
    assert "plan" in err() and z.size == 0
    assert c.untouched()


@pytest.mark.parametrize("bits,p", [(64, P62), (32, P30)])
def test_workspace_too_small_or_misaligned_is_refused(bits, p):
    c = Case(bits, p)
    digits = B * (K + 1) * c.levels * N * (bits // 8)
    assert c.rotate(ws=c.ws, ws_bytes=digits - 1) == EINVAL and "workspace_bytes" in err()
    assert c.bootstrap(ws=c.ws, ws_bytes=c.ws.nbytes - 1) == EINVAL and "workspace_bytes" in err()
    assert c.bootstrap(ws=c.ws, ws_bytes=digits) == EINVAL and "workspace_bytes" in err()     # enough for blind_rotate only
    assert c.rotate(ws=c.ws[1:]) == EINVAL and "aligned" in err()
    assert c.untouched()


def test_overlaps_are_refused():
    c = Case()
    big = np.full(4 * B * (K + 1) * N, 7, dtype=np.uint64)
    acc = big[:B * (K + 1) * N]
    assert c.rotate(acc=acc, lut=big[N:N + (K + 1) * N]) == EINVAL and "acc overlaps lut" in err()
    assert c.rotate(acc=acc, rot=big[8:].view(np.uint32)[:(L + 1) * B]) == EINVAL and "acc overlaps rot_t" in err()
    ws = big.view(np.uint8)[16 * 8:]
    assert c.rotate(acc=acc, ws=ws) == EINVAL and "acc overlaps workspace" in err()
    out = big[:B * (K * N + 1)]
    assert c.bootstrap(out=out, lwe_in=big[4:4 + B * (L + 1)]) == EINVAL and "lwe_out overlaps lwe_in" in err()
    assert c.bootstrap(out=out, lut=big[8:8 + (K + 1) * N]) == EINVAL and "lwe_out overlaps lut" in err()
    assert c.bootstrap(out=out, ws=ws) == EINVAL and "lwe_out overlaps workspace" in err()
    assert c.bootstrap(lwe_in=big[16:16 + B * (L + 1)], ws=ws) == EINVAL and "lwe_in overlaps workspace" in err()
    assert c.bootstrap(lut=big[16:16 + (K + 1) * N], ws=ws) == EINVAL and "lut overlaps workspace" in err()
    assert (big == 7).all() and c.untouched()


def test_host_path_refuses_an_exponent_that_is_not_below_2n():
    c = Case()
    c.rot[5] = 2 * N
    assert c.rotate() == EINVAL and "rot_t[5]" in err()
    assert c.untouched()


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_modswitch_and_extract_refuse_bad_arguments(bits, p):
    c = Case(bits, p)
    ms, ex = c.fn("lwe_modswitch_batch"), c.fn("sample_extract_batch")
    lwe = np.arange(B * (L + 1), dtype=c.dtype)
    rot = np.full((L + 1) * B, 7, dtype=np.uint32)
    assert ms(c.plan._h, None, ptr(lwe), L, B, 0, None) == EINVAL and "rot_t" in err()
    assert ms(c.plan._h, ptr(rot), None, L, B, 0, None) == EINVAL and "lwe" in err()
    assert ms(c.plan._h, ptr(lwe.view(np.uint32)[2:]), ptr(lwe), L, B, 0, None) == EINVAL and "rot_t overlaps lwe" in err()
    assert ms(None, ptr(rot), ptr(lwe), L, B, 0, None) == EINVAL and "plan" in err()
    assert (rot == 7).all()
    glwe = np.arange(B * (K + 1) * N, dtype=c.dtype)
    out = np.full(B * (K * N + 1), 7, dtype=c.dtype)
    for index in (N, N + 1, 2 ** 40):
        assert ex(c.plan._h, ptr(out), ptr(glwe), K, index, B, 0, None) == EINVAL and "index" in err()
    assert ex(c.plan._h, None, ptr(glwe), K, 0, B, 0, None) == EINVAL and "lwe_out" in err()
    assert ex(c.plan._h, ptr(out), None, K, 0, B, 0, None) == EINVAL and "glwe" in err()
    assert ex(c.plan._h, ptr(glwe[N:]), ptr(glwe), K, 0, 1, 0, None) == EINVAL and "lwe_out overlaps glwe" in err()
    assert (out == 7).all()


def test_batch_zero_does_nothing():
    c = Case()
    assert c.fn("gadget_decompose_batch")(c.plan._h, None, None, None, K + 1, 8, 2, 0, 0, 0, None) == 0
    assert c.fn("gadget_decompose_batch")(c.plan._h, None, None, None, 0, 8, 2, 0, B, 0, None) == 0
    assert c.fn("lwe_modswitch_batch")(c.plan._h, None, None, L, 0, 0, None) == 0
    assert c.fn("sample_extract_batch")(c.plan._h, None, None, K, 0, 0, 0, None) == 0
    assert c.fn("blind_rotate_batch")(c.plan._h, None, None, 0, None, None, L, K, 8, 2, 0, None, 0, 0, None) == 0
    assert c.fn("bootstrap_batch")(c.plan._h, None, None, None, 0, None, L, K, 8, 2, 0, None, 0, 0, None) == 0


def test_python_wrappers_panic_on_bad_shapes():
    c = Case()
    p = c.plan
    with pytest.raises(cntt.Panic):
        p.gadget_decompose_batch(c.terms[:-1], c.acc, 8, 2, rot=c.rot[:B], mode="cmux")   # terms too short
    with pytest.raises(cntt.Panic):
        p.gadget_decompose_batch(c.terms, c.acc, 8, 2, mode="cmux")                       # the mode needs rot
    with pytest.raises(cntt.Panic):
        p.gadget_decompose_batch(c.terms, c.acc, 8, 2, rot=c.rot[:B], mode="spin")
    with pytest.raises(cntt.Panic):
        p.lwe_modswitch_batch(c.rot[:-1], c.lwe_in, L)                                   # rot_t too short
    with pytest.raises(cntt.Panic):
        p.lwe_modswitch_batch(c.rot, c.lwe_in, L + 1)                                    # not a whole number of ciphertexts
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc[:-1], c.lut, c.rot, c.key, L, K, 8, 2)                # acc not whole polynomials
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut[:N], c.rot, c.key, L, K, 8, 2)                 # lut too short
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut, c.rot[:B], c.key, L, K, 8, 2)                 # rot_t without its rows
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut, c.rot, c.key, L, K, 8, 3)                     # key sized for levels = 2
    with pytest.raises(cntt.Panic):
        p.sample_extract_batch(c.lwe_out[:-1], c.acc, K)                                 # lwe_out too short
    with pytest.raises(cntt.Panic):
        p.bootstrap_batch(c.lwe_out[:-1], c.lwe_in, c.lut, c.key, L, K, 8, 2)
    with pytest.raises(cntt.Panic):
        p.bootstrap_batch(c.lwe_out, c.lwe_in, c.lut, c.key, L, K, 8, 2, lut_per_element=True)   # one shared table given
    with pytest.raises(cntt.Panic):   # through the C checks: 32 * 2 > W = 62
        p.bootstrap_batch(c.lwe_out, c.lwe_in, c.lut, c.key, L, K, 32, 2)
    with pytest.raises(cntt.Panic):
        p.sample_extract_batch(c.lwe_out, c.acc.copy(), K, index=N)
    assert c.untouched()
