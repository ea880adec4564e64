"""C ABI of the programmable bootstrap (include/cntt_pbs.h through include/cntt_ext.h): the header is plain C11, the five names are
declared through cntt_ext.h and exported, cntt.h keeps its 87 entry points and cntt_ext.h's own text its 2, every CNTT_EINVAL case is
refused on host buffers by the argument checks that precede any device call (outputs untouched, argument named),
pbs_workspace_bytes is the header's formula, the Python wrappers panic on bad shapes -- and the plain-int model of the modulus switch
and of the sample extraction that tests/test_gpu_native_pbs.py compares the kernels with is itself checked here.  No GPU needed."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128
from concrete_ntt_amd._lib import EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cntt_ext.h")
PBS = os.path.join(ROOT, "include", "cntt_pbs.h")
HEADER = os.path.join(ROOT, "include", "cntt.h")
NEW = {"cntt_native_lwe_modswitch_batch", "cntt_native_blind_rotate_batch", "cntt_native_sample_extract_batch",
       "cntt_native_bootstrap_batch", "cntt_native_pbs_workspace_bytes"}


# -- the model (restated in tests/test_gpu_native_pbs.py) -------------------------------------------------------------------------
def ms(x, w, logn):
    return (((x >> (w - logn - 2)) + 1) >> 1) % (2 << logn)


def extract(glwe, h, w):
    """glwe: k + 1 lists of n ints -> k n + 1 ints."""
    n, M, k = len(glwe[0]), 1 << w, len(glwe) - 1
    out = []
    for p in range(k):
        out += [glwe[p][h - j] if j <= h else (-glwe[p][h - j + n]) % M for j in range(n)]
    return out + [glwe[k][h]]


def negacyclic(a, b, M):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] = (out[i + j] + x * y) % M
            else:
                out[i + j - n] = (out[i + j - n] - x * y) % M
    return out


@pytest.mark.parametrize("w", [32, 64, 128])
@pytest.mark.parametrize("logn", [5, 10, 15])
def test_modswitch_model_is_round_to_nearest_ties_up(w, logn):
    rng = np.random.default_rng(w + logn)
    two_n, s = 2 << logn, w - logn - 1
    words = [0, 1, (1 << w) - 1, (1 << w) - (1 << (s - 1)), (1 << w) - (1 << (s - 1)) - 1]
    for k in (0, 1, two_n // 2, two_n - 1):
        words += [(k << s) + (1 << (s - 1)), (k << s) + (1 << (s - 1)) - 1]
    words += [int.from_bytes(rng.bytes(w // 8), "little") for _ in range(50)]
    for x in words:
        exact = Fraction(x * two_n, 1 << w)
        nearest = int(exact + Fraction(1, 2))          # floor(q + 1/2): ties up
        assert ms(x, w, logn) == nearest % two_n, (w, logn, x)
        assert abs(exact - nearest) <= Fraction(1, 2)
    assert ms((1 << w) - 1, w, logn) == 0              # rounds up to 2n, which wraps


@pytest.mark.parametrize("k", [1, 2])
def test_extraction_model_satisfies_the_phase_identity(k):
    """<extract(ct, h) mask, flattened key> subtracted from its body is coefficient h of body - sum_p A_p S_p (schoolbook)."""
    n, w = 16, 32
    M = 1 << w
    rng = np.random.default_rng(k)
    glwe = [[int(x) for x in rng.integers(0, M, size=n)] for _ in range(k + 1)]
    key = [[int(x) for x in rng.integers(0, 2, size=n)] for _ in range(k)]
    phase = list(glwe[k])
    for p in range(k):
        phase = [(x - y) % M for x, y in zip(phase, negacyclic(glwe[p], key[p], M))]
    flat = [s for p in key for s in p]
    for h in (0, 1, 7, n - 1):
        lwe = extract(glwe, h, w)
        assert len(lwe) == k * n + 1
        assert (lwe[-1] - sum(a * s for a, s in zip(lwe, flat))) % M == phase[h], (k, h)


# -- the surface -----------------------------------------------------------------------------------------------------------------
def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_reached_through_cntt_ext_h():
    for path in (PBS, EXT):
        r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert set(declarations(PBS)) == NEW
    text = subprocess.run(["gcc", "-std=c11", "-E", "-P", "-x", "c", EXT], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", text))
    assert re.search(r'^#include "cntt_pbs.h"$', open(EXT).read(), flags=re.M)


def test_library_exports_the_five_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    base = declarations(HEADER)
    assert len(base) == 87, len(base)
    assert not (NEW & set(base))
    # the file's own text declares its two functions and nothing else, and names none of the new ones in front of a "("
    assert sorted(declarations(EXT)) == ["cntt_native_external_product_batch", "cntt_native_max_terms"]
    assert not (NEW & set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", open(EXT).read())))


def test_end_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_host_plan.py reads the transform units: three kernels, u32 / u64 /
    128-bit words (the set-up kernel also in its streaming form), none with a private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_pbs.o")
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
    for kernel, count in (("native_lwe_modswitch_kernel", 3), ("native_pbs_init_kernel", 6), ("native_sample_extract_kernel", 3)):
        assert sum(kernel in s for s in seen) == count, (kernel, seen)


@pytest.mark.parametrize("cls,wb", [(native32.Plan32, 4), (native64.Plan32, 8), (native128.Plan32, 16), (native64.Plan52, 8)])
def test_workspace_bytes_is_the_formula_of_the_header(cls, wb):
    def up(x):
        return (x + 255) // 256 * 256

    for n, L, k, levels, batch in ((32, 0, 1, 1, 1), (1024, 7, 1, 3, 5), (256, 630, 2, 4, 37), (2048, 3, 0, 2, 1000)):
        plan = cls.try_new(n)
        want = up(batch * (k + 1) * levels * n * wb) + up((L + 1) * batch * 4) + up(batch * (k + 1) * n * wb)
        assert plan.pbs_workspace_bytes(L, k, levels, batch) == want, (n, L, k, levels, batch)
        assert want >= batch * (k + 1) * levels * n * wb          # at least what blind_rotate needs
    assert cntt.lib().cntt_native_pbs_workspace_bytes(None, 5, 1, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, L, K, B = 32, 3, 1, 2


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments of every call for native64 Plan32 at n = 32, L = 3, k = 1, batch = 2; outputs filled with 7."""

    def __init__(self, levels=2):
        self.plan = native64.Plan32.try_new(N)
        self.levels = levels
        self.acc = np.full(B * (K + 1) * N, 7, dtype=np.uint64)
        self.lut = np.arange((K + 1) * N, dtype=np.uint64)
        self.rot = np.zeros((L + 1) * B, dtype=np.uint32)
        self.keys = [np.zeros(L * (K + 1) * levels * (K + 1) * N, dtype=np.uint32) for _ in range(self.plan.NPRIMES)]
        self.lwe_in = np.arange(B * (L + 1), dtype=np.uint64)
        self.lwe_out = np.full(B * (K * N + 1), 7, dtype=np.uint64)
        self.ws = np.zeros(self.plan.pbs_workspace_bytes(L, K, levels, B), dtype=np.uint8)

    def kp(self, null_plane=None):
        return (ctypes.c_void_p * self.plan.NPRIMES)(*[None if i == null_plane else k.ctypes.data for i, k in enumerate(self.keys)])

    def rotate(self, base_log=8, levels=None, acc=None, lut=None, rot="own", keys="own", ws=None, ws_bytes=None, glwe_dim=K):
        acc = self.acc if acc is None else acc
        lut = self.lut if lut is None else lut
        rot = self.rot if isinstance(rot, str) else rot
        keys = self.kp() if isinstance(keys, str) else keys
        return cntt.lib().cntt_native_blind_rotate_batch(
            self.plan._h, ptr(acc), ptr(lut), 0, ptr(rot), keys, L, glwe_dim, base_log, self.levels if levels is None else levels, B,
            ptr(ws), (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes, 0, None)

    def bootstrap(self, base_log=8, levels=None, out=None, lwe_in=None, lut=None, keys="own", ws=None, ws_bytes=None, glwe_dim=K):
        out = self.lwe_out if out is None else out
        lwe_in = self.lwe_in if lwe_in is None else lwe_in
        lut = self.lut if lut is None else lut
        keys = self.kp() if isinstance(keys, str) else keys
        return cntt.lib().cntt_native_bootstrap_batch(
            self.plan._h, ptr(out), ptr(lwe_in), ptr(lut), 0, keys, L, glwe_dim, base_log, self.levels if levels is None else levels, B,
            ptr(ws), (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes, 0, None)

    def untouched(self):
        return (self.acc == 7).all() and (self.lwe_out == 7).all()


BAD = [(0, 2, "base_log"), (8, 0, "levels"), (33, 2, "base_log * levels"), (1, 65, "base_log * levels")]


@pytest.mark.parametrize("base_log,levels,word", BAD)
def test_the_decomposition_cases_are_refused(base_log, levels, word):
    c = Case()
    assert c.rotate(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.bootstrap(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.untouched()


def test_null_rot_and_null_key_plane_and_max_terms_are_refused():
    c = Case()
    assert c.rotate(rot=None) == EINVAL and "rot_t" in err()
    for call in (c.rotate, c.bootstrap):
        assert call(keys=c.kp(null_plane=3)) == EINVAL and "key residue plane" in err()
        assert call(keys=None) == EINVAL and "bsk_ntt" in err()
        # (k + 1) * levels past cntt_native_max_terms(): glwe_dim alone does it, before any buffer is looked at
        assert call(glwe_dim=c.plan.max_terms(), levels=1) == EINVAL and "cntt_native_max_terms" in err()
    assert c.untouched()


def test_workspace_too_small_or_misaligned_is_refused():
    c = Case()
    digits = B * (K + 1) * c.levels * N * 8
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
    assert (big == 7).all() and c.untouched()


def test_host_path_refuses_an_exponent_that_is_not_below_2n():
    c = Case()
    c.rot[5] = 2 * N
    assert c.rotate() == EINVAL and "rot_t[5]" in err()
    assert c.untouched()


def test_modswitch_and_extract_refuse_bad_arguments():
    plan = native64.Plan32.try_new(N)
    L_ = cntt.lib()
    lwe = np.arange(B * (L + 1), dtype=np.uint64)
    rot = np.full((L + 1) * B, 7, dtype=np.uint32)
    assert L_.cntt_native_lwe_modswitch_batch(plan._h, None, ptr(lwe), L, B, 0, None) == EINVAL and "rot_t" in err()
    assert L_.cntt_native_lwe_modswitch_batch(plan._h, ptr(rot), None, L, B, 0, None) == EINVAL and "lwe" in err()
    assert L_.cntt_native_lwe_modswitch_batch(plan._h, ptr(lwe.view(np.uint32)[2:]), ptr(lwe), L, B, 0, None) == EINVAL
    assert "rot_t overlaps lwe" in err()
    assert L_.cntt_native_lwe_modswitch_batch(None, ptr(rot), ptr(lwe), L, B, 0, None) == EINVAL and "plan" in err()
    assert (rot == 7).all()
    glwe = np.arange(B * (K + 1) * N, dtype=np.uint64)
    out = np.full(B * (K * N + 1), 7, dtype=np.uint64)
    for index in (N, N + 1, 2 ** 40):
        assert L_.cntt_native_sample_extract_batch(plan._h, ptr(out), ptr(glwe), K, index, B, 0, None) == EINVAL and "index" in err()
    assert L_.cntt_native_sample_extract_batch(plan._h, None, ptr(glwe), K, 0, B, 0, None) == EINVAL and "lwe_out" in err()
    assert L_.cntt_native_sample_extract_batch(plan._h, ptr(glwe[N:]), ptr(glwe), K, 0, 1, 0, None) == EINVAL
    assert "lwe_out overlaps glwe" in err()
    assert (out == 7).all()


def test_batch_zero_does_nothing():
    c = Case()
    L_ = cntt.lib()
    assert L_.cntt_native_lwe_modswitch_batch(c.plan._h, None, None, L, 0, 0, None) == 0
    assert L_.cntt_native_sample_extract_batch(c.plan._h, None, None, K, 0, 0, 0, None) == 0
    assert L_.cntt_native_blind_rotate_batch(c.plan._h, None, None, 0, None, None, L, K, 8, 2, 0, None, 0, 0, None) == 0
    assert L_.cntt_native_bootstrap_batch(c.plan._h, None, None, None, 0, None, L, K, 8, 2, 0, None, 0, 0, None) == 0


def test_python_wrappers_panic_on_bad_shapes():
    c = Case()
    p = c.plan
    with pytest.raises(cntt.Panic):
        p.lwe_modswitch_batch(c.rot[:-1], c.lwe_in, L)                                   # rot_t too short
    with pytest.raises(cntt.Panic):
        p.lwe_modswitch_batch(c.rot, c.lwe_in, L + 1)                                    # not a whole number of ciphertexts
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc[:-1], c.lut, c.rot, c.keys, L, K, 8, 2)               # acc not whole polynomials
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut[:N], c.rot, c.keys, L, K, 8, 2)                # lut too short
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut, c.rot[:B], c.keys, L, K, 8, 2)                # rot_t without its rows
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut, c.rot, c.keys[:-1], L, K, 8, 2)               # a plane missing
    with pytest.raises(cntt.Panic):
        p.blind_rotate_batch(c.acc, c.lut, c.rot, c.keys, L, K, 8, 3)                    # planes sized for levels = 2
    with pytest.raises(cntt.Panic):
        p.sample_extract_batch(c.lwe_out[:-1], c.acc, K)                                 # lwe_out too short
    with pytest.raises(cntt.Panic):
        p.bootstrap_batch(c.lwe_out[:-1], c.lwe_in, c.lut, c.keys, L, K, 8, 2)
    with pytest.raises(cntt.Panic):
        p.bootstrap_batch(c.lwe_out, c.lwe_in, c.lut, c.keys, L, K, 8, 2, lut_per_element=True)   # one shared table given
    with pytest.raises(cntt.Panic):   # through the C checks
        p.bootstrap_batch(c.lwe_out, c.lwe_in, c.lut, c.keys, L, K, 33, 2)
    with pytest.raises(cntt.Panic):
        p.sample_extract_batch(c.lwe_out, c.acc.copy(), K, index=N)
    assert c.untouched()
