"""C ABI of the native plans' multi-bit bootstrap (include/cntt_multibit.h): the header is plain C11 and declares the five calls, the
library exports them, the workspace figure is the header's formula, the refusals are made without a device, and the code object of the
new unit holds one kernel instance without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary64
from concrete_ntt_amd._lib import EINVAL, last_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "cntt_multibit.h")
NEW = {"cntt_native_multibit_grid", "cntt_native_multibit_accumulate_batch", "cntt_native_multibit_blind_rotate_batch",
       "cntt_native_multibit_bootstrap_batch", "cntt_native_multibit_pbs_workspace_bytes"}


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_declares_the_calls():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert set(declarations(HEADER)) == NEW and len(declarations(HEADER)) == 5
    text = open(HEADER).read()
    for phrase in ("least significant first", "(1 - s_", "NOT normalised", "NOT claimed", "cntt_native_max_terms = 1964", "First call",
                   "Plan52", "up(digits) + up(terms) + up(outputs) + up(rot) + up(acc)"):
        assert phrase in text, phrase
    assert "cntt_multibit.h" not in open(os.path.join(INC, "cntt.h")).read()


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_workspace_bytes_is_the_formula_of_the_header_and_the_bound_is_the_headers():
    def up(x):
        return (x + 255) & ~255

    for mod in (native32, native64, native128, native_binary64):
        for n, L, k, levels, g, batch in ((32, 0, 1, 1, 1, 1), (1024, 720, 1, 2, 3, 37), (4096, 12, 2, 3, 4, 5)):
            plan = mod.Plan32.try_new(n)
            polys = batch * (k + 1) * n
            want = (up(polys * levels * plan.WORD) + up(plan.NPRIMES * polys * levels * 4) + up(plan.NPRIMES * polys * 4)
                    + up((L + 1) * batch * 4) + up(polys * plan.WORD))
            assert plan.multibit_pbs_workspace_bytes(L, k, levels, g, batch) == want
    assert cntt.lib().cntt_native_multibit_pbs_workspace_bytes(None, 4, 1, 2, 2, 3) == 0
    assert native64.Plan52.try_new(1024).multibit_pbs_workspace_bytes(4, 1, 2, 2, 3) == 0
    assert native64.Plan32.try_new(1024).max_terms() == 1964
    grid = cntt.lib().cntt_native_multibit_grid
    assert grid(0) == 1 and grid(256) == 1 and grid(257) == 2 and grid(1 << 40) == grid(1 << 50) == 512


def refused(fn, *args):
    with pytest.raises(cntt.Panic) as e:
        fn(*args)
    return str(e.value)


def test_refusals_are_made_without_a_device():
    """host-memory operands: every refusal comes before the first device call, so none of these needs a GPU"""
    n, k, levels, beta, L, g, batch = 32, 1, 2, 4, 4, 2, 1
    plan = native64.Plan32.try_new(n)
    J = (k + 1) * levels
    lwe_in, lwe_out = np.zeros(batch * (L + 1), np.uint64), np.zeros(batch * (k * n + 1), np.uint64)
    lut, acc = np.zeros((k + 1) * n, np.uint64), np.zeros(batch * (k + 1) * n, np.uint64)
    rot_t = np.zeros((L + 1) * batch, np.uint32)

    def key(gg, LL=L, JJ=J):
        return [np.zeros(((LL // gg) * JJ * (k + 1) << gg) * n, np.uint32) for _ in range(plan.NPRIMES)]

    assert "grouping = 5" in refused(plan.multibit_bootstrap_batch, lwe_out, lwe_in, lut, key(1), L, k, beta, levels, 5)
    assert "grouping = 0" in refused(plan.multibit_blind_rotate_batch, acc, lut, rot_t, key(1), L, k, beta, levels, 0)
    assert "not a multiple of grouping" in refused(plan.multibit_bootstrap_batch, lwe_out, lwe_in, lut, key(1), L, k, beta, levels, 3)
    assert "exceeds the word width" in refused(plan.multibit_bootstrap_batch, lwe_out, lwe_in, lut, key(g), L, k, 33, levels, g)
    ws = np.zeros(16, np.uint8)
    assert "workspace_bytes = 16" in refused(plan.multibit_bootstrap_batch, lwe_out, lwe_in, lut, key(g), L, k, beta, levels, g, ws)
    bad_rot = rot_t.copy()
    bad_rot[1] = 2 * n
    assert "rot_t[1] = 64 is not below 2n" in refused(plan.multibit_blind_rotate_batch, acc, lut, bad_rot, key(g), L, k, beta, levels, g)
    # the max_terms bound: native64 at n = 32768 holds 61 terms; 2^4 * 2 * 2 = 64
    big = native64.Plan32.try_new(32768)
    mt = big.max_terms()
    assert mt < 64
    fn = cntt.lib().cntt_native_multibit_bootstrap_batch
    dummy = (ctypes.c_void_p * 5)(*[ctypes.c_void_p(16)] * 5)
    rc = fn(big._h, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 0, dummy, 4, 1, 4, 2, 4, 1, None, 0, 0, None)
    assert rc == EINVAL and ("= 64 exceeds cntt_native_max_terms() = %d" % mt) in last_error()
    # sizes whose workspace figure would wrap a size_t: refused, and the figure itself is 0
    rc = fn(plan._h, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 0, dummy, 4, 1 << 40, 4, 2, 2, 1 << 40, None, 0, 0, None)
    assert rc == EINVAL and "too large" in last_error()
    assert cntt.lib().cntt_native_multibit_pbs_workspace_bytes(plan._h, 4, 1 << 40, 2, 2, 1 << 40) == 0
    # a Plan52 kind, a NULL residue plane, a NULL plan
    p52 = native64.Plan52.try_new(n)
    rc = fn(p52._h, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 0, dummy, 4, 1, 4, 2, 2, 1, None, 0, 0, None)
    assert rc == EINVAL and "Plan52" in last_error()
    holes = (ctypes.c_void_p * 5)(16, 16, None, 16, 16)
    rc = fn(plan._h, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 0, holes, 4, 1, 4, 2, 2, 1, None, 0, 0, None)
    assert rc == EINVAL and "NULL key residue plane (bsk_mb[2])" in last_error()
    rc = fn(None, ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 0, dummy, 4, 1, 4, 2, 2, 1, None, 0, 0, None)
    assert rc == EINVAL and "plan is NULL" in last_error()
    acc_fn = cntt.lib().cntt_native_multibit_accumulate_batch
    rc = acc_fn(plan._h, holes, dummy, ctypes.c_void_p(16), dummy, 2, 1, 2, 1, 0, None)
    assert rc == EINVAL and "NULL residue plane (out_ntt[2])" in last_error()
    rc = acc_fn(plan._h, dummy, dummy, ctypes.c_void_p(16), dummy, 2, 1, 2, 1, 0, None)
    assert rc == EINVAL and "overlaps" in last_error()
    rc = acc_fn(p52._h, dummy, dummy, ctypes.c_void_p(16), dummy, 2, 1, 2, 1, 0, None)
    assert rc == EINVAL and "Plan52" in last_error()
    assert lwe_out.sum() == 0 and acc.sum() == 0


@pytest.mark.parametrize("call", ["blind_rotate_batch", "bootstrap_batch"])
def test_which_refusal_wins_when_two_arguments_are_wrong(call):
    """The order of the checks of multibit_host.hpp, which the prime plans share (test_prime_multibit_abi.py has the same cases): the
    grouping before the divisibility of lwe_dim and before the key, the digit budget before the workspace.  glwe_dim = 1, batch = 1;
    the pointers are never read."""
    plan = native64.Plan32.try_new(32)
    fn, p = plan._fn("multibit_" + call), ctypes.c_void_p
    args = (p(16), p(16), 0, p(16)) if call == "blind_rotate_batch" else (p(16), p(16), p(16), 0)
    dummy = (ctypes.c_void_p * plan.NPRIMES)(*[16] * plan.NPRIMES)

    def refusal(key, lwe_dim, base_log, levels, grouping, workspace=None, workspace_bytes=0):
        rc = fn(plan._h, *args, key, lwe_dim, 1, base_log, levels, grouping, 1, p(workspace), workspace_bytes, 0, None)
        assert rc == EINVAL
        return last_error()

    assert refusal(dummy, 4, 4, 2, 5) == "grouping = 5 is not in 1 ... 4"
    assert refusal(None, 4, 4, 2, 0) == "grouping = 0 is not in 1 ... 4"
    assert refusal(dummy, 4, 33, 2, 2, workspace=8, workspace_bytes=1 << 20) == "base_log * levels = 33 * 2 exceeds the word width 64"


def test_kernel_instance_has_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit: native_multibit_accumulate_kernel, one kernel, without a private segment or a spilled
    register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_multibit.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "mb.fat"), str(tmp_path / "mb.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = []
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) + int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
        # 46 VGPRs is the figure DESIGN records; 48 leaves one allocation granule for a compiler update, and anything above it is a
        # change of the inner loop that the record has to follow
        assert spills == 0 and scratch == 0 and vgprs <= 48, (name, spills, scratch, vgprs)
        seen.append(name)
    assert len(seen) == 1 and "native_multibit_accumulate_kernelIjE" in seen[0], seen
