"""C ABI of the prime plans' multi-bit bootstrap (include/cntt_prime_multibit.h): the header is plain C11 and declares the calls, the
library exports them, cntt.hpp mirrors them, the existing headers keep their surface, the workspace figure is the header's, and the
code object of the new unit holds the two kernel instances without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, MEM_DEVICE, MEM_HOST, last_error
from test_prime_pbs_model import P30, P62

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HEADER = os.path.join(INC, "cntt_prime_multibit.h")
CALLS = ["multibit_accumulate_batch", "multibit_blind_rotate_batch", "multibit_bootstrap_batch", "multibit_pbs_workspace_bytes"]
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS} | {"cntt_prime_multibit_grid"}
SURFACE = {"cntt.h": 87, "cntt_ext.h": 2, "cntt_pbs.h": 5, "cntt_keyswitch.h": 3, "cntt_pack.h": 2, "cntt_prime_pbs.h": 12,
           "cntt_prime_keyswitch.h": 6, "cntt_prime_pack.h": 4}


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_declares_the_calls():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert set(declarations(HEADER)) == NEW and len(declarations(HEADER)) == len(NEW) == 9
    text = open(HEADER).read()
    assert re.search(r'^#include "cntt_prime_pbs.h"$', text, flags=re.M)
    for phrase in ("least significant first", "(1 - s_", "n^-1 * fwd", "exact integer arithmetic mod p for EVERY prime", "NOT claimed",
                   "profiles/r17_prime_multibit.txt"):
        assert phrase in text, phrase
    assert "cntt_prime_multibit.h" not in open(os.path.join(INC, "cntt.h")).read()


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_existing_headers_keep_their_surface():
    for name, count in SURFACE.items():
        decl = declarations(os.path.join(INC, name))
        assert len(decl) == count, (name, len(decl))
        assert not (NEW & set(decl)), name


def test_cpp_mirror_has_the_four_methods():
    text = open(os.path.join(INC, "cntt.hpp")).read()
    assert '#include "cntt_prime_multibit.h"' in text
    for c in CALLS:
        assert "cntt_prime##BITS##_" + c in text and re.search(r"\b(void|size_t) %s\(" % c, text), c


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime32, P30, 4)])
def test_workspace_bytes_is_the_formula_of_the_header(mod, p, wb):
    def up(x):
        return (x + 255) & ~255

    for n, L, k, levels, g, batch in ((32, 0, 1, 1, 1, 1), (1024, 720, 1, 2, 3, 37), (4096, 12, 2, 3, 4, 5)):
        plan = mod.Plan.try_new(n, p)
        pb = batch * (k + 1) * n * wb
        want = up(pb * levels) + up((L + 1) * batch * 4) + up(pb)
        assert plan.multibit_pbs_workspace_bytes(L, k, levels, g, batch) == want == plan.pbs_workspace_bytes(L, k, levels, batch)
    assert getattr(cntt.lib(), "cntt_prime%d_multibit_pbs_workspace_bytes" % (8 * wb))(None, 4, 1, 2, 2, 3) == 0
    grid = cntt.lib().cntt_prime_multibit_grid
    assert grid(0) == 1 and grid(256) == 1 and grid(257) == 2 and grid(1 << 40) == grid(1 << 50)


def refusal(plan, call, first, lwe_dim, base_log, levels, grouping, key=16, workspace=None, workspace_bytes=0, where=MEM_HOST, glwe_dim=1):
    """The message of a refused blind rotation (`first`: acc) or bootstrap (`first`: lwe_out) at the C ABI with batch = 1;
    the other pointers are never read: every refusal asked for here comes before the first device call and the first host read."""
    fn, p = plan._fn("multibit_" + call), ctypes.c_void_p
    args = (p(first), p(16), 0, p(16)) if call == "blind_rotate_batch" else (p(first), p(16), p(16), 0)
    rc = fn(plan._h, *args, p(key), lwe_dim, glwe_dim, base_log, levels, grouping, 1, p(workspace), workspace_bytes, where, None)
    assert rc == EINVAL
    return last_error()


@pytest.mark.parametrize("call", ["blind_rotate_batch", "bootstrap_batch"])
@pytest.mark.parametrize("mod,p,bits", [(prime64, P62, 62), (prime32, P30, 30)])
def test_which_refusal_wins_when_two_arguments_are_wrong(mod, p, bits, call):
    """The order of the checks of multibit_host.hpp, which the native plans share (test_native_multibit_abi.py has the same cases): the
    grouping before the divisibility of lwe_dim and before the key, the digit budget before the workspace."""
    plan = mod.Plan.try_new(32, p)
    assert refusal(plan, call, 16, 4, 4, 2, 5) == "grouping = 5 is not in 1 ... 4"
    assert refusal(plan, call, 16, 4, 4, 2, 0, key=None) == "grouping = 0 is not in 1 ... 4"
    assert refusal(plan, call, 16, 4, bits // 2 + 1, 2, 2, workspace=8, workspace_bytes=1 << 20) == \
        "base_log * levels = %d * 2 exceeds the bit length %d of the modulus" % (bits // 2 + 1, bits)


def test_blind_rotation_takes_a_workspace_of_the_unrounded_digits():
    """cntt_prime_multibit.h: the blind rotation needs the digits alone, batch * (glwe_dim + 1) * n * sizeof(word) * levels bytes, NOT
    rounded up to 256.  A device workspace of exactly that size passes the workspace check (the next refusal, the NULL acc, is the one
    reported) and one byte less does not.  The shape: the smallest plan, n = 32 of prime32, batch 1, levels 1.  With glwe_dim = 1 the
    digits take 8 n bytes, a multiple of 256 at every n a plan accepts (n >= 32), so that shape cannot tell the two sizes apart;
    glwe_dim = 2 is the nearest one that can: 384 bytes against 512."""
    assert prime32.Plan.try_new(16, P30) is None
    plan, glwe_dim = prime32.Plan.try_new(32, P30), 2
    need = 1 * (glwe_dim + 1) * 32 * 4 * 1
    assert need % 256 == 128 and plan.multibit_pbs_workspace_bytes(4, glwe_dim, 1, 2, 1) > 512
    ws = dict(workspace=4096, where=MEM_DEVICE, glwe_dim=glwe_dim)
    assert refusal(plan, "blind_rotate_batch", None, 4, 4, 1, 2, workspace_bytes=need, **ws) == "acc is NULL"
    assert refusal(plan, "blind_rotate_batch", None, 4, 4, 1, 2, workspace_bytes=need - 1, **ws) == \
        "workspace_bytes = %d is below the %d bytes this call needs" % (need - 1, need)


def test_kernel_instances_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit: prime_multibit_accumulate_kernel on u32 and u64 words, two kernels, neither with a
    private segment or a spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_multibit.o")
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
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        seen.append(name)
    assert len(seen) == 2, seen
    assert sum("prime_multibit_accumulate_kernelIjE" in s for s in seen) == 1, seen
    assert sum("prime_multibit_accumulate_kernelImE" in s for s in seen) == 1, seen
