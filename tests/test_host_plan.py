"""CPU-only checks of the product's host side: plan construction (its own number theory, separate
code from the oracle) against the golden vectors and the oracle, the C-ABI surface, error mapping.
No compute entry point is called here (they need a GPU and have no fallback)."""
import ctypes
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import _lib, prime32, prime64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _mod(bits):
    return prime64 if bits == 64 else prime32


def test_library_exports_every_declared_symbol():
    hdr = os.path.join(ROOT, "include", "cntt.h")
    pre = subprocess.run(["gcc", "-E", "-P", hdr], check=True, capture_output=True, text=True).stdout
    names = sorted(set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", pre)))
    assert len(names) >= 59
    L = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_plans_match_golden(golden):
    for ent in golden["plans"]:
        pl = _mod(ent["bits"]).Plan.try_new(ent["n"], ent["p"])
        assert pl is not None
        info = pl.info()
        assert (info.ntt_size, info.modulus, info.root) == (ent["n"], ent["p"], ent["w"])
        assert (info.n_inv_mod_p, info.big_q, bool(info.has_shoup)) == (ent["n_inv"], ent["big_q"], ent["has_shoup"])
        assert pl.table(_lib.TWID)[:8].tolist() == ent["twid_head"]
        assert sha(pl.table(_lib.TWID)) == ent["twid_sha256"]
        assert sha(pl.table(_lib.INV_TWID)) == ent["inv_twid_sha256"]
        if ent["has_shoup"]:
            assert (info.n_inv_mod_p_shoup, info.p_barrett) == (ent["n_inv_shoup"], ent["p_barrett"])
            assert pl.table(_lib.TWID_SHOUP)[:8].tolist() == ent["twid_shoup_head"]
            assert pl.table(_lib.INV_TWID_SHOUP)[:8].tolist() == ent["inv_twid_shoup_head"]
            assert sha(pl.table(_lib.TWID_SHOUP)) == ent["twid_shoup_sha256"]
        else:
            assert pl.table(_lib.TWID_SHOUP) is None
        assert pl.ntt_size() == ent["n"] and pl.modulus() == ent["p"]


@pytest.mark.parametrize("bits,n,p", [(64, 4096, 4611686018427322369), (64, 2048, 18446744069414584321),
                                      (64, 1024, 1125899904679937), (64, 32768, 1125899904679937),
                                      (64, 2048, 2251799813554177),
                                      (64, 512, 9223372036853661697), (32, 8192, 1073479681),
                                      (32, 256, 4293918721), (32, 2048, 2147352577)])
def test_plans_match_oracle(oracle, bits, n, p):
    pl = _mod(bits).Plan.try_new(n, p)
    ref = oracle.Plan.try_new(n, p, bits)
    for which, name in ((_lib.TWID, "twid"), (_lib.TWID_SHOUP, "twid_shoup"), (_lib.INV_TWID, "inv_twid"),
                        (_lib.INV_TWID_SHOUP, "inv_twid_shoup")):
        a, b = pl.table(which), ref.table(name)
        assert (a is None) == (b is None)
        if a is not None:
            assert np.array_equal(a, b), name
    info = pl.info()
    assert (info.n_inv_mod_p, info.big_q) == (ref.n_inv_mod_p, ref.big_q)
    if info.has_shoup:
        assert (info.n_inv_mod_p_shoup, info.p_barrett) == (ref.n_inv_mod_p_shoup, ref.p_barrett)
    expect_cls = 0 if p < (1 << (bits - 2)) else (1 if p < (1 << (bits - 1)) else 2)
    if bits == 64 and p < (1 << 51) and n <= 16384:
        expect_cls = 3 if p < (1 << 50) else 4   # double-precision FMA butterflies (csrc/ntt_arith.hpp, CLS_FP / CLS_FP51)
    if bits == 64 and p >= (1 << 63) and (1 << 64) - p < (1 << 32) and n <= 16384:
        expect_cls = 5   # p = 2^64 - c, c < 2^32 (CLS_PM64)
    if bits == 32 and p >= (1 << 31) and n <= 16384:
        expect_cls = 6   # 32-bit words on double-precision butterflies (CLS_FPW)
    assert info.arith_class == expect_cls


def test_try_new_none_and_panics(golden):
    for c in golden["try_new_none"]:
        assert _mod(c["bits"]).Plan.try_new(c["n"], c["p"]) is None, c
    for m in (prime64, prime32):
        for p in (0, 1):
            with pytest.raises(cntt.Panic):
                m.Plan.try_new(64, p)
    # test_plan_crash_github_11: src/prime64.rs:1879-1882
    assert prime64.Plan.try_new(2048, 1024) is None


def test_native_plans_host_side():
    from concrete_ntt_amd import native32, native64, native128, native_binary32, native_binary64, native_binary128
    kinds = [(native32.Plan32, 3, 4), (native64.Plan32, 5, 4), (native128.Plan32, 10, 4),
             (native_binary32.Plan32, 2, 4), (native_binary64.Plan32, 3, 4), (native_binary128.Plan32, 5, 4),
             (native32.Plan52, 2, 8), (native64.Plan52, 3, 8), (native_binary32.Plan52, 1, 8),
             (native_binary64.Plan52, 2, 8)]
    p32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801, 1068433409, 1068564481, 1069219841,
           1071513601, 1073479681]  # src/lib.rs:453-462
    p52 = [1125899881086977, 1125899885412353, 1125899886395393]  # src/lib.rs:601-603
    for cls, k, res in kinds:
        pl = cls.try_new(256)
        assert pl is not None and pl.ntt_size() == 256
        assert _lib.lib().cntt_native_nprimes(pl._h) == k
        for i in range(k):
            sub = pl.ntt(i)
            assert sub.ntt_size() == 256 and sub.modulus() == (p52 if res == 8 else p32)[i]
        assert pl.ntt(k) is None
        assert cls.try_new(16) is None or res == 8      # prime32 needs n >= 32, prime64 n >= 16
        assert cls.try_new(1 << 17) is None             # the primes are 1 mod 2^17 only
        assert cls.try_new(48) is None


def test_ew_grid_stays_below_the_dispatch_limit():
    """Grid of the element-wise kernels (fill, split, CRT, pointwise, global stages): one 256-thread block per 256 work items, but
    never more than a dispatch can hold -- 2^32 - 1 work-items per dimension, i.e. fewer than 2^24 blocks (the
    round-3 cap of 2^30 blocks made every launch over 2^32 items fail with hipErrorInvalidConfiguration; 16 GiB of u32 is a
    plausible fill on a 288 GB part).  The kernels are grid-stride with 64-bit indices, so the capped grid covers any count."""
    import ctypes
    f = cntt.lib().cntt_ew_grid
    f.restype, f.argtypes = ctypes.c_uint, [ctypes.c_size_t]
    for count in (1, 255, 256, 257, 65536 * 1024, (2**24 - 1) * 256, (2**24 - 1) * 256 + 1, 2**32 - 1, 2**32, 2**32 + 1, 2**34, 2**36,
                  2**40):
        g = f(count)
        assert 1 <= g <= 2**24 - 1 and g * 256 <= 2**32 - 1, (count, g)
        if count <= (2**24 - 1) * 256:
            assert g == (count + 255) // 256, (count, g)


def test_no_gpu_means_loud_failure():
    if cntt.device_count() > 0:
        pytest.skip("a GPU is present")
    pl = prime64.Plan.try_new(64, 4611686018427322369)
    with pytest.raises(cntt.DeviceError):
        pl.fwd(np.zeros(64, dtype=np.uint64))


def test_length_assert_is_a_panic():
    pl = prime32.Plan.try_new(64, 1062862849)
    with pytest.raises(cntt.Panic):  # assert_eq!(buf.len(), self.ntt_size()): src/prime32.rs:710
        pl.fwd(np.zeros(32, dtype=np.uint32))
    with pytest.raises(cntt.Panic):
        pl.inv(np.zeros(128, dtype=np.uint32))


def test_async_load_kernels_do_not_spill(tmp_path):
    """The persistent kernels prefetch with inline-asm global loads (csrc/ntt_kernel.hpp gather_async, csrc/ntt_blk.hpp
    Pf::issue): a register the compiler spills or reassigns while such a load is in flight would be overwritten when the
    data lands.  Read the gfx950 code objects of the units that use them and require zero spills and zero scratch in every
    persistent kernel -- except shapes compiled WITHOUT the prefetch for exactly that reason (mul_kernel_blk<..., PREFETCH =
    false>, ordinary loads only: none in the current build, ntt_mul_one.hpp).
    The objects are part of the build: their absence fails (a rebuild with another compiler must not skip this)."""
    import re
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        # a box without the ROCm toolchain cannot read the code objects: skip THERE -- wherever the tools exist
        # (the build image, the GPU box) missing objects still fail below; CNTT_REQUIRE_CODE_OBJECTS=1 turns the skip into a failure
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    objdir = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj")
    checked, exempt = 0, 0
    for unit in ("ntt_inst_u64_fwd", "ntt_inst_u64_inv", "ntt_inst_u32_fwd", "ntt_inst_u32_inv", "ntt_inst_u64_mul",
                 "ntt_inst_u32_mul", "ntt_inst_u64_fp", "ntt_inst_u64_fp51", "ntt_inst_u64_pm"):
        obj = os.path.join(objdir, unit + ".o")
        assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
        fat, co = str(tmp_path / (unit + ".fat")), str(tmp_path / (unit + ".co"))
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True,
                               text=True).stdout
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "_wp" not in name and "_blk" not in name:
                continue
            spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            if re.search(r"mul_kernel_blk.*Lb0EEEv", name):   # <..., PREFETCH = false>
                exempt += 1
                continue
            assert spills == 0 and scratch == 0, (name, spills, scratch)
            checked += 1
    assert checked > 80 and exempt <= 6, (checked, exempt)
    shutil.rmtree(str(tmp_path), ignore_errors=True)


def _build_examples():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)


def test_c_examples_build_and_fail_loudly_without_gpu():
    """The C ABI is plain C (gcc -std=c11 -pedantic on examples/*.c), include/cntt.hpp is plain C++17, and there is no CPU path: without a GPU the
    first compute call returns CNTT_EDEVICE and the program says so."""
    _build_examples()
    import torch
    if torch.cuda.is_available() or cntt.device_count() > 0:
        pytest.skip("GPU present: covered by test_c_examples_run_on_gpu")
    for name, needle in (("mul_poly_prime", "status 4"), ("mul_poly_native", "status 4"), ("readme_example", "device error")):
        r = subprocess.run([os.path.join(ROOT, "examples", name)], capture_output=True, text=True)
        assert r.returncode == 1 and needle in r.stderr, (name, r.returncode, r.stderr)


@pytest.mark.gpu
def test_c_examples_run_on_gpu():
    """examples/mul_poly_prime.c and mul_poly_native.c (the reference's examples/*.rs through the C ABI) and the
    README example + a product::Plan round trip through the C++17 mirror include/cntt.hpp."""
    _build_examples()
    for name in ("mul_poly_prime", "mul_poly_native", "readme_example"):
        r = subprocess.run([os.path.join(ROOT, "examples", name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "Success!" in r.stdout, (name, r.returncode, r.stdout, r.stderr)


# ---- the aliasing and alignment contract of the core _batch calls (include/cntt.h, "Operands") ----------------------------------------------
# Refusals are pointer comparisons made before any device call, so they are CNTT_EINVAL with or without a GPU and leave every buffer as it
# was; a permitted call goes on to the device and returns CNTT_OK with one and CNTT_EDEVICE without -- never CNTT_EINVAL.  The permitted
# calls run last (`later`): with a GPU they compute.
EINVAL, HOST = _lib.EINVAL, _lib.MEM_HOST


def _ptr(a):
    return a.ctypes.data


def _err():
    return _lib.last_error()


@pytest.mark.parametrize("bits,p", [(64, 4611686018427322369), (32, 1062862849)])
def test_prime_batch_overlaps_are_refused(bits, p):
    n, B, later = 32, 3, []
    L, pl = cntt.lib(), _mod(bits).Plan.try_new(32, p)
    f = lambda name: getattr(L, "cntt_prime%d_%s" % (bits, name))
    big = np.full(64 * n, 7, dtype=pl.dtype)
    before = big.copy()
    a, near, far, far2 = big[:B * n], big[n:n + B * n], big[8 * n:8 * n + B * n], big[16 * n:16 * n + B * n]
    for name, second in (("mul_assign_normalize_batch", "rhs"), ("mul_ntt_batch", "rhs_ntt")):
        assert f(name)(pl._h, _ptr(a), _ptr(near), B, HOST, None) == EINVAL and "lhs overlaps " + second in _err()
        assert f(name)(pl._h, _ptr(a), _ptr(a), B, HOST, None) == EINVAL and "lhs overlaps " + second in _err()
        later.append(lambda name=name: f(name)(pl._h, _ptr(a), _ptr(big[B * n:]), B, HOST, None))      # right behind it: no overlap
    assert f("mul_accumulate_batch")(pl._h, _ptr(a), _ptr(near), _ptr(far), B, HOST, None) == EINVAL and "acc overlaps lhs" in _err()
    assert f("mul_accumulate_batch")(pl._h, _ptr(a), _ptr(far), _ptr(near), B, HOST, None) == EINVAL and "acc overlaps rhs" in _err()
    # lhs and rhs are read only: the same buffer, or overlapping ones, are permitted (mul_accumulate(acc, x, x), as the reference allows)
    later.append(lambda: f("mul_accumulate_batch")(pl._h, _ptr(a), _ptr(far), _ptr(far), B, HOST, None))
    later.append(lambda: f("mul_accumulate_batch")(pl._h, _ptr(a), _ptr(far), _ptr(big[9 * n:]), B, HOST, None))
    J, O = 2, 2
    out, terms, key = big[:B * O * n], big[20 * n:20 * n + B * J * n], big[40 * n:40 * n + J * O * n]
    ext = f("external_product_batch")
    assert ext(pl._h, _ptr(out), _ptr(big[B * O * n - 1:]), _ptr(key), J, O, B, 0, HOST, None) == EINVAL and "out overlaps terms" in _err()
    assert ext(pl._h, _ptr(out), _ptr(terms), _ptr(big[n:]), J, O, B, 1, HOST, None) == EINVAL and "out overlaps key_ntt" in _err()
    later.append(lambda: ext(pl._h, _ptr(out), _ptr(terms), _ptr(terms), J, O, B, 0, HOST, None))   # terms and key_ntt: both read only
    # nterms = 0: terms and key_ntt are not read and may be anything
    later.append(lambda: ext(pl._h, _ptr(out), _ptr(out), _ptr(out), 0, O, B, 1, HOST, None))
    # below the word's alignment
    raw = np.zeros(B * n * pl.dtype().itemsize + 16, dtype=np.uint8)
    off = (bits // 16 - raw.ctypes.data) % 16          # an address that is half a word past a 16-byte boundary
    assert f("fwd_batch")(pl._h, raw.ctypes.data + off, B, HOST, None) == EINVAL and "bufs is not %d-byte aligned" % (bits // 8) in _err()
    assert f("normalize_batch")(pl._h, raw.ctypes.data + off, B, HOST, None) == EINVAL and "values is not" in _err()
    assert np.array_equal(big, before)                      # a refused call touches nothing
    assert all(call() != EINVAL for call in later)


def test_native_batch_overlaps_are_refused():
    from concrete_ntt_amd import native64, native128
    n, B, later = 32, 2, []
    L, pl = cntt.lib(), native64.Plan32.try_new(32)
    k = pl.NPRIMES
    val = np.full(16 * n, 5, dtype=np.uint64)
    res = np.full(64 * n, 9, dtype=np.uint32)
    vb, rb = val.copy(), res.copy()
    planes = [res[i * B * n:(i + 1) * B * n] for i in range(k)]
    arr = lambda ps: (ctypes.c_void_p * k)(*[_ptr(q) for q in ps])
    for fn in (L.cntt_native_fwd_batch, L.cntt_native_inv_batch):
        later.append(lambda fn=fn: fn(pl._h, _ptr(val), arr(planes), B, HOST, None))
        bad = list(planes)
        bad[3] = res[2 * B * n + 1:2 * B * n + 1 + B * n]          # plane 3 one word into plane 2
        assert fn(pl._h, _ptr(val), arr(bad), B, HOST, None) == EINVAL and "residues[2] overlaps residues[3]" in _err()
        bad = list(planes)
        bad[0] = val[:B * n // 2].view(np.uint32)                  # plane 0 on top of the value
        assert fn(pl._h, _ptr(val), arr(bad), B, HOST, None) == EINVAL and "overlaps" in _err() and "value" in _err()
    assert "value overlaps residues[0]" in _err()                  # inv writes both; fwd, which only reads the value, names the plane first
    bad = list(planes)
    bad[0] = val[:B * n // 2].view(np.uint32)
    assert L.cntt_native_fwd_batch(pl._h, _ptr(val), arr(bad), B, HOST, None) == EINVAL and "residues[0] overlaps value" in _err()
    a, b, c = val[:B * n], val[4 * n:4 * n + B * n], val[8 * n:8 * n + B * n]
    mul = L.cntt_native_negacyclic_polymul_batch
    assert mul(pl._h, _ptr(a), _ptr(val[n:]), _ptr(c), B, HOST, None) == EINVAL and "prod overlaps lhs" in _err()
    assert mul(pl._h, _ptr(a), _ptr(b), _ptr(a), B, HOST, None) == EINVAL and "prod overlaps rhs" in _err()
    later.append(lambda: mul(pl._h, _ptr(a), _ptr(b), _ptr(b), B, HOST, None))      # negacyclic_polymul(prod, a, a): permitted
    # u128 words are 16-byte aligned
    p128 = native128.Plan32.try_new(32)
    raw = np.zeros(3 * (n * 16) + 32, dtype=np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 16
    q = [base + 8, base + 16 + n * 16, base + 16 + 2 * n * 16]
    assert mul(p128._h, q[0], q[1], q[2], 1, HOST, None) == EINVAL and "prod is not 16-byte aligned" in _err()
    assert np.array_equal(val, vb) and np.array_equal(res, rb)   # a refused call touches nothing
    assert all(call() != EINVAL for call in later)


def test_product_batch_overlaps_are_refused(oracle):
    from concrete_ntt_amd import product
    n, B, later = 32, 2, []
    lp = oracle.largest_prime_in_arithmetic_progression64
    p0 = lp(64, 1, 0, 2**30)
    primes = [lp(64, 1, 0, p0 - 1), p0]
    pl = product.Plan.try_new(n, primes[0] * primes[1], primes)
    L, dl = cntt.lib(), pl.ntt_domain_len()
    big = np.full(64 * n, 3, dtype=np.uint64)
    before = big.copy()
    ntt, std = big[:B * dl], big[16 * n:16 * n + B * n]
    assert L.cntt_product_fwd_batch(pl._h, _ptr(ntt), _ptr(big[B * dl - 1:]), B, 0, 0, HOST, None) == EINVAL and "ntt overlaps standard" in _err()
    later.append(lambda: L.cntt_product_fwd_batch(pl._h, _ptr(ntt), _ptr(std), B, 0, 0, HOST, None))
    for mode in (0, 1):   # inv writes both of its buffers
        assert L.cntt_product_inv_batch(pl._h, _ptr(big[1:]), _ptr(ntt), B, mode, HOST, None) == EINVAL and "standard overlaps ntt" in _err()
    a, b, c = ntt, big[20 * n:20 * n + B * dl], big[40 * n:40 * n + B * dl]
    assert L.cntt_product_mul_assign_normalize_batch(pl._h, _ptr(a), _ptr(a), B, HOST, None) == EINVAL and "lhs overlaps rhs" in _err()
    assert L.cntt_product_mul_accumulate_batch(pl._h, _ptr(a), _ptr(big[1:]), _ptr(c), B, HOST, None) == EINVAL and "acc overlaps lhs" in _err()
    assert L.cntt_product_mul_accumulate_batch(pl._h, _ptr(a), _ptr(b), _ptr(big[1:]), B, HOST, None) == EINVAL and "acc overlaps rhs" in _err()
    later.append(lambda: L.cntt_product_mul_accumulate_batch(pl._h, _ptr(a), _ptr(b), _ptr(b), B, HOST, None))
    J, O = 2, 2
    out, terms, key = big[:B * O * n], big[20 * n:20 * n + B * J * n], big[40 * n:40 * n + J * O * dl]
    ext = L.cntt_product_external_product_batch
    assert ext(pl._h, _ptr(out), _ptr(big[n:]), _ptr(key), J, O, B, 0, 0, 0, HOST, None) == EINVAL and "out overlaps terms" in _err()
    assert ext(pl._h, _ptr(out), _ptr(terms), _ptr(big[n:]), J, O, B, 0, 0, 1, HOST, None) == EINVAL and "out overlaps key_ntt" in _err()
    later.append(lambda: ext(pl._h, _ptr(out), _ptr(terms), _ptr(terms), J, O, B, 0, 0, 0, HOST, None))
    assert np.array_equal(big, before)                      # a refused call touches nothing
    assert all(call() != EINVAL for call in later)
