"""C ABI of the prime plans' ring packing (include/cntt_prime_ring_pack.h): the header is plain C11 on its own and includes
cntt_prime_automorphism.h itself, its names are the five per word width plus the grid function, all are exported, every CNTT_EINVAL case
is refused on host buffers by the argument checks that precede any device call (output poison intact, argument named), the workspace
sizes are the header's formulas, the grid rule is what the header says, the Python wrappers panic on bad shapes, and the code object of
the new unit has its kernels without scratch or spills.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64
from concrete_ntt_amd._lib import EINVAL, Panic
from prime_ring_pack_model import HEADER, grid, merge_workspace_bytes, ring_pack_workspace_bytes
from test_prime_automorphism_abi import Raw, declarations, err, ptr
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["glwe_embed_batch", "glwe_merge_batch", "glwe_merge_workspace_bytes", "ring_pack_batch", "ring_pack_workspace_bytes"]
GRID = "cntt_prime_ring_pack_grid"
NEW = {"cntt_prime%d_%s" % (bits, c) for bits in (32, 64) for c in CALLS} | {GRID}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert len(NEW) == 11 and set(decl) == NEW and len(decl) == 11
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_prime_automorphism.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "message j sits at coefficient j n / M, NOT at coefficient j" in flat and "the factor is n for every M" in flat
    assert "glwe[q][i] = -lwe[q n + n - i] mod p" in flat and "shift = n / 2^s, t = 2^s + 1" in flat
    assert "up(batch H k levels n sizeof(T)) + up(batch H (k + 1) n sizeof(T)) + up(batch Q (k + 1) n sizeof(T))" in flat
    for name in ("cntt.h", "cntt_ext.h", "cntt_prime_automorphism.h"):
        other = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        assert "cntt_prime_ring_pack.h" not in other and not (NEW & set(declarations(os.path.join(ROOT, "include", name)))), name


def test_library_exports_the_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit, read the way tests/test_native_multibit_abi.py reads its unit: the embedding x two word
    types, the merge x two word types x streaming or not x staged or not x GLWE sources or LWE leaves, none with a private segment or a
    spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "prime_ring_pack.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "ring.fat"), str(tmp_path / "ring.co")
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
    assert len(seen) == 18, seen
    for word in ("Ij", "Im"):
        assert sum(("4cntt23prime_glwe_embed_kernel" + word) in s for s in seen) == 1, (word, seen)
        assert sum(("4cntt23prime_ring_merge_kernel" + word + "Lb") in s for s in seen) == 8, (word, seen)


@pytest.mark.parametrize("mod,p,wb", [(prime64, P62, 8), (prime64, PM64, 8), (prime32, P30, 4)])
def test_workspace_bytes_are_the_formulas_of_the_header(mod, p, wb):
    for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
        plan = mod.Plan.try_new(n, p)
        assert plan.glwe_merge_workspace_bytes(k, levels, batch) == merge_workspace_bytes(n, wb, k, levels, batch)
        for m in (1, 2, 4, 8, n):
            assert plan.ring_pack_workspace_bytes(m, k, levels, batch) == ring_pack_workspace_bytes(n, wb, m, k, levels, batch), (n, m, k)
    # the three parts, spelled out once: M = 8 at n = 32, k = 1, levels = 3, batch = 5 on 8-byte words -> H = 4, Q = 2
    if wb == 8:
        assert mod.Plan.try_new(32, p).ring_pack_workspace_bytes(8, 1, 3, 5) == 5 * 4 * 3 * 32 * 8 + 5 * 4 * 2 * 32 * 8 + 5 * 2 * 2 * 32 * 8
    L = cntt.lib()
    assert getattr(L, "cntt_prime%d_glwe_merge_workspace_bytes" % (8 * wb))(None, 1, 2, 3) == 0
    assert getattr(L, "cntt_prime%d_ring_pack_workspace_bytes" % (8 * wb))(None, 4, 1, 2, 3) == 0


def test_grid_rule():
    """one workgroup per output polynomial up to 8 per CU of a 256-CU part, fewer where the two staged polynomials limit what a CU holds"""
    g = cntt.lib().cntt_prime_ring_pack_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(2048, 10, 8) == 2048 and g(5000, 10, 8) == 2048
    assert g(5000, 5, 4) == 2048                       # small polynomials: the wave cap
    assert g(5000, 11, 8) == 5 * 256                   # 2 x 16 KiB staged: five per CU
    assert g(5000, 12, 8) == 2 * 256                   # 2 x 32 KiB staged: two per CU
    assert g(5000, 13, 8) == 2048 and g(5000, 14, 4) == 2048   # past the LDS limit: the global gather, the wave cap again
    assert g(5000, 13, 4) == 2 * 256
    for polys in (0, 1, 300, 5000):
        for logn in (4, 5, 10, 11, 12, 13, 14):
            for w in (4, 8):
                assert g(polys, logn, w) == grid(polys, logn, w), (polys, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, M = 32, 1, 2, 3, 4
LOGN = 5
POISON = 7


class Case:
    """Valid host arguments at n = 32: k = 1, levels = 3, 2 pairs of GLWE ciphertexts, 2 x 4 LWE ciphertexts, the five trace keys; the
    output filled with 7."""

    def __init__(self, bits=64, p=P62):
        self.bits, self.p = bits, p
        self.dtype = np.uint64 if bits == 64 else np.uint32
        self.plan = (prime64 if bits == 64 else prime32).Plan.try_new(N, p)
        self.even = np.arange(B * (K + 1) * N, dtype=self.dtype)
        self.odd = np.arange(B * (K + 1) * N, dtype=self.dtype) + 3
        self.lwe = np.arange(B * M * (K * N + 1), dtype=self.dtype)
        self.out = np.full(B * (K + 1) * N, POISON, dtype=self.dtype)
        self.key = np.zeros(LOGN * K * LEVELS * (K + 1) * N, dtype=self.dtype)
        self.ws = np.zeros(self.plan.ring_pack_workspace_bytes(M, K, LEVELS, B), dtype=np.uint8)

    def fn(self, name):
        return getattr(cntt.lib(), "cntt_prime%d_%s" % (self.bits, name))

    def pick(self, **kw):
        return {k: (getattr(self, k) if isinstance(v, str) else v) for k, v in kw.items()}

    def embed(self, plan="own", out="own", lwe="own", k=K, batch=B * M):
        a = self.pick(out=out, lwe=lwe)
        return self.fn("glwe_embed_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), k, batch, 0, None)

    def merge(self, plan="own", out="own", even="own", odd="own", key="own", shift=5, t=3, k=K, base_log=4, levels=LEVELS, batch=B, ws=None,
              ws_bytes=None):
        a = self.pick(out=out, even=even, odd=odd, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("glwe_merge_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["even"]), ptr(a["odd"]), ptr(a["key"]), shift,
                                           t, k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def pack(self, plan="own", out="own", lwe="own", key="own", m=M, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, lwe=lwe, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return self.fn("ring_pack_batch")(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), ptr(a["key"]), m, k, base_log, levels,
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
    merge_ws = c.plan.glwe_merge_workspace_bytes(K, LEVELS, B)

    def refused(call, kw, word):
        assert call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw

    # call 1
    emb_out = np.full(B * M * (K + 1) * N, POISON, dtype=c.dtype)
    for kw, word in [(dict(plan=None), "plan"), (dict(out=None), "glwe_out is NULL"), (dict(lwe=None), "lwe_in is NULL"),
                     (dict(out=big[:emb_out.size], lwe=big[8:8 + c.lwe.size]), "glwe_out overlaps lwe_in"),
                     (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"), (dict(out=Raw(emb_out.ctypes.data + 1)), "glwe_out is not"),
                     (dict(k=(1 << 32) - 1), "glwe_dim"), (dict(k=(1 << 64) - 1), "glwe_dim"), (dict(batch=1 << 56, k=1), "2^63 bytes")]:
        refused(lambda **a: c.embed(**{"out": emb_out, **a}), kw, word)
        assert (emb_out == POISON).all()
    # what calls 2 and 3 share with the Galois keyswitch
    shared = [
        (dict(plan=None), "plan"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the bit length"),
        (dict(out=None), "glwe_out is NULL"),
        (dict(key=None), "ak_ntt is NULL"),
        (dict(out=out_in_big, key=big[8:8 + c.key.size]), "glwe_out overlaps ak_ntt"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(key=big[:c.key.size], ws=ws_in_big), "workspace overlaps ak_ntt"),
        (dict(key=Raw(c.key.ctypes.data + w // 2)), "ak_ntt is not"),
        (dict(ws=odd[off:off + c.ws.nbytes]), "aligned"),
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
    ]
    # call 2
    for kw, word in shared + [
            (dict(k=1 << 31, levels=1, batch=1), "2^63 bytes"),
            (dict(t=0), "t = 0"), (dict(t=6), "t = 6"), (dict(t=2 * N), "below 2n"), (dict(t=2 * N + 1), "odd exponent below 2n"),
            (dict(shift=2 * N), "shift = %d" % (2 * N)), (dict(shift=1 << 40), "shift"),
            (dict(even=None), "glwe_even is NULL"), (dict(odd=None), "glwe_odd is NULL"),
            (dict(out=out_in_big, even=big[8:8 + c.even.size]), "glwe_out overlaps glwe_even"),
            (dict(out=out_in_big, odd=big[8:8 + c.odd.size]), "glwe_out overlaps glwe_odd"),
            (dict(even=big[:c.even.size], ws=ws_in_big), "workspace overlaps glwe_even"),
            (dict(odd=big[:c.odd.size], ws=ws_in_big), "workspace overlaps glwe_odd"),
            (dict(even=Raw(c.even.ctypes.data + 1)), "glwe_even is not"), (dict(odd=Raw(c.odd.ctypes.data + 1)), "glwe_odd is not"),
            (dict(ws=c.ws, ws_bytes=merge_ws - 1), "workspace_bytes"),
            (dict(batch=(1 << 32) // LEVELS + 1), "2^32"), (dict(batch=1 << 32, k=0, key=None), "2^32")]:
        refused(c.merge, kw, word)
    # call 3
    for kw, word in shared + [
            (dict(k=1 << 31, levels=1, batch=1, m=1), "2^63 bytes"),                 # H = 1: the launch bound passes, the keys do not fit
            (dict(m=0), "lwe_count = 0"), (dict(m=3), "lwe_count = 3"), (dict(m=12), "lwe_count = 12"), (dict(m=2 * N), "lwe_count = %d" % (2 * N)),
            (dict(lwe=None), "lwe_in is NULL"),
            (dict(out=out_in_big, lwe=big[8:8 + c.lwe.size]), "glwe_out overlaps lwe_in"),
            (dict(lwe=big[:c.lwe.size], ws=ws_in_big), "workspace overlaps lwe_in"),
            (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"),
            (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=merge_ws), "workspace_bytes"),
            # batch * H * max(k * levels, k + 1) >= 2^32 with H = M / 2 = 2: half the batch of call 2 is refused already
            (dict(batch=(1 << 32) // (2 * LEVELS) + 1), "2^32"), (dict(batch=1 << 31, k=0, key=None), "2^32"),
            (dict(batch=(1 << 32) // LEVELS + 1, m=1), "2^32")]:
        refused(c.pack, kw, word)


@pytest.mark.parametrize("bits,p", [(64, PM64), (32, P30)])
def test_batch_zero_does_nothing_and_keyless_calls_need_no_key(bits, p):
    c = Case(bits, p)
    assert c.fn("glwe_embed_batch")(c.plan._h, None, None, K, 0, 0, None) == 0
    assert c.fn("glwe_merge_batch")(c.plan._h, None, None, None, None, 5, 3, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.fn("ring_pack_batch")(c.plan._h, None, None, None, M, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.embed(batch=0) == 0 and c.merge(batch=0) == 0 and c.pack(batch=0) == 0 and c.untouched()
    # k = 0 with a NULL key passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    body = np.arange(B * N, dtype=c.dtype)
    out = np.zeros(B * N, dtype=c.dtype)
    assert c.merge(k=0, key=None, even=body, odd=body + 1, out=out) != EINVAL
    assert c.pack(k=0, key=None, lwe=np.arange(B * M, dtype=c.dtype), out=out) != EINVAL
    # every valid lwe_count passes, with the workspace of its own formula
    for m in (1, 2, 4, 8, 16, 32):
        ws = np.zeros(c.plan.ring_pack_workspace_bytes(m, K, LEVELS, 1), dtype=np.uint8)
        assert c.pack(m=m, batch=1, lwe=np.zeros(m * (K * N + 1), dtype=c.dtype), out=np.zeros((K + 1) * N, dtype=c.dtype), ws=ws) != EINVAL, m


@pytest.mark.parametrize("mod,p", [(prime64, P62), (prime32, P30)])
def test_python_wrappers_panic_on_bad_shapes(mod, p):
    c = Case(64 if mod is prime64 else 32, p)
    pl = c.plan
    one_key = c.key[:c.key.size // LOGN]
    emb_out = np.zeros(B * M * (K + 1) * N, dtype=c.dtype)
    for args in [(emb_out[:-1], c.lwe, K), (emb_out, c.lwe[:-1], K), (emb_out, c.lwe, K + 1), (emb_out, c.lwe, -1)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_embed_batch(*args)
    for args in [(c.out[:-N], c.even, c.odd, one_key, 5, 3, K, 4, LEVELS), (c.out, c.even, c.odd[:-N], one_key, 5, 3, K, 4, LEVELS),
                 (c.out, c.even, c.odd, one_key[:-N], 5, 3, K, 4, LEVELS), (c.out, c.even, c.odd, one_key, 5, 3, K, 4, LEVELS + 1),
                 (c.out, c.even, c.odd, one_key, -1, 3, K, 4, LEVELS), (c.out, c.even, c.odd, one_key, 2 * N, 3, K, 4, LEVELS),
                 (c.out, c.even, c.odd, one_key, 5, 2, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_merge_batch(*args)
    for args in [(c.out[:-N], c.lwe, c.key, M, K, 4, LEVELS), (c.out, c.lwe[:-1], c.key, M, K, 4, LEVELS), (c.out, c.lwe, one_key, M, K, 4, LEVELS),
                 (c.out, c.lwe, c.key, 0, K, 4, LEVELS), (c.out, c.lwe[:B * 3 * (K * N + 1)], c.key, 3, K, 4, LEVELS),
                 (c.out, c.lwe, c.key, M, K, 0, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.ring_pack_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.ring_pack_batch(c.out, c.lwe, c.key, M, K, 4, LEVELS, workspace=c.ws[:255])
    for fn, args in ((pl.glwe_merge_workspace_bytes, (K, LEVELS, -1)), (pl.glwe_merge_workspace_bytes, (K, 0, 1)),
                     (pl.ring_pack_workspace_bytes, (0, K, LEVELS, 1)), (pl.ring_pack_workspace_bytes, (M, K, LEVELS, -1))):
        with pytest.raises(Panic):
            fn(*args)
    assert c.untouched()
