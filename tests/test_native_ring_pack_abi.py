"""C ABI of the native plans' ring packing (include/cntt_ring_pack.h), after tests/test_native_automorphism_abi.py: the header is plain C11
on its own and includes cntt_ext.h only, its names are the six it declares, all are exported, every CNTT_EINVAL case is refused
on host buffers by the argument checks that precede any device call (output poison intact, argument named; the kind refusals and
k * levels = max_terms + 1 included), the workspace sizes are the header's formulas, the grid rule is what the header says, and the Python
wrappers panic on bad shapes.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128, native_binary32, native_binary64
from concrete_ntt_amd._lib import EINVAL, Panic
from native_ring_pack_model import HEADER, grid, merge_workspace_bytes, ring_pack_workspace_bytes
from test_native_automorphism_abi import Raw, declarations, err, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
NEW = {"cntt_native_glwe_embed_batch", "cntt_native_glwe_merge_batch", "cntt_native_glwe_merge_workspace_bytes", "cntt_native_ring_pack_batch",
       "cntt_native_ring_pack_workspace_bytes", "cntt_native_ring_pack_grid"}


# -- the surface --------------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c11_on_its_own_and_declares_its_names():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    decl = declarations(HEADER)
    assert set(decl) == NEW and len(decl) == 6
    text = open(HEADER).read()
    assert re.findall(r'^#include "(.*)"$', text, flags=re.M) == ["cntt_ext.h"]
    flat = re.sub(r"[\s*]+", " ", text)
    assert "nterms = k levels, nout = k + 1, accumulate = 1" in flat and "stage s uses key r = log2 n - s" in flat
    assert "message j sits at coefficient j n / M" in flat and "the factor is n for every M" in flat
    assert "WHAT DIFFERS FROM THE PRIME PLANS" in flat and "n is NOT a unit mod 2^w" in flat and "headroom BELOW the message" in flat
    assert "grows by 2^(log2 n - 1 - i)" in flat and "a binary kind (calls 2 and 3)" in flat
    assert "profiles/r28_native_ring_pack.txt" in flat
    for name in sorted(os.listdir(INC)):
        if name == "cntt_ring_pack.h" or not name.endswith(".h"):
            continue
        raw = open(os.path.join(INC, name)).read()
        assert "cntt_ring_pack.h" not in raw and not (NEW & set(declarations(os.path.join(INC, name)))), name


def test_library_exports_exactly_the_six_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    c_names = set(re.findall(r"\s[TW]\s+(cntt_[a-z0-9_]+)$", syms, flags=re.M))
    assert NEW <= c_names
    assert {s for s in c_names if s.startswith("cntt_native_") and ("ring_pack" in s or "glwe_embed" in s or "glwe_merge" in s)} == NEW


@pytest.mark.parametrize("mod", [native32, native64, native128, native_binary64])
def test_workspace_bytes_are_the_formulas_of_the_header(mod):
    for P in (mod.Plan32, getattr(mod, "Plan52", None)):
        if P is None:
            continue
        for n, k, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 1, 3, 5), (256, 3, 4, 37), (2048, 2, 2, 1000), (64, 1, 7, 3)):
            plan = P.try_new(n)
            wb = plan.WORD
            assert plan.glwe_merge_workspace_bytes(k, levels, batch) == merge_workspace_bytes(n, wb, k, levels, batch)
            for m in (1, 2, 4, n // 2, n):
                assert plan.ring_pack_workspace_bytes(m, k, levels, batch) == ring_pack_workspace_bytes(n, wb, m, k, levels, batch), (n, m, k)
    wb = mod.Plan32.WORD
    plan = mod.Plan32.try_new(32)
    assert plan.ring_pack_workspace_bytes(8, 1, 3, 8) == 8 * 4 * 3 * 32 * wb + 8 * 4 * 2 * 32 * wb + 8 * 2 * 2 * 32 * wb
    assert plan.ring_pack_workspace_bytes(1, 1, 3, 8) == plan.ring_pack_workspace_bytes(2, 1, 3, 8) == 8 * 3 * 32 * wb + 2 * 8 * 2 * 32 * wb
    L = cntt.lib()
    assert L.cntt_native_glwe_merge_workspace_bytes(None, 1, 2, 3) == 0 and L.cntt_native_ring_pack_workspace_bytes(None, 4, 1, 2, 3) == 0


def test_grid_rule():
    g = cntt.lib().cntt_native_ring_pack_grid
    assert g(0, 10, 8) == 1 and g(1, 10, 8) == 1 and g(2047, 10, 8) == 2047 and g(5000, 10, 8) == 2048
    assert g(5000, 11, 16) == 512 and g(5000, 12, 16) == 2048                   # two polynomials of 32 KiB are staged, two pairs per CU; of 64 KiB not
    assert g(5000, 12, 8) == 512 and g(5000, 13, 4) == 512 and g(5000, 13, 8) == 2048 and g(5000, 14, 4) == 2048
    for polys in (0, 1, 300, 5000, 1 << 30):
        for logn in (4, 5, 10, 11, 12, 13, 14, 15):
            for w in (4, 8, 16):
                assert g(polys, logn, w) == grid(polys, logn, w), (polys, logn, w)


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B, LEVELS, M = 32, 1, 2, 3, 4
LOGN = 5
POISON = 7
KEY = K * LEVELS * (K + 1) * N


class Case:
    """Valid host arguments at n = 32: k = 1, levels = 3, batch 2, M = 4; all five trace keys as residue planes; the output filled with 7."""

    def __init__(self, P):
        self.plan = P.try_new(N)
        self.dtype, self.cw = self.plan.word_dtype, 2 if self.plan.WORD == 16 else 1
        self.pe = N * self.cw
        self.even = np.arange(B * (K + 1) * self.pe, dtype=self.dtype)
        self.odd = np.arange(B * (K + 1) * self.pe, dtype=self.dtype)
        self.lwe = np.arange(B * M * (K * N + 1) * self.cw, dtype=self.dtype)
        self.out = np.full(B * (K + 1) * self.pe, POISON, dtype=self.dtype)
        self.key = [np.zeros(LOGN * KEY, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.ws = np.zeros(self.plan.ring_pack_workspace_bytes(M, K, LEVELS, B), dtype=np.uint8)

    def planes(self, sel):
        if sel is None:
            return None
        return (ctypes.c_void_p * self.plan.NPRIMES)(*[None if p is None else ptr(p) for p in sel])

    def pick(self, **kw):
        return {k: (getattr(self, k) if isinstance(v, str) else v) for k, v in kw.items()}

    def embed(self, plan="own", out="own", lwe="own", k=K, batch=B):
        a = self.pick(out=out, lwe=lwe)
        return cntt.lib().cntt_native_glwe_embed_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), k, batch, 0, None)

    def merge(self, plan="own", out="own", even="own", odd="own", key="own", shift=5, t=3, k=K, base_log=4, levels=LEVELS, batch=B, ws=None,
              ws_bytes=None):
        a = self.pick(out=out, even=even, odd=odd, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_glwe_merge_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["even"]), ptr(a["odd"]),
                                                       self.planes(a["key"]), shift, t, k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def pack(self, plan="own", out="own", lwe="own", key="own", m=M, k=K, base_log=4, levels=LEVELS, batch=B, ws=None, ws_bytes=None):
        a = self.pick(out=out, lwe=lwe, key=key)
        wsb = (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes
        return cntt.lib().cntt_native_ring_pack_batch(self.plan._h if plan == "own" else None, ptr(a["out"]), ptr(a["lwe"]), self.planes(a["key"]), m,
                                                      k, base_log, levels, batch, ptr(ws), wsb, 0, None)

    def untouched(self):
        return bool((self.out == POISON).all())


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32, native64.Plan52], ids=["native64", "native32", "native128", "native64_plan52"])
def test_every_invalid_argument_is_refused(P):
    c = Case(P)
    W, w, rb = 8 * c.plan.WORD, c.plan.WORD, c.plan.RES
    big = np.full(16384, POISON, dtype=c.dtype)
    out_in_big = big[:c.out.size]
    ws_in_big = big.view(np.uint8)[16 * w:16 * w + c.ws.nbytes]
    plane_in_big = big.view(c.plan.res_dtype)[8 * w // rb:8 * w // rb + c.key[0].size]     # starts 8 words into `big`
    odd_ws = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd_ws.ctypes.data) % 16                                        # an address that is 4 mod 16
    mg_ws = c.plan.glwe_merge_workspace_bytes(K, LEVELS, B)
    last = c.plan.NPRIMES - 1

    def refused(call, kw, word):
        assert call(**kw) == EINVAL, kw
        assert word in err(), (kw, err())
        assert c.untouched() and (big == POISON).all(), kw

    def with_plane(planes, i, p):
        return planes[:i] + [p] + planes[i + 1:]

    # call 1
    for kw, word in [(dict(plan=None), "plan is NULL"), (dict(out=None), "glwe_out is NULL"), (dict(lwe=None), "lwe_in is NULL"),
                     (dict(out=out_in_big, lwe=big[8:8 + B * (K * N + 1) * c.cw]), "glwe_out overlaps lwe_in"),
                     (dict(out=Raw(c.out.ctypes.data + w // 2)), "glwe_out is not"), (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"),
                     (dict(k=(1 << 32) - 1), "glwe_dim"), (dict(k=(1 << 64) - 1), "glwe_dim"), (dict(batch=1 << 62), "2^63 bytes")]:
        refused(c.embed, kw, word)
    # calls 2 and 3
    shared = [
        (dict(plan=None), "plan is NULL"),
        (dict(base_log=0), "base_log is 0"),
        (dict(levels=0), "levels is 0"),
        (dict(base_log=W // 3 + 1, levels=3), "base_log * levels"),
        (dict(base_log=W, levels=2), "exceeds the word width %d" % W),
        (dict(out=None), "glwe_out is NULL"),
        (dict(key=None), "ak_ntt is NULL"),
        (dict(key=with_plane(c.key, last, None)), "NULL key residue plane (ak_ntt[%d])" % last),
        (dict(out=out_in_big, key=with_plane(c.key, 0, plane_in_big)), "glwe_out overlaps ak_ntt[0]"),
        (dict(out=out_in_big, ws=ws_in_big), "glwe_out overlaps workspace"),
        (dict(key=with_plane(c.key, last, plane_in_big), ws=ws_in_big), "workspace overlaps ak_ntt[%d]" % last),
        (dict(key=with_plane(c.key, 1 % c.plan.NPRIMES, Raw(c.key[0].ctypes.data + rb // 2))), "ak_ntt[%d] is not" % (1 % c.plan.NPRIMES)),
        (dict(out=Raw(c.out.ctypes.data + w // 2)), "glwe_out is not"),
        (dict(ws=odd_ws[off:off + c.ws.nbytes]), "workspace is not 16-byte aligned"),
        (dict(k=(1 << 32) - 1), "glwe_dim"),
        (dict(k=(1 << 64) - 1), "glwe_dim"),
        (dict(batch=1 << 63), "2^32"),
    ]
    merge_only = [
        (dict(t=0), "t = 0"), (dict(t=6), "t = 6"), (dict(t=2 * N), "t = 64"), (dict(t=(1 << 64) - 1), "t = "),
        (dict(shift=2 * N), "shift = 64"), (dict(shift=(1 << 64) - 1), "shift = "),
        (dict(even=None), "glwe_even is NULL"), (dict(odd=None), "glwe_odd is NULL"),
        (dict(out=out_in_big, even=big[8:8 + c.even.size]), "glwe_out overlaps glwe_even"),
        (dict(out=out_in_big, odd=big[8:8 + c.odd.size]), "glwe_out overlaps glwe_odd"),
        (dict(even=big[:c.even.size], ws=ws_in_big), "workspace overlaps glwe_even"),
        (dict(even=Raw(c.even.ctypes.data + 1)), "glwe_even is not"), (dict(odd=Raw(c.odd.ctypes.data + w // 2)), "glwe_odd is not"),
        (dict(ws=c.ws, ws_bytes=mg_ws - 1), "workspace_bytes"),
        # batch * max(k * levels, k + 1) >= 2^32 with H = 1
        (dict(batch=(1 << 32) // (K * LEVELS) + 1), "2^32"), (dict(batch=1 << 32, k=0, levels=1), "2^32"),
    ]
    for kw, word in shared + merge_only:
        refused(c.merge, kw, word)
    assert c.merge(out=c.even) == EINVAL and "glwe_out overlaps glwe_even" in err()      # no call runs in place
    pack_only = [
        (dict(m=0), "lwe_count = 0"), (dict(m=3), "lwe_count = 3"), (dict(m=2 * N), "lwe_count = 64"), (dict(m=(1 << 63)), "lwe_count"),
        (dict(lwe=None), "lwe_in is NULL"),
        (dict(out=out_in_big, lwe=big[8:8 + c.lwe.size]), "glwe_out overlaps lwe_in"),
        (dict(lwe=big[:c.lwe.size], ws=ws_in_big), "workspace overlaps lwe_in"),
        (dict(lwe=Raw(c.lwe.ctypes.data + 1)), "lwe_in is not"),
        (dict(ws=c.ws, ws_bytes=c.ws.nbytes - 1), "workspace_bytes"), (dict(ws=c.ws, ws_bytes=mg_ws), "workspace_bytes"),
        # batch * H * max(k * levels, k + 1) >= 2^32 with H = M / 2 = 2
        (dict(batch=(1 << 32) // (2 * K * LEVELS) + 1), "2^32"), (dict(batch=1 << 31, k=0, levels=1), "2^32"),
    ]
    for kw, word in shared + pack_only:
        refused(c.pack, kw, word)


@pytest.mark.parametrize("P", [native_binary64.Plan32, native_binary32.Plan52])
def test_binary_kinds_are_refused_by_calls_2_and_3_and_served_by_1(P):
    c = Case(P)
    assert c.merge() == EINVAL and "native_binary kind" in err() and c.untouched()
    assert c.pack() == EINVAL and "native_binary kind" in err() and c.untouched()
    assert c.embed(out=None) == EINVAL and "glwe_out is NULL" in err()           # ... past the kind, at the pointers
    assert c.embed() != EINVAL                                                   # (what follows needs a device: any status but CNTT_EINVAL)


def test_max_terms_bound_counts_k_times_levels():
    """native64 Plan32 at n = 32768 holds 61 terms: k = 1, base_log = 1, levels = 62 fits the word and not the exact range; levels = 61
    passes, and so does k = 0 with any levels, which sums nothing"""
    plan = native64.Plan32.try_new(32768)
    assert plan.max_terms() == 61
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * 5)(*[16] * 5)
    assert L.cntt_native_glwe_merge_batch(plan._h, p(16), p(16), p(16), dummy, 0, 3, 1, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "glwe_dim * levels = 62 exceeds cntt_native_max_terms() = 61" in err()
    assert L.cntt_native_ring_pack_batch(plan._h, p(16), p(16), dummy, 4, 1, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "glwe_dim * levels = 62 exceeds cntt_native_max_terms() = 61" in err()
    assert L.cntt_native_glwe_merge_batch(plan._h, None, p(16), p(16), dummy, 0, 3, 1, 1, 61, 1, None, 0, 0, None) == EINVAL
    assert "glwe_out is NULL" in err()                                          # 61 terms got past the size checks
    assert L.cntt_native_ring_pack_batch(plan._h, None, p(16), None, 4, 0, 1, 62, 1, None, 0, 0, None) == EINVAL
    assert "glwe_out is NULL" in err()


def test_byte_counts_past_2_63_are_refused_before_they_are_formed():
    plan = native32.Plan52.try_new(16)
    assert plan.max_terms() > 1 << 30
    L, p = cntt.lib(), ctypes.c_void_p
    dummy = (ctypes.c_void_p * plan.NPRIMES)(*[16] * plan.NPRIMES)
    assert L.cntt_native_glwe_merge_batch(plan._h, p(16), p(16), p(16), dummy, 0, 3, (1 << 30) - 1, 1, 1, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()
    assert L.cntt_native_ring_pack_batch(plan._h, p(16), p(16), dummy, 4, (1 << 30) - 1, 1, 1, 1, None, 0, 0, None) == EINVAL
    assert "2^63 bytes" in err()
    assert L.cntt_native_glwe_embed_batch(plan._h, p(16), p(16), (1 << 31), 1 << 26, 0, None) == EINVAL
    assert "2^63 bytes" in err()


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32])
def test_empty_calls_do_nothing_and_k_zero_needs_no_key(P):
    c = Case(P)
    L = cntt.lib()
    assert L.cntt_native_glwe_embed_batch(c.plan._h, None, None, K, 0, 0, None) == 0
    assert L.cntt_native_glwe_merge_batch(c.plan._h, None, None, None, None, 0, 3, K, 8, 3, 0, None, 0, 0, None) == 0
    assert L.cntt_native_ring_pack_batch(c.plan._h, None, None, None, M, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.embed(batch=0) == 0 and c.merge(batch=0) == 0 and c.pack(batch=0) == 0 and c.untouched()
    # k = 0 with a NULL key passes the argument checks (what follows needs a device: any status but CNTT_EINVAL)
    body, out = np.arange(B * N * c.cw, dtype=c.dtype), np.zeros(B * N * c.cw, dtype=c.dtype)
    assert c.merge(k=0, key=None, even=body, odd=body.copy(), out=out) != EINVAL
    assert c.pack(k=0, key=None, lwe=np.arange(B * M * c.cw, dtype=c.dtype), out=out) != EINVAL
    for m in (1, 2, N):
        lwe = np.arange(B * m * (K * N + 1) * c.cw, dtype=c.dtype)
        assert c.pack(m=m, lwe=lwe, out=np.zeros_like(c.out)) != EINVAL


@pytest.mark.parametrize("P", [native64.Plan32, native32.Plan32, native128.Plan32])
def test_python_wrappers_panic_on_bad_shapes(P):
    c = Case(P)
    pl, pe = c.plan, c.pe
    one = [p[:KEY] for p in c.key]
    for args in [(c.out[:-pe], c.lwe[:B * (K * N + 1) * c.cw], K), (c.out, c.lwe[:B * (K * N + 1) * c.cw - c.cw], K), (c.out, c.lwe[:B * (K * N + 1) * c.cw], -1)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_embed_batch(*args)
    for args in [(c.out[:-pe], c.even, c.odd, one, 5, 3, K, 4, LEVELS), (c.out, c.even, c.odd[:-pe], one, 5, 3, K, 4, LEVELS),
                 (c.out, c.even, c.odd, c.key, 5, 3, K, 4, LEVELS), (c.out, c.even, c.odd, None, 5, 3, K, 4, LEVELS),
                 (c.out, c.even, c.odd, one, -1, 3, K, 4, LEVELS), (c.out, c.even, c.odd, one, 5, -3, K, 4, LEVELS),
                 (c.out, c.even, c.odd, one, 5, 3, K, 0, LEVELS), (c.out, c.even, c.odd, one[:-1], 5, 3, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.glwe_merge_batch(*args)
    for args in [(c.out[:-pe], c.lwe, c.key, M, K, 4, LEVELS), (c.out, c.lwe[:-c.cw], c.key, M, K, 4, LEVELS), (c.out, c.lwe, one, M, K, 4, LEVELS),
                 (c.out, c.lwe, None, M, K, 4, LEVELS), (c.out, c.lwe, c.key, 0, K, 4, LEVELS), (c.out, c.lwe, c.key, M, K, 0, LEVELS),
                 (c.out, c.lwe, c.key[:-1], M, K, 4, LEVELS)]:
        with pytest.raises((Panic, TypeError)):
            pl.ring_pack_batch(*args)
    with pytest.raises(Panic):                                                 # through the C checks: the workspace is too small
        pl.ring_pack_batch(c.out, c.lwe, c.key, M, K, 4, LEVELS, workspace=c.ws[:255])
    with pytest.raises(Panic):                                                 # ... and an even exponent
        pl.glwe_merge_batch(c.out, c.even, c.odd, one, 5, 4, K, 4, LEVELS)
    for fn, args in ((pl.glwe_merge_workspace_bytes, (K, LEVELS, -1)), (pl.glwe_merge_workspace_bytes, (K, 0, 1)),
                     (pl.ring_pack_workspace_bytes, (0, K, LEVELS, 1)), (pl.ring_pack_workspace_bytes, (M, -1, LEVELS, 1))):
        with pytest.raises(Panic):
            fn(*args)
    assert c.untouched()
