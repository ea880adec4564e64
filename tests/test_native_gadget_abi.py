"""C ABI of the rotation / gadget decomposition and of the external product on undecomposed polynomials (include/cntt_ext.h through
include/cntt_gadget.h): the symbols and the enum are declared by cntt_ext.h and exported, cntt.h keeps its surface, every
CNTT_EINVAL case is refused by the argument checks that precede any device call with the output untouched, the "native_gadget"
switch exists -- and the big-integer model of the digits that the GPU tests compare against is itself checked here: closed form ==
sequential rule, digit range, recomposition and rounding distance.  No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cntt_ext.h")
HEADER = os.path.join(ROOT, "include", "cntt.h")
NEW = {"cntt_native_gadget_decompose_batch", "cntt_native_external_product_decomposed_batch"}


# -- the model (restated in tests/test_gpu_native_gadget.py, which cannot import this file's namesake from the library) -----------
def rounded(x, w, beta, ell):
    s = w - beta * ell
    return x if s == 0 else ((x + (1 << (s - 1))) % (1 << w)) >> s


def digits_sequential(x, w, beta, ell):
    """d_1 .. d_ell by the rule of cntt_gadget.h, from the low level up."""
    state, B, out = rounded(x, w, beta, ell), 1 << beta, []
    for _ in range(ell):
        d = state % B
        state >>= beta
        if d >= B // 2:
            d -= B
            state += 1
        out.append(d)
    return out[::-1]


def digits_closed(x, w, beta, ell):
    B = 1 << beta
    K = sum((B // 2) * B ** (ell - l) for l in range(1, ell + 1))
    t = (rounded(x, w, beta, ell) + K) % B ** ell
    return [((t >> (beta * (ell - l))) & (B - 1)) - B // 2 for l in range(1, ell + 1)]


def edge_words(w, beta, ell):
    s = w - beta * ell
    words = {0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1, 0x9E3779B97F4A7C15F39CC0605CEDC834 % (1 << w)}
    if s:
        for k in (0, 1, (1 << (beta * ell)) - 1, (1 << (beta * ell - 1)) - 1, 1 << (beta * ell - 1)):
            words.add((k << s) + (1 << (s - 1)))       # the rounding ties
            words.add(((k << s) + (1 << (s - 1)) - 1) % (1 << w))
    return sorted(words)


def shapes(w):
    return [(b, l) for b in range(1, w + 1) for l in range(1, w // b + 1)]


@pytest.mark.parametrize("w,step", [(32, 1), (64, 5), (128, 37)])
def test_digit_model(w, step):
    for beta, ell in shapes(w)[::step] + [(w, 1), (1, w), (1, 1)]:
        B, s = 1 << beta, w - beta * ell
        for x in edge_words(w, beta, ell):
            d = digits_sequential(x, w, beta, ell)
            assert d == digits_closed(x, w, beta, ell), (w, beta, ell, x)
            assert all(-B // 2 <= v < B // 2 for v in d)
            r = rounded(x, w, beta, ell)
            assert sum(v << (w - beta * l) for l, v in enumerate(d, 1)) % (1 << w) == (r << s) % (1 << w)
            dist = (x - (r << s)) % (1 << w)
            dist = min(dist, (1 << w) - dist)
            assert dist <= (1 << (s - 1) if s else 0), (w, beta, ell, x)


# -- the surface ---------------------------------------------------------------------------------------------------------------
def preprocessed(path):
    return subprocess.run(["gcc", "-std=c11", "-E", "-P", "-x", "c", path], check=True, capture_output=True, text=True).stdout


def test_symbols_and_enum_are_declared_by_cntt_ext_h_and_exported():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", EXT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    text = preprocessed(EXT)
    names = set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", text))
    assert NEW <= names
    assert re.search(r"CNTT_SRC_PLAIN = 0, CNTT_SRC_ROTATE = 1, CNTT_SRC_CMUX = 2 \} cntt_src_mode_t;", text)
    base = preprocessed(HEADER)
    assert not (NEW & set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", base))) and "cntt_src_mode" not in base
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_native_gadget_switch_exists_and_is_documented():
    # default 0: the fused kernel measured slower than decomposition + external product on every shape (profiles/r07_native_gadget_ab.txt)
    cntt.debug_set("reset", 0)
    assert cntt.debug_get("native_gadget") == 0
    cntt.debug_set("native_gadget", 1)
    assert cntt.debug_get("native_gadget") == 1
    cntt.debug_set("native_gadget", -1)
    assert cntt.debug_get("native_gadget") == 0
    hdr = open(HEADER).read()
    table = hdr[hdr.index("TESTING ONLY"):hdr.index("int cntt_debug_set")]
    assert '"native_gadget"' in table


# -- CNTT_EINVAL: host buffers, refused before any device call -------------------------------------------------------------------
from concrete_ntt_amd._lib import EINVAL  # noqa: E402


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def decompose(plan, terms, polys, rot, npolys, beta, ell, mode, batch):
    return cntt.lib().cntt_native_gadget_decompose_batch(plan._h, ptr(terms), ptr(polys), None if rot is None else ptr(rot), npolys,
                                                         beta, ell, mode, batch, 0, None)


def fused(plan, out, polys, rot, addend, keys, npolys, beta, ell, mode, nout, batch):
    kp = (ctypes.c_void_p * plan.NPRIMES)(*[k.ctypes.data for k in keys])
    return cntt.lib().cntt_native_external_product_decomposed_batch(
        plan._h, ptr(out), ptr(polys), None if rot is None else ptr(rot), None if addend is None else ptr(addend), kp, npolys, beta, ell,
        mode, nout, batch, 0, None)


def error_code():
    return EINVAL


BAD = [  # (base_log, levels, mode, with rot, word in the message)
    (0, 2, 0, True, "base_log"), (8, 0, 0, True, "levels"), (33, 2, 0, True, "base_log * levels"), (8, 2, 3, True, "src_mode"),
    (8, 2, -1, True, "src_mode"), (8, 2, 1, False, "rot"), (8, 2, 2, False, "rot")]


@pytest.mark.parametrize("beta,ell,mode,with_rot,word", BAD)
def test_decompose_refuses_bad_arguments(beta, ell, mode, with_rot, word):
    plan = native64.Plan32.try_new(32)
    polys = np.arange(64, dtype=np.uint64)
    terms = np.full(64 * max(ell, 1), 7, dtype=np.uint64)
    rot = np.zeros(2, dtype=np.uint32) if with_rot else None
    assert decompose(plan, terms, polys, rot, 1, beta, ell, mode, 2) == error_code()
    assert word in cntt.lib().cntt_last_error().decode()
    assert (terms == 7).all()


@pytest.mark.parametrize("beta,ell,mode,with_rot,word", BAD)
def test_fused_refuses_bad_arguments(beta, ell, mode, with_rot, word):
    plan = native64.Plan32.try_new(32)
    polys = np.arange(64, dtype=np.uint64)
    out = np.full(64, 7, dtype=np.uint64)
    keys = [np.zeros(32 * max(ell, 1), dtype=np.uint32) for _ in range(plan.NPRIMES)]
    rot = np.zeros(2, dtype=np.uint32) if with_rot else None
    assert fused(plan, out, polys, rot, None, keys, 1, beta, ell, mode, 1, 2) == error_code()
    assert word in cntt.lib().cntt_last_error().decode()
    assert (out == 7).all()


@pytest.mark.parametrize("cls,wbits", [(native32.Plan32, 32), (native64.Plan32, 64), (native128.Plan32, 128)])
def test_base_log_times_levels_is_bounded_by_the_word_of_the_kind(cls, wbits):
    plan = cls.try_new(32)
    dt = plan.word_dtype
    per = 32 * (2 if wbits == 128 else 1)
    polys = np.zeros(per, dtype=dt)
    terms = np.full(per * (wbits + 1), 7, dtype=dt)
    assert decompose(plan, terms, polys, None, 1, 1, wbits + 1, 0, 1) == error_code()
    assert decompose(plan, terms, polys, None, 1, wbits // 2 + 1, 2, 0, 1) == error_code()
    assert (terms == 7).all()


def test_overlaps_and_rot_range_and_max_terms_are_refused():
    plan = native64.Plan32.try_new(32)
    n, code = 32, error_code()
    buf = np.full(6 * n, 7, dtype=np.uint64)
    rot = np.zeros(1, dtype=np.uint32)
    # terms (2 polynomials at word 16) overlaps polys (word 0 .. 31)
    assert decompose(plan, buf[16:], buf[:n], rot, 1, 8, 2, 1, 1) == code
    assert "terms overlaps polys" in cntt.lib().cntt_last_error().decode()
    keys = [np.zeros(2 * n, dtype=np.uint32) for _ in range(plan.NPRIMES)]
    assert fused(plan, buf[16:], buf[:n], rot, None, keys, 1, 8, 2, 1, 1, 1) == code
    assert "out overlaps polys" in cntt.lib().cntt_last_error().decode()
    # an addend that overlaps out without being out
    assert fused(plan, buf[2 * n:3 * n], buf[:n], rot, buf[2 * n + 8:], keys, 1, 8, 2, 1, 1, 1) == code
    assert "addend" in cntt.lib().cntt_last_error().decode()
    # host path: an exponent that is not below 2n
    rot[0] = 2 * n
    assert decompose(plan, buf[n:3 * n], buf[:n], rot, 1, 8, 2, 1, 1) == code
    assert "rot[0]" in cntt.lib().cntt_last_error().decode()
    assert fused(plan, buf[n:2 * n], buf[:n], rot, None, keys, 1, 8, 2, 2, 1, 1) == code
    assert "rot[0]" in cntt.lib().cntt_last_error().decode()
    rot[0] = 0
    # npolys * levels past cntt_native_max_terms()
    t = plan.max_terms() + 1
    assert fused(plan, buf[n:2 * n], buf[:n], rot, None, keys, t, 1, 1, 0, 1, 1) == code
    assert "cntt_native_max_terms" in cntt.lib().cntt_last_error().decode()
    assert (buf == 7).all()


def test_python_wrappers_panic_on_bad_shapes():
    plan = native64.Plan32.try_new(32)
    polys = np.zeros(64, dtype=np.uint64)
    with pytest.raises(cntt.Panic):
        plan.gadget_decompose_batch(np.zeros(64, dtype=np.uint64), polys, 8, 2)            # terms too short
    with pytest.raises(cntt.Panic):
        plan.gadget_decompose_batch(np.zeros(128, dtype=np.uint64), polys, 8, 2, mode="cmux")   # no rot
    with pytest.raises(cntt.Panic):
        plan.external_product_decomposed_batch(np.zeros(64, dtype=np.uint64), polys, [np.zeros(64, dtype=np.uint32)] * 4, 8, 2, 1)
    out = np.full(64, 7, dtype=np.uint64)
    with pytest.raises(cntt.Panic):   # through the C checks: base_log * levels > 64
        plan.external_product_decomposed_batch(out, polys, [np.zeros(32 * 3, dtype=np.uint32) for _ in range(5)], 33, 3, 1)
    assert (out == 7).all()
