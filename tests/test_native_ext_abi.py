"""C ABI of the native external product (include/cntt_ext.h): the header compiles as plain C11, the library exports what it declares,
cntt.h keeps its 87 entry points, cntt_native_max_terms() equals an independent big-integer recomputation of the exactness bound from
the kinds' primes, and the "native_ext" testing switch exists.  No GPU needed."""
import os
import re
import subprocess

import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import (native32, native64, native128, native_binary32, native_binary64, native_binary128)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cntt_ext.h")
HEADER = os.path.join(ROOT, "include", "cntt.h")

P32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801, 1068433409, 1068564481, 1069219841, 1071513601, 1073479681]
P52 = [1125899881086977, 1125899885412353, 1125899886395393, 1125899899174913, 1125899902124033, 1125899903107073]
# name -> (plan class, primes, word bits, binary, primes of the top mixed-radix digit)
KINDS = {
    "native32_plan32": (native32.Plan32, P32[:3], 32, False, 1),
    "native64_plan32": (native64.Plan32, P32[:5], 64, False, 2),
    "native128_plan32": (native128.Plan32, P32[:10], 128, False, 2),
    "native_binary32_plan32": (native_binary32.Plan32, P32[:2], 32, True, 1),
    "native_binary64_plan32": (native_binary64.Plan32, P32[:3], 64, True, 1),
    "native_binary128_plan32": (native_binary128.Plan32, P32[:5], 128, True, 2),
    "native32_plan52": (native32.Plan52, P52[:2], 32, False, 1),
    "native64_plan52": (native64.Plan52, P52[:3], 64, False, 1),
    "native_binary32_plan52": (native_binary32.Plan52, P52[:1], 32, True, 1),
    "native_binary64_plan52": (native_binary64.Plan52, P52[:2], 64, True, 1),
}


def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def expected_max_terms(primes, word_bits, binary, top, n, plan32):
    """Largest T with T n A^2 (binary: T n A), A = 2^w - 1, inside the exact range of the reconstruction: the reference's sign rule
    on the top digit, and for the Plan32 kinds the accumulating CRT's 27-bit rounded fraction sum (k primes, < 1.5 units each)."""
    m = 1
    for p in primes:
        m *= p
    mt = 1
    for p in primes[len(primes) - top:]:
        mt *= p
    pre = m // mt
    lim = min((m - pre) // 2, (m + pre) // 2 - 1)
    if plan32:
        lim = min(lim, (m - 1) // 2, (m * (2 ** 27 - 3 * len(primes))) >> 28)
    a = 2 ** word_bits - 1
    d = n * a * (1 if binary else a)
    return max(1, lim // d)


def test_ext_header_is_plain_c11():
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", EXT],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(EXT).read()
    assert '#include "cntt.h"' in src
    assert "no counterpart in the reference" in src.split("*/")[0]


def test_library_exports_every_ext_symbol():
    names = declarations(EXT)
    assert set(names) == {"cntt_native_external_product_batch", "cntt_native_max_terms"}
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    cntt.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))
    assert set(names) <= exported


def test_cntt_h_keeps_87_entry_points():
    names = declarations(HEADER)
    assert len(names) == 87, len(names)
    assert "cntt_native_external_product_batch" not in names and "cntt_native_max_terms" not in names


@pytest.mark.parametrize("n", [32, 1024, 16384, 65536])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_max_terms_is_the_big_integer_bound(kind, n):
    cls, primes, bits, binary, top = KINDS[kind]
    plan = cls.try_new(n)
    if any((p - 1) % (2 * n) for p in primes):   # no 2n-th root of unity modulo one of the primes: try_new is None
        assert plan is None
        return
    want = expected_max_terms(primes, bits, binary, top, n, kind.endswith("plan32"))
    assert plan.max_terms() == want
    assert want >= 1


def test_max_terms_reference_points():
    # native64 Plan32 (the figures cntt_ext.h quotes): 2^149.95 / 2 / 2^138 at n = 1024, less the accumulating CRT's margin
    assert native64.Plan32.try_new(1024).max_terms() == 1964
    assert native64.Plan32.try_new(32768).max_terms() == 61


def test_too_many_terms_is_einval_before_any_device_work():
    import numpy as np
    plan = native64.Plan32.try_new(32)
    t = plan.max_terms() + 1
    out = np.full(32, 7, dtype=np.uint64)
    with pytest.raises(cntt.Panic):
        plan.external_product_batch(out, np.zeros(32 * t, dtype=np.uint64),
                                    [np.zeros(32 * t, dtype=np.uint32) for _ in range(5)], t, 1)
    assert (out == 7).all()


def test_native_ext_switch_exists_and_is_documented():
    cntt.debug_set("reset", 0)
    assert cntt.debug_get("native_ext") == 1
    cntt.debug_set("native_ext", 0)
    assert cntt.debug_get("native_ext") == 0
    cntt.debug_set("native_ext", -1)
    assert cntt.debug_get("native_ext") == 1
    hdr = open(HEADER).read()
    table = hdr[hdr.index("TESTING ONLY"):hdr.index("int cntt_debug_set")]
    assert '"native_ext"' in table
