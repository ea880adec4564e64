"""The join of the fused prime64 product at n = 1024 (csrc/ntt_kernel.hpp MulWp::run, JOIN): forward transform -> Montgomery product
against rhs_ntt (mul_fused_join) -> inverse transform whose last stage multiplies an UNREDUCED sum by 1/N (Bfly::inv_norm_join).  Both
rest on range arguments (csrc/ntt_arith.hpp; replayed in exact integers by test_fused_join_bounds_model.py); this file
drives the device code to the top of those ranges and compares word for word.

Primes (all of the 64-bit lazy class, 2^51 <= p < 2^62, asserted on the plan): the headline 4611686018427322369 = 2^62 - 65535 (4p is
just under 2^64: no slack), the smallest lazy prime the test helpers name (1152921504607338497, just above 2^60: the reference's Barrett
estimate reaches 2p there), the largest prime = 1 mod 2n below 2^62 and the first one the helpers' search finds above the class floor 2^51.
Batches 1, 5, 13: a single wavefront, the ragged tail of one 12-polynomial tile, and the split walk (one tile + one leftover wavefront).
Inputs, each for lhs (coefficients) against each for rhs_ntt (NTT-domain words, canonical): all p - 1, all zero, alternating 0 / p - 1,
a delta at index 0, a delta at index n - 1, seeded uniform words.
Per case: mul_ntt_batch == oracle fwd; mul_assign_normalize; inv == the three-launch device form, and rhs_ntt is unchanged."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
from random_cases import _search
from test_gpu_multitrip_transforms import LAZY, P62, make_plans
from test_gpu_parity import LAZY_ABOVE_POW2

pytestmark = pytest.mark.gpu

N = 1024
BATCHES = (1, 5, 13)
PATTERNS = ("pm1", "zero", "alt", "delta0", "deltaN", "uniform")


def _primes():
    smallest_named = min(p for bits, p in LAZY_ABOVE_POW2 if bits == 64)
    largest = _search(N, (1 << 62) - 1)
    floor = _search(N, (1 << 51) + (1 << 36))
    assert smallest_named == 1152921504607338497 and (1 << 51) < floor < largest < (1 << 62)
    return [("headline", P62), ("smallest-named", smallest_named), ("largest", largest), ("class-floor", floor)]


def _pattern(oracle, name, p, batch, seed):
    """batch polynomials of one input pattern, uint64"""
    out = np.zeros((batch, N), dtype=np.uint64)
    if name == "pm1":
        out[:] = p - 1
    elif name == "alt":
        out[:, 1::2] = p - 1
    elif name == "delta0":
        out[:, 0] = p - 1
    elif name == "deltaN":
        out[:, N - 1] = p - 1
    elif name == "uniform":
        out[:] = oracle.fill_uniform(batch * N, p, seed, 64).reshape(batch, N)
    else:
        assert name == "zero"
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    """per prime: plans, the patterns at the largest batch and the oracle's answer for every (lhs, rhs) pair -- computed once"""
    out = {}
    bmax = max(BATCHES)
    for name, p in _primes():
        plan, oplan = make_plans(oracle, 64, N, p, LAZY)
        lhs = {k: _pattern(oracle, k, p, bmax, 0x1700 + i) for i, k in enumerate(PATTERNS)}
        rhs = {k: _pattern(oracle, k, p, bmax, 0x1780 + i) for i, k in enumerate(PATTERNS)}
        lhs_ntt = {}
        for k, v in lhs.items():
            t = v.copy()
            for row in t:
                oplan.fwd(row)
            lhs_ntt[k] = t
        want = {}
        for ka in PATTERNS:
            for kb in PATTERNS:
                t = lhs_ntt[ka].copy()
                for i in range(bmax):
                    bn = rhs[kb][i].copy()
                    oplan.mul_assign_normalize(t[i], bn)
                    oplan.inv(t[i])
                want[ka, kb] = t
        out[name] = (p, plan, lhs, rhs, want)
    return out


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).to("cuda:0")


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("prime", ["headline", "smallest-named", "largest", "class-floor"])
def test_fused_join_at_the_top_of_its_ranges(cases, prime, batch):
    import torch
    p, plan, lhs, rhs, want = cases[prime]
    for kb in PATTERNS:
        b = _dev(rhs[kb][:batch])
        b0 = b.clone()
        for ka in PATTERNS:
            a = _dev(lhs[ka][:batch])
            fused = a.clone()
            plan.mul_ntt_batch(fused, b)
            three = a.clone()
            plan.fwd_batch(three)
            plan.mul_assign_normalize_batch(three, b)
            plan.inv_batch(three)
            torch.cuda.synchronize()
            got = fused.cpu().numpy().view(np.uint64).reshape(batch, N)
            assert int(got.max()) < p, ("not canonical", prime, batch, ka, kb)
            assert np.array_equal(got, want[ka, kb][:batch]), ("mul_ntt_batch vs oracle", prime, batch, ka, kb)
            assert torch.equal(fused, three), ("fused vs three launches", prime, batch, ka, kb)
        assert torch.equal(b, b0), ("rhs_ntt changed", prime, batch, kb)
