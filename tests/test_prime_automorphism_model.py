"""The model of tests/prime_automorphism_model.py against its specification (include/cntt_prime_automorphism.h), on the CPU: the gather
form is the scatter that defines sigma_t; the group law; the NTT-slot permutation against the CPU oracle's forward transform, which pins
the slot order before any GPU run; the trace on noise-free keys; and the derived rounding bound of the Galois keyswitch.  No GPU."""
import random

import numpy as np
import pytest

from oracle import pyoracle
from prime_automorphism_model import (autom_gather, autom_gather_np, autom_scatter, automorphism_key, model_autoks, model_trace, ntt_permutation,
                                      phase, trace_exponents, trace_keys)
from test_prime_pbs_model import P30, P62, PM64, lift, wbits


def odd(n):
    return range(1, 2 * n, 2)


@pytest.mark.parametrize("n", [16, 32])
def test_gather_form_is_the_scatter_definition(n):
    p = P62
    rng = random.Random("autom/gather/%d" % n)
    f = [rng.randrange(p) for _ in range(n)]
    f[3] = 0                                                           # a zero stays zero under the sign
    for t in odd(n):
        want = autom_scatter(f, t, p)
        assert autom_gather(f, t, p) == want, t
        assert autom_gather_np(np.array(f, dtype=np.uint64), t, p).tolist() == want, t
        assert sorted(min(x, p - x) for x in want) == sorted(min(x, p - x) for x in f)


@pytest.mark.parametrize("n", [16, 32])
def test_group_law_identity_and_inverse(n):
    p = P30
    rng = random.Random("autom/group/%d" % n)
    f = [rng.randrange(p) for _ in range(n)]
    assert autom_gather(f, 1, p) == f
    inv = [f[0]] + [(-x) % p for x in reversed(f[1:])]                 # X -> X^-1 = -X^(n-1): coefficient i moves to n - i, negated
    assert autom_gather(f, 2 * n - 1, p) == inv
    for s in odd(n):
        for t in odd(n):
            assert autom_gather(autom_gather(f, t, p), s, p) == autom_gather(f, s * t % (2 * n), p), (s, t)


def max_logn(p):
    return ((p - 1) & -(p - 1)).bit_length() - 2


def slot_check(p, bits, n, ts, rng):
    dtype = np.uint64 if bits == 64 else np.uint32
    plan = pyoracle.Plan.try_new(n, p, bits)
    assert plan is not None, (p, n)
    f = np.array([rng.randrange(p) for _ in range(n)], dtype=dtype)
    fhat = f.copy()
    plan.fwd(fhat)
    for t in ts:
        g = autom_gather_np(f, t, p).astype(dtype)
        plan.fwd(g)
        assert np.array_equal(g, fhat[ntt_permutation(t, n)]), (p, n, t)


@pytest.mark.parametrize("p,bits", [(P62, 64), (PM64, 64), (P30, 32)])
def test_ntt_slot_formula_against_the_oracle(p, bits):
    """fwd(sigma_t f) == permute(fwd f) for EVERY odd t at n = 16 (64-bit words only: 32-bit plans start at 32) and 32, and for seeded
    random t at n = 1024 and at the largest size the modulus has a root for, capped at 2^16.  The forward transform leaves its words in
    [0, p) for these primes, so the comparison is word for word."""
    rng = random.Random("autom/slots/%d" % p)
    for n in ([16] if bits == 64 else []) + [32]:
        slot_check(p, bits, n, odd(n), rng)
    for n in sorted({1024, 1 << min(16, max_logn(p))}):
        ts = [1, 3, n + 1, n // 2 + 1, 2 * n - 1] + [2 * rng.randrange(n) + 1 for _ in range(6)]
        slot_check(p, bits, n, ts, rng)


def binary_key(rng, k, n):
    return [[rng.randrange(2) for _ in range(n)] for _ in range(k)]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("p,beta,ell", [(PM64, 16, 4), (P30, 10, 3)])
def test_trace_on_noise_free_keys_with_no_rounding(p, beta, ell, k):
    """base_log * levels = W: the rounding term is zero, so for every steps in [0, log2 n] coefficient i of the phase is exactly
    2^steps phase[i] where 2^steps divides i and 0 elsewhere"""
    n, logn = 16, 4
    assert beta * ell == wbits(p)
    rng = random.Random("autom/trace/%d/%d" % (p, k))
    S = binary_key(rng, k, n)
    ct = [rng.randrange(p) for _ in range((k + 1) * n)]
    ph = phase(ct, S, p)
    keys = trace_keys(rng, p, S, logn, n, beta, ell)
    per = k * ell * (k + 1) * n
    for steps in range(logn + 1):
        assert trace_exponents(n, steps) == [n + 1, n // 2 + 1, n // 4 + 1, 3][:steps]
        out = model_trace(ct, keys[:steps * per], p, steps, k, n, beta, ell)
        want = [(ph[i] << steps) % p if i % (1 << steps) == 0 else 0 for i in range(n)]
        assert phase(out, S, p) == want, (steps, k)
    assert model_trace(ct, [], p, 0, k, n, beta, ell) == ct


@pytest.mark.parametrize("p,beta,ell", [(PM64, 7, 3), (P62, 11, 2), (P30, 4, 3), (P30, 22, 1)])
def test_rounding_bound_of_the_galois_keyswitch(p, beta, ell):
    """s = W - base_log * levels > 0, binary key, noise-free AK: phase(out) - sigma_t(phase(in)) = sum_r (x_r - r_r 2^s) (*) sigma_t(S_r)
    with |x - r 2^s| <= 2^(s-1) per coefficient and n binary coefficients per product, so every coefficient lies within k n 2^(s-1) --
    derived, not measured.  With add_input the phase of the input is added on top."""
    n = 16
    s = wbits(p) - beta * ell
    assert s > 0
    rng = random.Random("autom/bound/%d/%d" % (p, beta))
    for k in (1, 2):
        S = binary_key(rng, k, n)
        for t in (3, n + 1, 2 * n - 1, 2 * rng.randrange(n) + 1):
            ct = [rng.randrange(p) for _ in range((k + 1) * n)]
            key = automorphism_key(rng, p, S, t, n, beta, ell)
            ph = phase(ct, S, p)
            rot = autom_gather(ph, t, p)
            for add in (False, True):
                out = model_autoks(ct, key, p, t, k, n, beta, ell, add)
                assert all(0 <= v < p for v in out)
                want = [(x + y) % p for x, y in zip(rot, ph)] if add else rot
                err = [abs(lift((x - y) % p, p)) for x, y in zip(phase(out, S, p), want)]
                assert max(err) <= k * n * (1 << (s - 1)), (p, k, t, add, max(err))
    # k = 0: the body alone
    ct = [rng.randrange(p) for _ in range(n)]
    assert model_autoks(ct, [], p, 5, 0, n, beta, ell, False) == autom_gather(ct, 5, p)
