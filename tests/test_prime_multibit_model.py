"""tests/prime_multibit_model.py against its specification, on the CPU: the closed form of the transformed monomial against the oracle's
forward transform; the pointwise bundle step against the ring form; with noiseless keys the group step multiplies by
X^(sum a_i s_i) up to the decomposition's rounding; the layout of bsk_mb; and grouping = 1 against the classic CMux iteration.
No GPU needed."""
import random

import numpy as np
import pytest

from oracle import pyoracle
from prime_multibit_model import (P31, P51, PG64, flatten_keys, mb_offset, model_accumulate, model_group_step, model_multibit_rotate,
                                  monomial_ntt, negacyclic_fast, subset_exponents, trivial_ggsw)
from test_prime_pbs_model import P30, P32, P50, P62, P63, PM64, model_terms_element, negacyclic, source, wbits

# one prime of each arithmetic class on each word type: lazy, strict, Montgomery, 2^64 - c, the two classes on doubles / lazy, strict,
# above 2^31
CLASSES = [(P62, 64), (P63, 64), (PG64, 64), (PM64, 64), (P50, 64), (P51, 64), (P30, 32), (P31, 32), (P32, 32)]


def oracle_fwd(plan, coeffs):
    buf = np.array(coeffs, dtype=plan.dtype)
    plan.fwd(buf)
    return [int(x) for x in buf]


def psi_of(plan):
    return oracle_fwd(plan, [0, 1] + [0] * (plan.n - 2))[0]


@pytest.mark.parametrize("p,bits", CLASSES)
def test_monomial_closed_form_equals_the_forward_transform(p, bits):
    """fwd(X^e)[c] = psi^(e (2 bitrev(c) + 1)) with psi = fwd(X)[0] = the forward twiddle at bitrev(1), psi^n = -1; X^e for e >= n is
    -X^(e - n).  n = 16 is below the 32-bit plans' smallest size: they run at 32 and 64."""
    for n in ((16, 64) if bits == 64 else (32, 64)):
        plan = pyoracle.Plan.try_new(n, p, bits)
        psi = psi_of(plan)
        assert psi == int(plan.table("twid")[n // 2]) and pow(psi, n, p) == p - 1
        for e in (0, 1, n - 1, n, 2 * n - 1):
            x = [0] * n
            x[e % n] = 1 if e < n else p - 1
            assert monomial_ntt(e, psi, n, p) == oracle_fwd(plan, x), (p, n, e)


def test_subset_exponents_bit_order_and_wrap():
    assert subset_exponents([5], 16) == [0, 5]
    assert subset_exponents([1, 2, 4], 16) == [0, 1, 2, 3, 4, 5, 6, 7]
    assert subset_exponents([31, 31, 30, 1], 16) == [0, 31, 31, 30, 30, 29, 29, 28, 1, 0, 0, 31, 31, 30, 30, 29]


@pytest.mark.parametrize("p,bits", [(PM64, 64), (P30, 32)])
def test_pointwise_step_equals_the_ring_step(p, bits):
    """inv(model_accumulate(fwd(digits), n^-1 fwd(keys))) = model_group_step(keys): the NTT-domain formula is the ring formula"""
    n, k, beta, ell, g = 32, 1, 6, 2, 2
    plan = pyoracle.Plan.try_new(n, p, bits)
    psi, ninv = psi_of(plan), pow(n, p - 2, p)
    rng = random.Random("mbmodel/pointwise/%d" % p)
    J = (k + 1) * ell
    elem = [[rng.randrange(p) for _ in range(n)] for _ in range(k + 1)]
    keys = [[[[rng.randrange(p) for _ in range(n)] for _ in range(k + 1)] for _ in range(J)] for _ in range(1 << g)]
    a = [2 * n - 1, n + 3]
    terms = [x for d in model_terms_element(elem, 0, p, beta, ell, mode="plain") for x in oracle_fwd(plan, d)]
    key_ntt = [v * ninv % p for pat in keys for row in pat for poly in row for v in oracle_fwd(plan, poly)]
    out = model_accumulate(terms, key_ntt, a, psi, n, p, J, k + 1, g, 1)
    got = []
    for o in range(k + 1):
        buf = np.array(out[o * n:(o + 1) * n], dtype=plan.dtype)
        plan.inv(buf)
        got.append([int(x) for x in buf])
    assert got == model_group_step(elem, a, keys, p, beta, ell)


def test_fast_negacyclic_is_the_models():
    rng = random.Random("mbmodel/nega")
    for p in (PM64, P30, 97):
        a, b = [rng.randrange(p) for _ in range(16)], [rng.randrange(p) for _ in range(16)]
        assert negacyclic_fast(a, b, p) == negacyclic(a, b, p)


def centred(x, p):
    return x if x <= p // 2 else x - p


@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("p", [P62, P30])
def test_noiseless_keys_multiply_by_the_selected_monomial(p, g):
    """2^g groups whose secret bits run through every pattern; key (r, t) = the zero-mask GGSW of [t == the pattern of group r].  Each
    step is then X^(e_s) times the recomposed digits of the accumulator, which differ from it by at most 2^(s-1) per coefficient
    (s = W - base_log levels): after G steps |acc - X^(sum a_i s_i) lut| <= G 2^(s-1)."""
    n, k, beta, ell = 16, 1, 5, 3
    G, L = 1 << g, g << g
    W = wbits(p)
    rng = random.Random("mbmodel/noiseless/%d/%d" % (p, g))
    secret = [(r >> i) & 1 for r in range(G) for i in range(g)]
    keys = [[trivial_ggsw(1 if t == r else 0, p, n, k, beta, ell) for t in range(1 << g)] for r in range(G)]
    rot_t = [rng.randrange(2 * n) for _ in range(L)] + [rng.randrange(2 * n)]
    rot_t[0], rot_t[1 % L] = 2 * n - 1, n                                       # with g >= 2 a subset sum that wraps 2n
    lut = [rng.randrange(p) for _ in range((k + 1) * n)]
    out = model_multibit_rotate(lut, rot_t, flatten_keys(keys), p, n, L, k, beta, ell, g, 1)
    total = (rot_t[L] + sum(a * s for a, s in zip(rot_t, secret))) % (2 * n)
    bound = G * (1 << (W - beta * ell - 1))
    for q in range(k + 1):
        want = source(lut[q * n:(q + 1) * n], total, p, "rotate")
        assert all(abs(centred((x - y) % p, p)) <= bound for x, y in zip(out[q * n:(q + 1) * n], want)), (p, g, q)


def test_bsk_mb_layout():
    """bsk_mb is the C-order array [G][2^g][J][k + 1][n]: mb_offset, flatten_keys and the rotation model agree on it"""
    g, J, k, G, n = 3, 4, 1, 2, 4
    arr = np.arange(G * (1 << g) * J * (k + 1) * n).reshape(G, 1 << g, J, k + 1, n)
    for r, t, j, o in ((0, 0, 0, 0), (1, 5, 3, 1), (0, 7, 2, 0), (1, 0, 0, 1)):
        assert arr[r, t, j, o, 0] == mb_offset(r, t, j, o, g, J, k) * n
    assert mb_offset(1, 0, 0, 0, g, J, k) == (1 << g) * J * (k + 1)            # a group's size
    assert mb_offset(0, 1, 0, 0, g, J, k) == J * (k + 1)                        # a bsk_ntt slice
    assert flatten_keys(arr.tolist()) == list(range(arr.size))


@pytest.mark.parametrize("p", [PM64, P32])
@pytest.mark.parametrize("bit", [0, 1])
def test_grouping_one_equals_the_classic_iteration(p, bit):
    """g = 1 with K_1 = K and K_0 = Gd - K (Gd the zero-mask GGSW of 1, K that of the secret bit) against the classic step
    acc + ExtProd(K, X^a acc - acc).  With rec(x) the recomposed digits of x, |rec(x) - x| <= h = 2^(s-1) per coefficient:
    multi-bit gives rec(acc) + bit (X^a - 1) rec(acc), the classic step acc + bit rec(X^a acc - acc), so they differ by at most
    h + bit * 3 h."""
    n, k, beta, ell = 16, 1, 4, 3
    h = 1 << (wbits(p) - beta * ell - 1)
    rng = random.Random("mbmodel/classic/%d/%d" % (p, bit))
    K, Gd = trivial_ggsw(bit, p, n, k, beta, ell), trivial_ggsw(1, p, n, k, beta, ell)
    K0 = [[[(x - y) % p for x, y in zip(gp, kp)] for gp, kp in zip(grow, krow)] for grow, krow in zip(Gd, K)]
    for a in (0, 1, n, 2 * n - 1, rng.randrange(2 * n)):
        acc = [[rng.randrange(p) for _ in range(n)] for _ in range(k + 1)]
        multi = model_group_step(acc, [a], [K0, K], p, beta, ell)
        terms = model_terms_element(acc, a, p, beta, ell, mode="cmux")
        for o in range(k + 1):
            classic = list(acc[o])
            for j, d in enumerate(terms):
                classic = [(x + y) % p for x, y in zip(classic, negacyclic(d, K[j][o], p))]
            assert all(abs(centred((x - y) % p, p)) <= h + 3 * h * bit for x, y in zip(multi[o], classic)), (p, bit, a, o)
