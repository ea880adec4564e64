"""tests/native_multibit_model.py against its specification, on the CPU: the per-prime accumulate model composed with the oracle's
residue split, transforms and CRT equals the schoolbook ring expression of include/cntt_multibit.h for each of the six Plan32 kinds and
g = 1 ... 4; the kernel's lazy arithmetic equals the model on all ten primes with every operand P - 1; the vectorised per-plane form
equals the plain-int one.  No GPU needed."""
import random

import numpy as np
import pytest

from native_multibit_model import (KINDS, PRIMES32, R, fast_accumulate_plane, lazy_inner_sum, lazy_word, model_accumulate_native,
                                   model_multibit_rotate, negacyclic_int, plain_terms, redc, ring_group_step, rotate)
from oracle import pyoracle
from prime_multibit_model import model_accumulate, monomial_ntt


def psi_of(n, p):
    plan = pyoracle.Plan.try_new(n, p, 32)
    buf = np.array([0, 1] + [0] * (n - 2), dtype=plan.dtype)
    plan.fwd(buf)
    return int(buf[0])


def to_words(nat, ints):
    if nat.word == 16:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=pyoracle.word_dtype(nat.word))


def from_words(nat, a):
    if nat.word == 16:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[0::2], a[1::2])]
    return [int(x) for x in a]


def oracle_fwd(nat, poly, binary=False):
    res = nat.residues()
    (nat.fwd_binary if binary else nat.fwd)(to_words(nat, poly), res)
    return [[int(x) for x in r] for r in res]


@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_group_step_model_equals_the_schoolbook_ring_expression(kind, g):
    """digits -> the oracle's fwd (split + transforms) -> the per-prime accumulate model with n^-1 -> the oracle's inv (unnormalised
    transforms + CRT) = sum_t X^(e_t) sum_j d_j (*) K_t[j][o] mod 2^w.  Worst-case magnitudes in the first polynomials: all-ones words
    against all-ones keys (1 for the binary kinds)."""
    nprimes, w, binary = KINDS[kind]
    n, k, beta, ell = 32, 1, w // 4, 2
    J, M = (k + 1) * ell, 1 << w
    nat = pyoracle.Native.try_new(kind, n)
    psis = [psi_of(n, PRIMES32[i]) for i in range(nprimes)]
    rng = random.Random("nmb/group/%s/%d" % (kind, g))
    elem = [[M - 1] * n] + [[rng.randrange(M) for _ in range(n)] for _ in range(k)]
    top = 1 if binary else M - 1
    keys = [[[[top] * n if (t, j, o) == (0, 0, 0) else [rng.randrange(top + 1) for _ in range(n)] for o in range(k + 1)] for j in range(J)]
            for t in range(1 << g)]
    a = [2 * n - 1, n, 0, rng.randrange(2 * n)][:g]
    terms = plain_terms(elem, w, beta, ell)
    tplanes = [[] for _ in range(nprimes)]
    for d in terms:
        for i, r in enumerate(oracle_fwd(nat, d)):
            tplanes[i] += r
    kplanes = [[] for _ in range(nprimes)]
    for pat in keys:
        for row in pat:
            for poly in row:
                for i, r in enumerate(oracle_fwd(nat, poly, binary)):
                    kplanes[i] += r
    out = model_accumulate_native(tplanes, kplanes, a, psis, n, J, k + 1, g, 1)
    want = ring_group_step(terms, a, keys, w)
    for o in range(k + 1):
        res = [np.array(out[i][o * n:(o + 1) * n], dtype=np.uint32) for i in range(nprimes)]
        value = nat.words()
        nat.inv(value, res)
        assert from_words(nat, value) == want[o], (kind, g, o)


def test_group_step_is_exact_at_max_terms_with_worst_case_words():
    """native64 at n = 1024: cntt_native_max_terms = 1964 = 2^2 * 491, so g = 2 with J = 491 sits exactly on the bound the calls
    enforce.  Worst-case words: every term and every key polynomial is all-ones words (2^64 - 1) and every exponent is 0, so no monomial
    flips a sign and coefficient n - 1 of the sum is 1964 * n * (2^64 - 1)^2, the largest value the bound admits.  All J terms and all
    2^g * J keys being one polynomial each, the schoolbook expression is 1964 times ONE negacyclic product -- cheap enough here."""
    import concrete_ntt_amd  # noqa: F401  (the library's own figure of the bound, no GPU needed)
    from concrete_ntt_amd import native64
    kind, n, g, J, w = "native64_plan32", 1024, 2, 491, 64
    assert native64.Plan32.try_new(n).max_terms() == (1 << g) * J == 1964
    nprimes, M = KINDS[kind][0], 1 << w
    nat = pyoracle.Native.try_new(kind, n)
    ones = [M - 1] * n
    planes = oracle_fwd(nat, ones)                                  # terms and keys: the same residues
    out = []
    for i in range(nprimes):
        p = PRIMES32[i]
        one = np.array(planes[i], dtype=np.uint32)
        out.append(fast_accumulate_plane(np.tile(one, J), np.tile(one, J << g), [0, 0], psi_of(n, p), n, p, J, 1, g, 1))
    value = nat.words()
    nat.inv(value, out)
    prod = negacyclic_int(ones, ones)
    assert int(prod[n - 1]) == n * (M - 1) ** 2                     # the worst coefficient: no cancellation
    assert from_words(nat, value) == [int(x) * 1964 % M for x in prod]


def test_accumulate_model_is_the_prime_model_times_n_inverse():
    n, p, g, nterms, nout, batch = 32, PRIMES32[0], 2, 3, 2, 2
    rng = random.Random("nmb/ninv")
    psi = psi_of(n, p)
    terms = [rng.randrange(p) for _ in range(batch * nterms * n)]
    key = [rng.randrange(p) for _ in range((nterms * nout << g) * n)]
    rows = [5, 2 * n - 1, n, 63]
    got = model_accumulate_native([terms], [key], rows, [psi], n, nterms, nout, g, batch)[0]
    ninv = pow(n, -1, p)
    assert got == [x * ninv % p for x in model_accumulate(terms, key, rows, psi, n, p, nterms, nout, g, batch)]
    assert [int(x) for x in fast_accumulate_plane(terms, key, rows, psi, n, p, nterms, nout, g, batch)] == got


@pytest.mark.parametrize("nterms", [1, 3, 4, 5, 8, 9])
@pytest.mark.parametrize("p", PRIMES32)
def test_lazy_sum_equals_the_model_with_every_operand_p_minus_1(p, nterms):
    """four products, one reduction, a 32-bit running sum: with all operands P - 1 a full chunk holds 4 (P - 1)^2, the largest value the
    kernel's 64-bit register and its reduction meet.  lazy_inner_sum asserts the register does not wrap and redc its input range."""
    assert p < 1 << 30 and 4 * (p - 1) ** 2 < R * p < 5 * (p - 1) ** 2
    n, g = 32, 2
    psi, ninv, r2 = psi_of(n, p), pow(n, -1, p), R * R % p
    xs, ys = [p - 1] * nterms, [p - 1] * nterms
    assert lazy_inner_sum(xs, ys, p) == nterms * (p - 1) ** 2 * pow(R, -1, p) % p
    es = [0, n, 2 * n - 1, (3 * n - 1) % (2 * n)]                 # the subset sums of (n, 2n - 1)
    for c in (0, 1, n - 1):
        monos = [monomial_ntt(e, psi, n, p)[c] for e in es]
        tab = [m * ninv * r2 % p for m in monos]
        want = sum(m * nterms * (p - 1) ** 2 for m in monos) * ninv % p
        assert lazy_word([xs] * 4, [ys] * 4, tab, p) == want, (p, nterms, c)
    plane = model_accumulate([p - 1] * (nterms * n), [p - 1] * ((nterms << g) * n), [n, 2 * n - 1], psi, n, p, nterms, 1, g, 1)
    for c in (0, 1, n - 1):
        tab = [m * ninv * r2 % p for m in (monomial_ntt(e, psi, n, p)[c] for e in es)]
        assert lazy_word([xs] * 4, [ys] * 4, tab, p) == plane[c] * ninv % p, (p, nterms, c)


def test_redc_range_is_tight():
    p = PRIMES32[-1]
    assert redc(R * p - 1, p) == (R * p - 1) * pow(R, -1, p) % p and redc(0, p) == 0
    with pytest.raises(AssertionError):
        redc(R * p, p)
    with pytest.raises(AssertionError):
        redc(5 * (p - 1) ** 2, p)                                   # a chunk of five would leave the range


def test_rotation_model_with_a_noiseless_key_selects_the_monomial():
    """one group of g = 2 with secret bits (1, 0): pattern t = 1 is the GGSW of 1, the others of 0 -> acc = X^(a_0) rec(X^body lut)"""
    w, n, k, beta, ell, g = 32, 32, 1, 8, 3, 2
    M, J = 1 << w, (k + 1) * ell
    rng = random.Random("nmb/noiseless")
    lut = [rng.randrange(M) for _ in range((k + 1) * n)]
    key = []
    for t in range(1 << g):
        for q in range(k + 1):
            for l in range(1, ell + 1):
                for o in range(k + 1):
                    key += [(1 << (w - beta * l)) if (t == 1 and o == q) else 0] + [0] * (n - 1)
    rot_t = [7, 40, 3]
    out = model_multibit_rotate(lut, rot_t, key, w, n, 2, k, beta, ell, g, 1)
    h = 1 << (w - beta * ell - 1)
    for q in range(k + 1):
        want = rotate(rotate(lut[q * n:(q + 1) * n], 3, M), 7, M)
        assert all(min((x - y) % M, (y - x) % M) <= h for x, y in zip(out[q * n:(q + 1) * n], want))
    assert len(key) == (1 << g) * J * (k + 1) * n
