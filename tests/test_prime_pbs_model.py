"""The pure-int model of include/cntt_prime_pbs.h -- source modes mod p, the signed gadget decomposition of the balanced lift with an
unmasked top digit, the exact modulus switch Z_p -> Z_2n, sample extraction -- which tests/test_gpu_prime_pbs.py imports and compares the
kernels with, checked here against its own specification: digit ranges, exact integer reconstruction, the error bound, the rounding
against fractions.Fraction, the extraction phase identity and a noiseless external-product phase identity under the header's key
convention.  Also replayed: the one-addition form of the digits that the kernel uses (csrc/prime_pbs.hpp), word width included, so
that a slip in that derivation shows without a GPU.  No GPU needed."""
from fractions import Fraction

import numpy as np
import pytest

P62 = 4611686018427322369          # the headline prime (lazy class)
PM64 = 18446744069414584321        # 2^64 - 2^32 + 1, W = 64
P50 = 1125899904679937              # below 2^50 (the 64-bit class on doubles)
P63 = 9223372036853661697         # 63-bit (strict range)
P30 = 1062862849
P32 = 4293918721                   # above 2^31
PRIMES = [P62, PM64, P50, P63, P32, P30, 12289, 97]


# -- the model ----------------------------------------------------------------------------------------------------------------------
def wbits(p):
    return p.bit_length()


def lift(x, p):
    return x if x <= (p - 1) // 2 else x - p


def source(f, a, p, mode):
    """f: n ints below p; a < 2n -> the source polynomial of cntt_prime_pbs.h"""
    if mode == "plain":
        return list(f)
    n = len(f)
    g = []
    for i in range(n):
        t = (i - a) % (2 * n)
        v = f[t % n]
        g.append((-v) % p if t >= n else v)
    if mode == "cmux":
        g = [(x - y) % p for x, y in zip(g, f)]
    return g


def signed_digits(x, p, beta, ell):
    """[d_1 .. d_ell] as signed ints: the sequential rule of the header, word for word"""
    W, B = wbits(p), 1 << beta
    s = W - beta * ell
    assert beta >= 1 and ell >= 1 and s >= 0
    xp = lift(x, p)
    state = (xp + (1 << (s - 1))) >> s if s else xp           # Python's >> floors towards minus infinity
    out = []
    for _ in range(ell - 1):
        d = state % B
        state = (state - d) // B
        if d >= B // 2:
            d -= B
            state += 1
        out.append(d)
    out.append(state)                                         # the top digit, unmasked
    return out[::-1]


def digits(x, p, beta, ell):
    """the stored form: canonical residues"""
    return [d % p for d in signed_digits(x, p, beta, ell)]


def model_terms_element(elem, a, p, beta, ell, mode="cmux"):
    """elem: npolys lists of n ints -> npolys * ell lists, term order q * ell + (l - 1)"""
    terms = []
    for f in elem:
        cols = [digits(x, p, beta, ell) for x in source(f, a, p, mode)]
        terms += [[c[l] for c in cols] for l in range(ell)]
    return terms


def ms(x, p, logn):
    two_n = 2 << logn
    return ((2 * x * two_n + p) // (2 * p)) % two_n


def model_modswitch(lwe, L, batch, p, logn):
    """lwe: batch * (L + 1) ints -> rot_t, (L + 1) * batch ints, transposed, body row negated"""
    two_n = 2 << logn
    out = [0] * ((L + 1) * batch)
    for b in range(batch):
        for i in range(L + 1):
            m = ms(lwe[b * (L + 1) + i], p, logn)
            out[i * batch + b] = (two_n - m) % two_n if i == L else m
    return out


def model_extract(glwe, h, p):
    """glwe: k + 1 lists of n ints -> k n + 1 ints"""
    n, k = len(glwe[0]), len(glwe) - 1
    out = []
    for q in range(k):
        out += [glwe[q][h - j] if j <= h else (-glwe[q][h - j + n]) % p for j in range(n)]
    return out + [glwe[k][h]]


def negacyclic(a, b, p):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            if i + j < n:
                out[i + j] = (out[i + j] + x * y) % p
            else:
                out[i + j - n] = (out[i + j - n] - x * y) % p
    return out


def kernel_form_digits(x, p, beta, ell, tb):
    """csrc/prime_pbs.hpp replayed on tb-bit words: y = x' + off mod 2^tb, the bit `neg`, bit fields for the levels below the top."""
    M = 1 << tb
    W = wbits(p)
    s, sh1 = W - beta * ell, W - beta
    off = (1 << (s - 1)) if s else 0
    for l in range(2, ell + 1):
        off += 1 << (W - beta * l + beta - 1)
    assert off < (1 << (W - 1)) < p
    hp, thr = (p - 1) // 2, p - off
    mask, half = (1 << beta) - 1, 1 << (beta - 1)
    topsub = (1 << (tb - sh1)) % M if sh1 else 0
    hi = x > hp
    y = (x + off - (p if hi else 0)) % M
    t = ((y >> sh1) - (topsub if hi and x < thr else 0)) % M
    out = [(t + p) % M if t >> (tb - 1) else t]
    sh = sh1
    for _ in range(1, ell):
        sh -= beta
        e = (y >> sh) & mask
        out.append(e - half if e >= half else (e + p - half) % M)
    return out


def bit_serial_ms(x, p, logn, tb):
    """the kernel's modulus switch: logn + 2 doublings with a conditional subtraction on tb-bit words"""
    M, r, q = 1 << tb, x, 0
    for _ in range(logn + 2):
        carry = r >> (tb - 1)
        r = (r << 1) % M
        q <<= 1
        if carry or r >= p:
            r = (r - p) % M
            q |= 1
    return ((q + 1) >> 1) % (2 << logn)


# -- the inputs the GPU tests share -------------------------------------------------------------------------------------------------
def settings(p):
    """(base_log, levels) of the issue that are valid for p; (W, 1) always is"""
    W = wbits(p)
    cand = [(1, 1), (8, 3), (23, 1), (31, 2), (16, 4), (W, 1)]
    return sorted({(b, l) for b, l in cand if b * l <= W})


def edge_words(p, beta, ell):
    """0, 1, p - 1, (p - 1) / 2 and its neighbours, and the words whose rounding lands on +- B^levels / 2 and next to it"""
    W = wbits(p)
    s = W - beta * ell
    h = (p - 1) // 2
    words = {0, 1, 2, p - 1, p - 2, h, h + 1, h - 1}
    top = (1 << (beta * ell - 1)) << s          # (B^levels / 2) 2^s
    for c in (top, -top):
        for d in (-(1 << s), -(1 << (s - 1)) - 1, -(1 << (s - 1)), -(1 << (s - 1)) + 1, -1, 0, 1, (1 << (s - 1)) - 1, 1 << (s - 1)) if s else (-1, 0, 1):
            v = c + d
            if -h <= v <= h:
                words.add(v % p)
    return sorted(words)


def modswitch_words(p, logn, rng, count=24):
    two_n = 2 << logn
    words = {0, 1, p - 1, (p + 1) // 2, (p - 1) // 2}
    for k in (1, 2, two_n // 2, two_n - 1):
        # the boundary between k - 1 and k lies at (2 k - 1) p / (2 * 2n)
        c = (2 * k - 1) * p // (2 * two_n)
        words |= {max(c - 1, 0), c, min(c + 1, p - 1), k * p // two_n, min(k * p // two_n + 1, p - 1)}
    words |= {int(rng.integers(0, p, dtype=np.uint64)) for _ in range(count)}
    return sorted(words)


# -- the model against its specification --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PRIMES)
def test_digit_ranges_reconstruction_and_error_bound(p):
    W = wbits(p)
    rng = np.random.default_rng(p % 1000)
    for beta in range(1, W + 1):
        for ell in range(1, W // beta + 1):
            if W > 16 and (beta, ell) not in settings(p) and (beta * ell) % 7 != 0 and beta * ell != W:
                continue
            B, s = 1 << beta, W - beta * ell
            xs = edge_words(p, beta, ell) + [int(rng.integers(0, p, dtype=np.uint64)) for _ in range(6)]
            for x in xs:
                d = signed_digits(x, p, beta, ell)
                assert len(d) == ell
                assert all(-B // 2 <= v < B // 2 for v in d[1:]), (p, beta, ell, x, d)
                assert -B // 2 <= d[0] <= B // 2, (p, beta, ell, x, d)
                total = sum(v << (W - beta * (l + 1)) for l, v in enumerate(d))
                xp = lift(x, p)
                r = (xp + (1 << (s - 1))) >> s if s else xp
                assert total == r << s                                   # as integers: nothing wraps
                assert abs(total - xp) <= ((1 << (s - 1)) if s else 0)
                assert (sum(c * pow(2, W - beta * (l + 1), p) for l, c in enumerate(digits(x, p, beta, ell))) - total) % p == 0


@pytest.mark.parametrize("p", [97, 12289])
def test_both_ends_of_the_top_digit_are_reachable(p):
    W = wbits(p)
    seen = set()
    for beta, ell in ((1, 1), (2, 1), (1, 2), (2, 2), (3, 2)):
        if beta * ell > W:
            continue
        tops = {signed_digits(x, p, beta, ell)[0] for x in range(p)}
        B = 1 << beta
        assert min(tops) >= -B // 2 and max(tops) <= B // 2
        seen |= {t == B // 2 for t in tops} | {("low", t == -B // 2) for t in tops}
    assert True in seen and ("low", True) in seen


@pytest.mark.parametrize("p", PRIMES)
def test_kernel_form_equals_the_sequential_rule(p):
    """the one-addition form on 32- / 64-bit words, the carry case W = word width with base_log * levels = W included"""
    W = wbits(p)
    tbs = [64] if W > 32 else [32, 64]
    rng = np.random.default_rng(p % 999)
    pairs = settings(p) + [(b, l) for b in (1, 2, 3, 5, 7, 11, 16, 21, 32) for l in (1, 2, 3, 4, 6) if b * l <= W]
    if W % 2 == 0:
        pairs.append((W // 2, 2))
    for beta, ell in pairs:
        xs = edge_words(p, beta, ell) + [int(rng.integers(0, p, dtype=np.uint64)) for _ in range(40)]
        for tb in tbs:
            for x in xs:
                assert kernel_form_digits(x, p, beta, ell, tb) == digits(x, p, beta, ell), (p, beta, ell, tb, x)
    if p < 20000:
        for beta, ell in pairs:
            for x in range(p):
                assert kernel_form_digits(x, p, beta, ell, 32) == digits(x, p, beta, ell), (p, beta, ell, x)


@pytest.mark.parametrize("p", PRIMES)
def test_modswitch_is_round_to_nearest(p):
    rng = np.random.default_rng(p % 997)
    tb = 64 if wbits(p) > 32 else 32
    for logn in range(4, 16):
        two_n = 2 << logn
        for x in modswitch_words(p, logn, rng):
            exact = Fraction(x * two_n, p)
            nearest = int(exact + Fraction(1, 2))
            assert abs(exact - nearest) < Fraction(1, 2)                 # p is odd: never a tie
            assert ms(x, p, logn) == nearest % two_n, (p, logn, x)
            assert bit_serial_ms(x, p, logn, tb) == ms(x, p, logn), (p, logn, x)
    assert ms(p - 1, p, 4) == 0                                          # rounds up to 2n, which wraps


def test_modswitch_model_layout():
    p, logn, L, batch = 12289, 4, 2, 3
    lwe = list(range(100, 100 + batch * (L + 1)))
    rot = model_modswitch(lwe, L, batch, p, logn)
    assert rot[1 * batch + 2] == ms(lwe[2 * (L + 1) + 1], p, logn)
    assert rot[L * batch + 1] == (32 - ms(lwe[1 * (L + 1) + L], p, logn)) % 32


@pytest.mark.parametrize("p", [PM64, P62, 12289])
@pytest.mark.parametrize("k", [1, 2])
def test_extraction_model_satisfies_the_phase_identity(p, k):
    """<extract(ct, h) mask, flattened key> subtracted from its body is coefficient h of body - sum_q A_q S_q (schoolbook) mod p."""
    n = 16
    rng = np.random.default_rng(k)
    glwe = [[int(x) for x in rng.integers(0, p, size=n, dtype=np.uint64)] for _ in range(k + 1)]
    key = [[int(x) for x in rng.integers(0, 2, size=n)] for _ in range(k)]
    phase = list(glwe[k])
    for q in range(k):
        phase = [(x - y) % p for x, y in zip(phase, negacyclic(glwe[q], key[q], p))]
    flat = [s for q in key for s in q]
    for h in (0, 1, 7, n - 1):
        lwe = model_extract(glwe, h, p)
        assert len(lwe) == k * n + 1
        assert (lwe[-1] - sum(a * s for a, s in zip(lwe, flat))) % p == phase[h], (p, k, h)


def test_source_modes():
    p, n = 97, 16
    f = list(range(1, n + 1))
    f[3] = 0
    assert source(f, 0, p, "rotate") == f and source(f, 0, p, "cmux") == [0] * n
    assert source(f, n, p, "rotate") == [(-x) % p for x in f]
    g = source(f, 1, p, "rotate")
    assert g[0] == (-f[n - 1]) % p and g[1:] == f[:n - 1]
    assert source(f, 2 * n - 1, p, "rotate") == f[1:] + [(-f[0]) % p]
    assert source(source(f, 5, p, "rotate"), 2 * n - 5, p, "rotate") == f
    assert source(f, 3, p, "cmux") == [(x - y) % p for x, y in zip(source(f, 3, p, "rotate"), f)]


@pytest.mark.parametrize("p,beta,ell", [(PM64, 16, 4), (PM64, 8, 3), (P62, 8, 3), (12289, 2, 7), (P30, 10, 3)])
def test_noiseless_external_product_phase_identity(p, beta, ell):
    """The header's key convention at n = 16, k = 1: row (q, l) = a GLWE encryption of zero with m 2^(W - beta l) mod p added on
    polynomial q (m a message polynomial, here the bit s_i times 1).  Then the phase of sum_j digit_j (*) row_j is m times the phase of
    the decomposed GLWE up to the rounding: |error| <= (1 + k n) 2^(s-1) per coefficient (the body's own rounding, and k products of
    rounding errors with a binary key polynomial)."""
    n, k, W = 16, 1, wbits(p)
    s = W - beta * ell
    rng = np.random.default_rng(beta * 100 + ell)
    S = [[int(x) for x in rng.integers(0, 2, size=n)] for _ in range(k)]
    glwe = [[int(x) for x in rng.integers(0, p, size=n, dtype=np.uint64)] for _ in range(k + 1)]

    def phase_of(ct):
        ph = list(ct[k])
        for q in range(k):
            ph = [(x - y) % p for x, y in zip(ph, negacyclic(ct[q], S[q], p))]
        return ph

    for bit in (0, 1):
        rows = []
        for q in range(k + 1):
            for l in range(1, ell + 1):
                mask = [[int(x) for x in rng.integers(0, p, size=n, dtype=np.uint64)] for _ in range(k)]
                body = [0] * n
                for c in range(k):
                    body = [(x + y) % p for x, y in zip(body, negacyclic(mask[c], S[c], p))]
                row = mask + [body]
                row[q][0] = (row[q][0] + bit * pow(2, W - beta * l, p)) % p
                rows.append(row)
        terms = model_terms_element(glwe, 0, p, beta, ell, mode="plain")
        out = [[0] * n for _ in range(k + 1)]
        for j, t in enumerate(terms):
            for o in range(k + 1):
                out[o] = [(x + y) % p for x, y in zip(out[o], negacyclic(t, rows[j][o], p))]
        want = phase_of(glwe)
        got = phase_of(out)
        bound = (1 + k * n) * ((1 << (s - 1)) if s else 0)
        for x, y in zip(got, want):
            assert abs(lift((x - bit * y) % p, p)) <= bit * bound, (p, beta, ell, bit)
