"""The model of tests/native_automorphism_model.py against its specification (include/cntt_automorphism.h), on the CPU, for w = 32, 64
and 128: the gather form is the scatter that defines sigma_t; the group law; the slot rule against an O(n^2) evaluation at
psi^(2 bitrev(c) + 1) and against the CPU oracle's transforms of the native plans, which pins the slot order of the Plan32 AND the
Plan52 kinds before any GPU run; the phase statements of the Galois keyswitch; the trace on noise-free keys; the workspace formulas and
the grid rule.  No GPU.

What the oracle says about call 2 (decisive for the Plan52 kinds): with the header's rule, permuting plane i of native fwd(f) gives, word
for word, the forward transform mod P_i of sigma_t applied to the residues of f -- for the Plan32 kind and for both Plan52 kinds, at
n = 16 / 32 / 1024.  So the Plan52 kinds are ACCEPTED.  The identity "fwd(sigma_t f) = perm(fwd f)" on the WORDS holds only where
sigma_t negates no non-zero word: the oracle's fwd reads a word as an unsigned integer, so -x mod 2^w = 2^w - x is not -x mod P_i.
Measured here: with random words it fails for every t != 1 on every kind, Plan32 included; with the negated sources zeroed it holds
for every t; and the inverse transform returns sigma_t f from either.  The header states exactly that."""
import random
import re

import numpy as np
import pytest

from native_automorphism_model import (HEADER, autom_gather, autom_gather_np, autom_scatter, automorphism_key, autoks_workspace_bytes, bitrev, digits,
                                       grid, model_autoks, model_trace, ntt_permutation, phase, trace_exponents, trace_keys, trace_workspace_bytes)
from oracle import pyoracle
from prime_automorphism_model import autom_gather_np as autom_gather_mod_p

WIDTHS = [32, 64, 128]
P32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801, 1068433409, 1068564481, 1069219841, 1071513601, 1073479681]
P52 = [1125899881086977, 1125899885412353, 1125899886395393, 1125899899174913, 1125899902124033, 1125899903107073]


def odd(n):
    return range(1, 2 * n, 2)


@pytest.mark.parametrize("w", WIDTHS)
def test_gather_form_is_the_scatter_definition_and_the_group_law(w):
    n, M = 16, 1 << w
    rng = random.Random("native-autom/%d" % w)
    f = [rng.randrange(M) for _ in range(n)]
    f[3], f[5] = 0, M // 2                                             # a zero stays zero; 2^(w-1) is its own negative
    assert autom_gather(f, 1, w) == f
    assert autom_gather(f, 2 * n - 1, w) == [f[0]] + [(-x) % M for x in reversed(f[1:])]
    for t in odd(n):
        assert autom_gather(f, t, w) == autom_scatter(f, t, w), t
        if w <= 64:
            a = np.array(f, dtype=np.uint32 if w == 32 else np.uint64)
            assert [int(x) for x in autom_gather_np(a, t)] == autom_scatter(f, t, w), t
        for s in (1, 3, n + 1, 2 * n - 1, 7):
            assert autom_gather(autom_gather(f, t, w), s, w) == autom_gather(f, s * t % (2 * n), w), (s, t)


def test_slot_rule_against_a_direct_evaluation():
    """one small prime, p = 97 = 1 mod 32, n = 16: slot c of the transform is f(psi^(2 bitrev(c) + 1)); sigma_t f there is f at
    psi^(t (2 bitrev(c) + 1)), which is slot c' of the rule"""
    p, n, logn = 97, 16, 4
    psi = next(g for g in range(2, p) if pow(g, n, p) == p - 1)        # a primitive 2n-th root of unity
    rng = random.Random("native-autom/slots")
    f = [rng.randrange(p) for _ in range(n)]

    def transform(g):
        return [sum(x * pow(psi, (2 * bitrev(c, logn) + 1) * i, p) for i, x in enumerate(g)) % p for c in range(n)]

    fhat = transform(f)
    for t in odd(n):
        g = [x % p for x in autom_scatter_mod(f, t, p)]
        src = ntt_permutation(t, n)
        assert transform(g) == [fhat[int(src[c])] for c in range(n)], t
        assert sorted(src.tolist()) == list(range(n))


def autom_scatter_mod(f, t, p):
    n = len(f)
    out = [0] * n
    for i, x in enumerate(f):
        e = i * t % (2 * n)
        out[e % n] = (-x) % p if e >= n else x
    return out


def words_of(ints, word):
    if word == 16:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=pyoracle.word_dtype(word))


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32", "native32_plan52", "native64_plan52"])
def test_slot_rule_against_the_oracle_for_plan32_and_plan52(kind):
    nprimes, word, is52, _ = pyoracle.NATIVE_INFO[kind]
    w = 8 * word
    rng = random.Random("native-autom/oracle/" + kind)
    for n in ([16] if is52 else []) + [32, 1024]:
        nat = pyoracle.Native.try_new(kind, n)
        assert nat is not None, (kind, n)
        f = [rng.randrange(1 << w) for _ in range(n)]
        fhat = nat.residues()
        nat.fwd(words_of(f, word), fhat)
        ts = list(odd(n)) if n <= 32 else [1, 3, n + 1, n // 2 + 1, 2 * n - 1] + [2 * rng.randrange(n) + 1 for _ in range(4)]
        subs = [pyoracle.Plan.try_new(n, (P52 if is52 else P32)[i], 64 if is52 else 32) for i in range(nprimes)]
        for t in ts:
            src = ntt_permutation(t, n)
            # 1. plane for plane, word for word: the permuted plane is the transform mod P_i of sigma_t of the residues
            for i, sub in enumerate(subs):
                p = (P52 if is52 else P32)[i]
                fi = np.array([x % p for x in f], dtype=nat.res_dtype)
                g = autom_gather_mod_p(fi, t, p).astype(nat.res_dtype)
                sub.fwd(g)
                assert np.array_equal(g, fhat[i][src]), (kind, n, t, i)
            # 2. the planes stand for sigma_t f mod 2^w: the inverse transform returns the same words as from fwd(sigma_t f)
            sig = autom_gather(f, t, w)
            direct = nat.residues()
            nat.fwd(words_of(sig, word), direct)
            literal = all(np.array_equal(direct[i], fhat[i][src]) for i in range(nprimes))      # (before inv, which works in place)
            back, back_direct = nat.words(), nat.words()
            nat.inv(back, [np.ascontiguousarray(fhat[i][src]) for i in range(nprimes)])
            nat.inv(back_direct, direct)
            assert back.any() and np.array_equal(back, back_direct), (kind, n, t, "inv")
            # 3. on the words: equal where sigma_t negates only zeros, and (measured) unequal otherwise unless t = 1
            u = [j * pow(t, -1, 2 * n) % (2 * n) for j in range(n)]
            z = list(f)
            for x in u:
                if x >= n:
                    z[x % n] = 0
            zhat, zdir = nat.residues(), nat.residues()
            nat.fwd(words_of(z, word), zhat)
            nat.fwd(words_of(autom_gather(z, t, w), word), zdir)
            assert all(np.array_equal(zdir[i], zhat[i][src]) for i in range(nprimes)), (kind, n, t, "zeroed")
            assert literal == (t == 1), (kind, n, t, "the word identity holds exactly when nothing is negated")


def binary_key(rng, k, n):
    return [[rng.randrange(2) for _ in range(n)] for _ in range(k)]


def lift(x, w):
    return x - (1 << w) if x >= 1 << (w - 1) else x


@pytest.mark.parametrize("w,k", [(32, 1), (64, 2), (128, 1), (64, 0)])
def test_noise_free_key_without_rounding_permutes_the_phase_exactly(w, k):
    n, M = 8, 1 << w
    rng = random.Random("native-autom/exact/%d/%d" % (w, k))
    S = binary_key(rng, k, n)
    beta, ell = w // 4, 4
    for t in (3, n + 1, 2 * n - 1):
        ct = [rng.randrange(M) for _ in range((k + 1) * n)]
        key = automorphism_key(rng, w, S, t, n, beta, ell)
        assert len(key) == k * ell * (k + 1) * n
        ph = phase(ct, S, w)
        rot = autom_gather(ph, t, w)
        assert phase(model_autoks(ct, key, w, t, k, n, beta, ell, False), S, w) == rot, (w, k, t)
        assert phase(model_autoks(ct, key, w, t, k, n, beta, ell, True), S, w) == [(x + y) % M for x, y in zip(rot, ph)], (w, k, t)
    ct = [rng.randrange(M) for _ in range(n)]
    assert model_autoks(ct, [], w, 5, 0, n, beta, ell, False) == autom_gather(ct, 5, w)          # k = 0: the body alone


@pytest.mark.parametrize("w,beta,ell", [(64, 7, 3), (32, 4, 3), (128, 40, 2), (32, 22, 1), (64, 2, 2)])
def test_rounding_bound_of_the_galois_keyswitch(w, beta, ell):
    """s = w - base_log * levels > 0, binary key, noise-free AK: phase(out) - sigma_t(phase(in)) = sum_r (x_r - r_r 2^s) (*) sigma_t(S_r)
    with |x - r 2^s| <= 2^(s-1) per coefficient and n coefficients of size at most 1 per product, so every coefficient lies within
    k n 2^(s-1) -- derived, not measured"""
    n, M = 8, 1 << w
    s = w - beta * ell
    assert s > 0
    rng = random.Random("native-autom/bound/%d/%d" % (w, beta))
    for k in (1, 2):
        S = binary_key(rng, k, n)
        for t in (3, n + 1, 2 * n - 1, 2 * rng.randrange(n) + 1):
            ct = [rng.randrange(M) for _ in range((k + 1) * n)]
            key = automorphism_key(rng, w, S, t, n, beta, ell)
            ph = phase(ct, S, w)
            rot = autom_gather(ph, t, w)
            for add in (False, True):
                out = model_autoks(ct, key, w, t, k, n, beta, ell, add)
                want = [(x + y) % M for x, y in zip(rot, ph)] if add else rot
                err = [abs(lift((x - y) % M, w)) for x, y in zip(phase(out, S, w), want)]
                assert max(err) <= k * n * (1 << (s - 1)), (w, k, t, add, max(err))


@pytest.mark.parametrize("w,k", [(32, 1), (64, 1), (64, 2), (128, 1)])
def test_trace_on_noise_free_keys_with_no_rounding(w, k):
    """for every steps in [0, log2 n] coefficient i of the phase is exactly 2^steps phase[i] mod 2^w where 2^steps divides i and 0
    elsewhere: the factor is not a unit, the top `steps` bits of phase[i] are lost"""
    n, logn, M = 8, 3, 1 << w
    beta, ell = w // 4, 4
    rng = random.Random("native-autom/trace/%d/%d" % (w, k))
    S = binary_key(rng, k, n)
    ct = [rng.randrange(M) for _ in range((k + 1) * n)]
    ph = phase(ct, S, w)
    keys = trace_keys(rng, w, S, logn, n, beta, ell)
    per = k * ell * (k + 1) * n
    assert trace_exponents(n, logn) == [n + 1, n // 2 + 1, 3]
    for steps in range(logn + 1):
        out = model_trace(ct, keys[:steps * per], w, steps, k, n, beta, ell)
        assert phase(out, S, w) == [(ph[i] << steps) % M if i % (1 << steps) == 0 else 0 for i in range(n)], (w, k, steps)
    assert model_trace(ct, [], w, 0, k, n, beta, ell) == ct
    assert digits(M - 1, w, beta, ell) == [0, 0, 0, -1]


def test_workspace_formulas_and_grid_rule():
    assert autoks_workspace_bytes(32, 8, 1, 3, 5) == 5 * 3 * 32 * 8
    assert autoks_workspace_bytes(16, 4, 1, 1, 1) == 256                      # 64 bytes, rounded up
    assert autoks_workspace_bytes(32, 16, 0, 3, 5) == 0
    assert trace_workspace_bytes(32, 16, 2, 3, 5) == 5 * 2 * 3 * 32 * 16 + 5 * 3 * 32 * 16
    assert trace_workspace_bytes(32, 4, 0, 3, 1) == 256
    assert grid(0, 10, 8) == 1 and grid(7, 10, 8) == 7 and grid(5000, 10, 8) == 2048
    assert grid(5000, 12, 16) == 512 and grid(5000, 13, 8) == 512 and grid(5000, 14, 4) == 512      # 64 KiB staged: 2 per CU
    assert grid(5000, 13, 16) == 2048 and grid(5000, 12, 8) == 5 * 256                              # 128 KiB: not staged; 32 KiB: 5 per CU
    flat = re.sub(r"[\s*]+", " ", open(HEADER).read())                         # ... and they are the header's
    assert "up(batch k levels n wb)" in flat and "that + up(batch (k + 1) n wb)" in flat
    assert "one per polynomial up to 8 per CU of a 256-CU part" in flat and "not a measured optimum" in flat
