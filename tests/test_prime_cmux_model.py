"""The plain-int model of include/cntt_prime_cmux.h (tests/prime_cmux_model.py) against the header's statements: the digits of c1 - c0
reconstruct it, a noise-free selector selects exactly, the model tree returns the trivial encryption of the addressed entry for every
address, and on trivial inputs the leaf stage is call 1.  No GPU needed."""
import random

import pytest

from prime_cmux_model import (cmux_tree_workspace_bytes, cmux_workspace_bytes, ggsw, grid, model_cmux, model_leaf, model_tree, phase,
                              selector_polys, stage_params, trivial)
from test_prime_pbs_model import P30, P32, P62, PM64, signed_digits, wbits

SMALL = [97, 12289]          # small primes keep the quadratic products of the plain-int model quick


@pytest.mark.parametrize("p", [P62, PM64, P30, P32, 12289, 97])
def test_digits_of_the_difference_reconstruct_it_when_nothing_is_rounded(p):
    rng = random.Random(p)
    W = wbits(p)
    splits = [(W, 1)] + [(W // ell, ell) for ell in (2, 3, 4) if W % ell == 0]
    assert splits
    for beta, ell in splits:
        assert beta * ell == W
        words = [0, 1, p - 1, (p - 1) // 2, (p + 1) // 2] + [rng.randrange(p) for _ in range(64)]
        for c0 in words:
            for c1 in (words[0], words[2], words[3], rng.randrange(p)):
                d = (c1 - c0) % p
                dig = signed_digits(d, p, beta, ell)
                assert sum(x << (W - beta * l) for l, x in enumerate(dig, 1)) % p == d, (p, beta, ell, c0, c1)
                assert all(abs(x) <= (1 << beta) // 2 for x in dig)


@pytest.mark.parametrize("p,k", [(97, 1), (12289, 0), (12289, 2)])
def test_noise_free_selector_selects_exactly(p, k):
    rng = random.Random(p * 10 + k)
    n, W = 8, wbits(p)
    beta, ell = (W, 1) if W % 2 else (W // 2, 2)
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    c0, c1 = ([rng.randrange(p) for _ in range((k + 1) * n)] for _ in range(2))
    for bit in (0, 1):
        sel = ggsw(rng, p, S, bit, n, beta, ell)
        assert len(sel) == selector_polys(k, ell) * n
        got = model_cmux(c0, c1, sel, p, k, n, beta, ell)
        assert phase(got, S, p) == phase(c1 if bit else c0, S, p), (p, k, bit)


@pytest.mark.parametrize("p,k", [(97, 1), (12289, 1), (12289, 0)])
def test_model_tree_returns_the_trivial_encryption_of_the_addressed_entry(p, k):
    """M = 8, every address: selectors that are the bare gadget (zero masks, zero noise) leave the table entry itself, zero masks and all"""
    rng = random.Random(p + k)
    n, m, W = 8, 8, wbits(p)
    beta, ell = (W, 1) if W % 2 else (W // 2, 2)
    lut = [[rng.randrange(p) for _ in range(n)] for _ in range(m)]
    assert stage_params(m) == [(4, 2), (2, 1), (1, 0)]
    bare = []
    for bit in (0, 1):
        g = []
        for q in range(k + 1):
            for l in range(1, ell + 1):
                for o in range(k + 1):
                    g += [(bit << (W - beta * l)) % p if o == q else 0] + [0] * (n - 1)
        bare.append(g)
    for a in range(m):
        sels = [w for i in range(3) for w in bare[(a >> i) & 1]]
        assert model_tree(lut, sels, p, m, k, n, beta, ell) == trivial(lut[a], k, n), (p, k, a)
    # with real (noise-free) GGSWs under a key the masks are no longer zero, the phase is the entry
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    for a in (0, 5, 7):
        sels = [w for i in range(3) for w in ggsw(rng, p, S, (a >> i) & 1, n, beta, ell)]
        assert phase(model_tree(lut, sels, p, m, k, n, beta, ell), S, p) == lut[a], (p, k, a)
    assert model_tree(lut[:1], [], p, 1, k, n, beta, ell) == trivial(lut[0], k, n)


@pytest.mark.parametrize("p,k,beta,ell", [(97, 1, 3, 2), (12289, 2, 4, 3), (12289, 0, 7, 2), (P30, 1, 10, 3)])
def test_leaf_stage_is_call_1_on_trivial_ciphertexts(p, k, beta, ell):
    rng = random.Random(p + 7 * k)
    n = 8
    sel = [rng.randrange(p) for _ in range(selector_polys(k, ell) * n)]       # any selector: the statement is about the words
    f0, f1 = ([rng.randrange(p) for _ in range(n)] for _ in range(2))
    assert model_leaf(f0, f1, sel, p, k, n, beta, ell) == model_cmux(trivial(f0, k, n), trivial(f1, k, n), sel, p, k, n, beta, ell)


def test_workspace_formulas_and_grid_rule():
    assert cmux_workspace_bytes(32, 8, 1, 3, 5) == 5 * 2 * 3 * 32 * 8
    assert cmux_workspace_bytes(16, 4, 0, 1, 1) == 256                        # 64 bytes, rounded up
    # M = 8 at n = 32, k = 1, levels = 3, batch = 5 on 8-byte words: H = 4, Q = 2 -> digits max(5*4*3, 5*2*2*3) = 60 polynomials
    assert cmux_tree_workspace_bytes(32, 8, 8, 1, 3, 5) == 60 * 32 * 8 + 5 * 4 * 2 * 32 * 8 + 5 * 2 * 2 * 32 * 8
    assert cmux_tree_workspace_bytes(32, 8, 8, 3, 3, 5) == 5 * 2 * 4 * 3 * 32 * 8 + 5 * 4 * 4 * 32 * 8 + 5 * 2 * 4 * 32 * 8   # Q (k + 1) > H
    assert cmux_tree_workspace_bytes(32, 8, 1, 1, 3, 5) == 0                  # one entry: the trivial ciphertext, no workspace
    assert cmux_tree_workspace_bytes(32, 8, 2, 1, 3, 5) == 5 * 3 * 32 * 8 + 5 * 2 * 32 * 8
    assert grid(0, 10, 8) == 1 and grid(7, 10, 8) == 7 and grid(2048, 4, 4) == 2048 and grid(5000, 14, 8) == 2048
