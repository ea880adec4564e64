"""The plain-int model of include/cntt_cmux.h (tests/native_cmux_model.py) against the header's statements, for w = 32, 64 and 128: the
two forms of the digits agree and reconstruct the difference, a noise-free selector selects exactly, the model tree returns the
addressed entry for every address, on trivial inputs the leaf stage is call 1, and the workspace and grid formulas.  No GPU needed."""
import random
import re

import pytest

from native_cmux_model import (HEADER, cmux_tree_workspace_bytes, cmux_workspace_bytes, digits, digits_by_offset, ggsw, grid, model_cmux, model_leaf,
                               model_tree, phase, selector_polys, stage_params, trivial)

WIDTHS = [32, 64, 128]


@pytest.mark.parametrize("w", WIDTHS)
def test_digits_of_the_difference_in_both_forms(w):
    """the sequential rule and the offset form of the kernels give the same digits; with base_log * levels = w they reconstruct the
    difference exactly, with s > 0 to within half a step 2^s"""
    rng = random.Random(w)
    M = 1 << w
    words = [0, 1, M - 1, M // 2, M // 2 - 1, M // 2 + 1] + [rng.randrange(M) for _ in range(64)]
    for beta, ell in [(w, 1), (w // 2, 2), (w // 4, 4), (1, w), (7, 3), (5, 1), (w - 1, 1), (w // 2 - 1, 2)]:
        s = w - beta * ell
        assert s >= 0
        for c0 in words:
            for c1 in (words[0], words[2], words[3], rng.randrange(M)):
                d = (c1 - c0) % M
                dig = digits(d, w, beta, ell)
                assert dig == digits_by_offset(d, w, beta, ell), (w, beta, ell, d)
                assert all(-(1 << beta) // 2 <= x < (1 << beta) // 2 for x in dig)
                back = sum(x << (w - beta * l) for l, x in enumerate(dig, 1)) % M
                err = (back - d) % M
                assert min(err, M - err) <= ((1 << s) >> 1), (w, beta, ell, d)
                if s == 0:
                    assert back == d
    assert digits(0, w, 7, 3) == [0, 0, 0]           # the zero masks of a trivial ciphertext add nothing


@pytest.mark.parametrize("w,k", [(32, 1), (64, 0), (64, 2), (128, 1)])
def test_noise_free_selector_selects_exactly(w, k):
    rng = random.Random(w * 10 + k)
    n, M = 8, 1 << w
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    c0, c1 = ([rng.randrange(M) for _ in range((k + 1) * n)] for _ in range(2))
    for beta, ell in ((w // 2, 2), (w // 4, 4)):
        for bit in (0, 1):
            sel = ggsw(rng, w, S, bit, n, beta, ell)
            assert len(sel) == selector_polys(k, ell) * n
            got = model_cmux(c0, c1, sel, w, k, n, beta, ell)
            assert phase(got, S, w) == phase(c1 if bit else c0, S, w), (w, k, bit)


@pytest.mark.parametrize("w,k", [(32, 1), (64, 1), (64, 0), (128, 1)])
def test_model_tree_returns_exactly_the_addressed_entry(w, k):
    """n = 8, M = 1, 2, 4, 8, every address, base_log * levels = w: noise-free selectors of the address bits under a binary key leave a
    ciphertext whose phase is lut[address]; selectors that are the bare gadget leave the trivial ciphertext itself"""
    rng = random.Random(w + k)
    n, M = 8, 1 << w
    beta, ell = w // 2, 2
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    assert stage_params(8) == [(4, 2), (2, 1), (1, 0)]
    bare = []
    for bit in (0, 1):
        g = []
        for q in range(k + 1):
            for l in range(1, ell + 1):
                for o in range(k + 1):
                    g += [(bit << (w - beta * l)) % M if o == q else 0] + [0] * (n - 1)
        bare.append(g)
    for m in (1, 2, 4, 8):
        depth = m.bit_length() - 1
        lut = [[rng.randrange(M) for _ in range(n)] for _ in range(m)]
        real = [[ggsw(rng, w, S, bit, n, beta, ell) for bit in (0, 1)] for _ in range(depth)]
        for a in range(m):
            sels = [v for i in range(depth) for v in real[i][(a >> i) & 1]]
            assert phase(model_tree(lut, sels, w, m, k, n, beta, ell), S, w) == lut[a], (w, k, m, a)
            sels = [v for i in range(depth) for v in bare[(a >> i) & 1]]
            assert model_tree(lut, sels, w, m, k, n, beta, ell) == trivial(lut[a], k, n), (w, k, m, a)


@pytest.mark.parametrize("w,k,beta,ell", [(32, 1, 3, 2), (64, 2, 4, 3), (64, 0, 7, 2), (128, 1, 40, 3), (32, 1, 16, 2)])
def test_leaf_stage_is_call_1_on_trivial_ciphertexts(w, k, beta, ell):
    rng = random.Random(w + 7 * k)
    n, M = 8, 1 << w
    sel = [rng.randrange(M) for _ in range(selector_polys(k, ell) * n)]       # any selector: the statement is about the words
    f0, f1 = ([rng.randrange(M) for _ in range(n)] for _ in range(2))
    assert model_leaf(f0, f1, sel, w, k, n, beta, ell) == model_cmux(trivial(f0, k, n), trivial(f1, k, n), sel, w, k, n, beta, ell)


def test_workspace_formulas_and_grid_rule():
    assert cmux_workspace_bytes(32, 8, 1, 3, 5) == 5 * 2 * 3 * 32 * 8
    assert cmux_workspace_bytes(16, 4, 0, 1, 1) == 256                        # 64 bytes, rounded up
    assert cmux_workspace_bytes(32, 16, 1, 3, 5) == 5 * 2 * 3 * 32 * 16
    # M = 8 at n = 32, k = 1, levels = 3, batch = 5 on 8-byte words: H = 4, Q = 2 -> digits max(5*4*3, 5*2*2*3) = 60 polynomials
    assert cmux_tree_workspace_bytes(32, 8, 8, 1, 3, 5) == 60 * 32 * 8 + 5 * 4 * 2 * 32 * 8 + 5 * 2 * 2 * 32 * 8
    assert cmux_tree_workspace_bytes(32, 8, 8, 3, 3, 5) == 5 * 2 * 4 * 3 * 32 * 8 + 5 * 4 * 4 * 32 * 8 + 5 * 2 * 4 * 32 * 8   # Q (k + 1) > H
    assert cmux_tree_workspace_bytes(32, 8, 1, 1, 3, 5) == 0                  # one entry: the trivial ciphertext, no workspace
    assert cmux_tree_workspace_bytes(32, 8, 2, 1, 3, 5) == 5 * 3 * 32 * 8 + 5 * 2 * 32 * 8
    assert cmux_tree_workspace_bytes(32, 16, 2, 1, 3, 5) == 5 * 3 * 32 * 16 + 5 * 2 * 32 * 16
    assert grid(0, 10, 8) == 1 and grid(7, 10, 8) == 7 and grid(2048, 4, 4) == 2048 and grid(5000, 14, 16) == 2048
    flat = re.sub(r"[\s*]+", " ", open(HEADER).read())                         # ... and they are the header's
    assert "up(batch (k + 1) levels n wb)" in flat
    assert "up(max(batch H levels, batch Q (k + 1) levels) n wb) + up(batch H (k + 1) n wb) + up(batch Q (k + 1) n wb)" in flat
    assert "one per polynomial up to 8 per CU of a 256-CU part" in flat
