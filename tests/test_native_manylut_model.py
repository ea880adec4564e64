"""The plain-int model of include/cntt_manylut.h (tests/native_manylut_model.py) against the header's statements, for w = 32, 64, 128: the
coarse modulus switch against the ms of cntt_pbs.h for the smaller ring and against the kernel's top-32-bit form, its ties and its wrap;
the interleaved table -- coefficient h of X^(-a) v for every a = 0 mod 2^t is +-f_h(a / 2^t); the extraction of several indices against
single ones; with noise-free keys every u[b][l] of the one-rotation circuit bootstrap has the phase exactly 0 or G_l on every exponent the
header's bound D admits, and is read wrong one step outside it; its selectors drive the model tree to every entry at M = 4; the header's
formulas.  No GPU needed."""
import random
import re

import pytest

from native_cbs_model import G, bsk, cbs_workspace_bytes, flatten, fpksk, lwe_encrypt, lwe_phase, model_circuit_bootstrap, ms, rotate
from native_cmux_model import model_tree, phase
from native_manylut_model import (HEADER, cbs_manylut_workspace_bytes, cbs_table, interleave, model_circuit_bootstrap_manylut, model_extract,
                                  model_extract_many, model_modswitch_coarse, model_u_manylut, ms_coarse, top32_ms_coarse)
from native_cbs_model import model_extract as model_extract_zero

WIDTHS = [32, 64, 128]
GADGETS = {32: ((8, 4), (8, 4), (5, 3)), 64: ((16, 4), (16, 4), (9, 3)), 128: ((32, 4), (16, 8), (21, 3))}   # pbs, ks (both fill w), cbs


def switch_words(w, logn, t):
    """0, 1, the all-ones word, and both sides of every boundary of the coarse grid: the exact ties j 2^w / 2n' + half a step, one below
    and one above them, and the grid points themselves"""
    M, step = 1 << w, 1 << (w - (logn - t) - 1)
    words = {0, 1, M - 1, M >> 1, (M >> 1) - 1}
    for j in range(2 << (logn - t)):
        c = j * step
        words |= {x % M for x in (c - 1, c, c + 1, c + step // 2 - 1, c + step // 2, c + step // 2 + 1)}
    return sorted(words)


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("logn", [3, 5, 10])
def test_coarse_modswitch_is_the_switch_of_the_smaller_ring_shifted(w, logn):
    M = 1 << w
    for t in (0, 1, logn - 1, logn):
        step = 1 << (w - (logn - t) - 1)
        for x in switch_words(w, logn, t):
            got = ms_coarse(x, w, logn, t)
            assert got == ms(x, w, logn - t) << t, (w, logn, t, x)              # the ms of cntt_pbs.h for n', shifted
            assert got % (1 << t) == 0 and got < (2 << logn), (w, logn, t, x)
            assert top32_ms_coarse(x, w, logn, t) == got, (w, logn, t, x)       # only the top 32 bits are read
            if t == 0:
                assert got == ms(x, w, logn)
        # exact ties go up; the all-ones word wraps to 0
        for j in (0, 1, (1 << (logn - t)) - 1, (2 << (logn - t)) - 1):
            tie = j * step + step // 2
            assert ms_coarse(tie, w, logn, t) == ((j + 1) % (2 << (logn - t))) << t, (w, logn, t, j)
            assert ms_coarse(tie - 1, w, logn, t) == j << t, (w, logn, t, j)
        assert ms_coarse(M - 1, w, logn, t) == 0
    # the layout: transposed, the body row negated mod 2n and still on the coarse grid
    rng = random.Random(w * logn)
    L, batch, t = 3, 2, 1
    lwe = [rng.randrange(M) for _ in range(batch * (L + 1))]
    rot = model_modswitch_coarse(lwe, L, batch, w, logn, t)
    assert all(r % 2 == 0 and r < (2 << logn) for r in rot)
    assert rot[L * batch + 1] == ((2 << logn) - ms_coarse(lwe[1 * (L + 1) + L], w, logn, t)) % (2 << logn)
    assert rot[2 * batch + 1] == ms_coarse(lwe[1 * (L + 1) + 2], w, logn, t)
    # the bit values of the circuit bootstrap lie on the coarse grid while 2^t <= n / 2
    for t in range(logn):
        assert ms_coarse(1 << (w - 2), w, logn, t) == (1 << logn) // 2
        assert ms_coarse((1 << (w - 1)) + (1 << (w - 2)), w, logn, t) == 3 * (1 << logn) // 2


@pytest.mark.parametrize("n", [16, 32])
def test_interleaved_table_and_many_index_extraction(n):
    """for every a = 0 mod 2^t in Z_2n and every h < 2^t, coefficient h of X^(-a) v is f_h(a / 2^t) for a < n and -f_h(a / 2^t - n') beyond"""
    w = 64
    M = 1 << w
    rng = random.Random(n)
    for t in range(4):
        nprime = n >> t
        fs = [[rng.randrange(M) for _ in range(nprime)] for _ in range(1 << t)]
        v = interleave(fs, n, t)
        for a in range(0, 2 * n, 1 << t):
            rotated = rotate(v, (2 * n - a) % (2 * n), w)          # X^(-a) v
            m = a >> t
            for h in range(1 << t):
                want = fs[h][m] if a < n else (-fs[h][m - nprime]) % M
                assert rotated[h] == want, (n, t, a, h)
        # the extraction of `count` indices is `count` single extractions, row after row; index 0 is the extraction of cntt_cbs.h's model
        k = 2
        glwe = [[rng.randrange(M) for _ in range(n)] for _ in range(k + 1)]
        assert model_extract(glwe, 0, w) == model_extract_zero(glwe, w)
        for count in (1, 7, 8, 9, n):
            got = model_extract_many(glwe, count, w)
            assert len(got) == count * (k * n + 1)
            for h in range(count):
                row = got[h * (k * n + 1):(h + 1) * (k * n + 1)]
                assert row == model_extract(glwe, h, w), (n, count, h)
                # coefficient h of X^j glwe[p] is the word j of the row
                assert row[n + 3] == rotate(glwe[1], 3, w)[h] and row[k * n] == glwe[k][h]


def noise_free_keys(rng, w, n, k, s_lwe, pbs, ks):
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    return S, bsk(rng, w, s_lwe, S, n, *pbs), fpksk(rng, w, S, n, *ks)


@pytest.mark.parametrize("w", WIDTHS)
def test_one_rotation_phases_are_exact_on_every_exponent_the_bound_admits(w):
    """n = 32, k = 1, t = 2, Lc = 3, the PBS gadget fills w.  The header: the bit is read right when D = (L + 1) / 2 + |e| 2n' / 2^w <
    n / 2^(t + 1) = 4 coarse steps.
    L = 0: the body alone is switched.  An input noise e = d 2^w / 2n' puts the exponent exactly d steps off n / 2 (3 n / 2): D = 1 / 2 +
    |d| < 4 admits d = -3 .. 3, each also with the largest offset that still rounds to the same step, and every u[b][l] has the phase
    exactly 0 / G_l.  d = 4 = n / 2^(t + 1) is outside the bound and IS read wrong: the exponent reaches n (2n = 0) and the sign flips,
    so the bound is tight in kind.
    L = 3 with all three key bits set: four switched words enter, D = 2 + |e| 2n' / 2^w < 4 admits |e| < 2^w / n' = 2^(w - 3)."""
    n, k, t, Lc = 32, 1, 2, 3
    pbs, ks, cbs = GADGETS[w]
    assert cbs[1] == Lc and Lc <= 1 << t <= n // 2
    M, nprime = 1 << w, n >> t
    step = M // (2 * nprime)
    rng = random.Random(3000 + w)
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    s_in = flatten(S)
    margin = n >> (t + 1)
    for bit in (0, 1):
        for d in range(-margin + 1, margin):
            assert 0.5 + abs(d) < margin
            for off in (0, step // 2 - 1, -(step // 2)):                      # the whole interval that rounds to this step, ties up
                lwe = [(bit * (M >> 1) + d * step + off) % M]
                us = model_u_manylut(lwe, [], w, 0, k, n, *pbs, cbs[0], Lc, t)
                assert len(us) == Lc
                for l, u in enumerate(us, start=1):
                    assert len(u) == k * n + 1 and lwe_phase(u, s_in, w) == bit * G(w, cbs[0], l), (w, bit, d, off, l)
        # just outside: D = 1 / 2 + 4 >= 4, and the bit is read as its complement
        us = model_u_manylut([(bit * (M >> 1) + margin * step) % M], [], w, 0, k, n, *pbs, cbs[0], Lc, t)
        for l, u in enumerate(us, start=1):
            assert lwe_phase(u, s_in, w) == (1 - bit) * G(w, cbs[0], l), (w, bit, l)
    L, s_lwe = 3, [1, 1, 1]
    B = bsk(rng, w, s_lwe, S, n, *pbs)
    edge = (1 << (w - 3)) - 1
    assert (L + 1) * M + 4 * edge * nprime < 2 * margin * M <= (L + 1) * M + 4 * (edge + 1) * nprime      # D < margin, doubled, times 2^w
    for bit in (0, 1):
        for e in (0, edge, -edge, rng.randint(-edge, edge)):
            lwe = lwe_encrypt(rng, w, s_lwe, (bit * (M >> 1) + e) % M)
            for l, u in enumerate(model_u_manylut(lwe, B, w, L, k, n, *pbs, cbs[0], Lc, t), start=1):
                assert lwe_phase(u, s_in, w) == bit * G(w, cbs[0], l), (w, bit, e, l)


@pytest.mark.parametrize("w", [32, 64])
def test_selectors_of_the_one_rotation_form_drive_the_model_tree_to_every_entry(w):
    """n = 16, L = 2, k = 1, t = 2, Lc = 3: (L + 1) / 2 = 1.5 < n / 2^(t + 1) = 2.  The keyswitch gadget fills w, so the selector rows
    are exact and the tree's only error is the rounding of its own decomposition, s = w - cbs_base_log Lc bits: at most
    (1 + k n) 2^(s - 1) per CMux (cntt_cmux.h), two stages at M = 4."""
    n, L, k, t = 16, 2, 1, 2
    pbs, ks, cbs = GADGETS[w]
    M = 1 << w
    rng = random.Random(3100 + w)
    s_lwe = [1, 1]
    S, B, F = noise_free_keys(rng, w, n, k, s_lwe, pbs, ks)
    sel = {}
    for bit in (0, 1):
        lwe = lwe_encrypt(rng, w, s_lwe, bit << (w - 1))
        sel[bit] = model_circuit_bootstrap_manylut(lwe, B, F, w, L, k, n, *pbs, *ks, *cbs, t)
    entries = [[rng.randrange(8) for _ in range(n)] for _ in range(4)]
    lut = [[m << (w - 3) for m in row] for row in entries]
    s = w - cbs[0] * cbs[1]
    bound = 2 * (1 + k * n) * (1 << (s - 1))
    for a in range(4):
        ph = phase(model_tree(lut, sel[a & 1] + sel[a >> 1], w, 4, k, n, *cbs), S, w)
        assert [(((x >> (w - 4)) + 1) >> 1) % 8 for x in ph] == entries[a], (w, a)
        assert all(min((x - y) % M, (y - x) % M) <= bound for x, y in zip(ph, lut[a])), (w, a)


def test_t_zero_is_the_circuit_bootstrap_of_cntt_cbs_h():
    w, n, L, k = 32, 16, 2, 1
    pbs, ks, cbs = (8, 4), (7, 3), (5, 1)
    rng = random.Random(5)
    s_lwe = [1, 1]
    S, B, F = noise_free_keys(rng, w, n, k, s_lwe, pbs, ks)
    lwe = lwe_encrypt(rng, w, s_lwe, 1 << 31, noise=3)
    assert model_circuit_bootstrap_manylut(lwe, B, F, w, L, k, n, *pbs, *ks, *cbs, 0) == \
        model_circuit_bootstrap(lwe, B, F, w, L, k, n, *pbs, *ks, *cbs)
    assert cbs_table(w, k, n, 5, 1, 0)[k] == [(1 << 32) - (1 << (32 - 5 - 1))] * n
    assert cbs_table(w, k, n, 5, 3, 2)[k][:8] == [(1 << 32) - (1 << 26), (1 << 32) - (1 << 21), (1 << 32) - (1 << 16), 0] * 2


def test_header_formulas_are_the_models():
    flat = re.sub(r"[\s*]+", " ", open(HEADER).read())
    for text in ("ms_t(x) = 2^t ((((x >> (w - (logn - t) - 2)) + 1) >> 1) mod 2n')", "ms_0 = ms, word for word", "v[m 2^t + h]",
                 "up((L + 1) batch 4) + up((k + 1) n wb) + up(batch (k + 1) pbs_levels n wb) + up(batch (k + 1) n wb) + up(E R 4) "
                 "+ up(S (k + 1) E (k + 1) n wb) + up((k + 1) E (k + 1) n wb)",
                 "v[m 2^t + h] = 2^w - H_(h+1) for h < Lc, 0 for Lc <= h < 2^t", "Lc <= 2^t <= n / 2", "batch (k + 1) pbs_levels >= 2^32",
                 "n / 2^(t + 1) steps of the coarse switch", "D = (L + 1) / 2 + |e| 2n' / 2^w", "D < n / 2^(t + 1)",
                 "profiles/r30_native_manylut.txt"):
        assert text in flat, text
    # one rotation: everything but the keyswitch half is per input bit
    assert cbs_manylut_workspace_bytes(32, 8, 3, 1, 2, 3, 2, 3) == 256 + 512 + 3072 + 1536 + 2560 + 12288 + 6144
    assert cbs_manylut_workspace_bytes(32, 8, 3, 1, 2, 3, 1, 3) == cbs_workspace_bytes(32, 8, 3, 1, 2, 3, 1, 3) - 1536 + 512
