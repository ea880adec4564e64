"""The plain-int model of include/cntt_prime_manylut.h (tests/prime_manylut_model.py) against the header's statements: the coarse modulus
switch against its definition and against the kernel's bit-serial form, ms_0 = ms; the interleaved table -- coefficient h of X^(-a) v for
every a = 0 mod 2^t is +-f_h(a / 2^t); the extraction of several indices against single ones; with noise-free keys every u[b][l] of the
one-rotation circuit bootstrap has the phase exactly 0 or G_l, and its selectors drive the model tree to every entry at M = 8; the
many-LUT bootstrap decodes 2^t tables under noisy keys within the header's bound; the header's formulas.  No GPU needed."""
import random
import re

import pytest

from prime_cbs_model import G, bsk, cbs_workspace_bytes, flatten, fpksk, lwe_encrypt, lwe_phase, model_circuit_bootstrap
from prime_cmux_model import model_tree, phase
from prime_manylut_model import (HEADER, bit_serial_ms_coarse, cbs_manylut_workspace_bytes, cbs_table, interleave,
                                 model_bootstrap_manylut, model_circuit_bootstrap_manylut, model_extract_many, model_modswitch_coarse,
                                 model_u_manylut, ms_coarse)
from test_gpu_prime_pbs import ALL
from test_prime_pbs_model import PM64, model_extract, model_modswitch, ms, source, wbits


def switch_words(p, logn, t):
    """0, 1, p - 1, (p +- 1) / 2 and floor(j p / 2n') +- 1 for every j: both sides of every boundary of the coarse grid and of its steps"""
    two_np = 2 << (logn - t)
    words = {0, 1, p - 1, (p - 1) // 2, (p + 1) // 2}
    for j in range(two_np + 1):
        c = j * p // two_np
        words |= {w for w in (c - 1, c, c + 1) if 0 <= w < p}
    return sorted(words)


@pytest.mark.parametrize("p", ALL)
def test_coarse_modswitch_is_the_switch_of_the_smaller_ring_shifted(p):
    assert len(ALL) == 13
    tb = 64 if wbits(p) > 32 else 32
    for logn in (4, 5):
        for t in range(logn + 1):
            for x in switch_words(p, logn, t):
                want = ms(x, p, logn - t) << t if t < logn else (((2 * x * 2 + p) // (2 * p)) % 2) << t
                got = ms_coarse(x, p, logn, t)
                assert got == want and got % (1 << t) == 0 and got < (2 << logn), (p, logn, t, x)
                assert bit_serial_ms_coarse(x, p, logn, t, tb) == got, (p, logn, t, x)
                if t == 0:
                    assert got == ms(x, p, logn)
    # the layout: transposed, the body row negated mod 2n and still on the coarse grid; t = 0 is the model of cntt_prime_pbs.h
    rng = random.Random(p)
    L, batch, logn = 3, 2, 4
    lwe = [rng.randrange(p) for _ in range(batch * (L + 1))]
    assert model_modswitch_coarse(lwe, L, batch, p, logn, 0) == model_modswitch(lwe, L, batch, p, logn)
    rot = model_modswitch_coarse(lwe, L, batch, p, logn, 2)
    assert all(r % 4 == 0 and r < 32 for r in rot)
    assert rot[L * batch + 1] == (32 - ms_coarse(lwe[1 * (L + 1) + L], p, logn, 2)) % 32


@pytest.mark.parametrize("n", [16, 32])
def test_interleaved_table_and_many_index_extraction(n):
    """for every a = 0 mod 2^t in Z_2n and every h < 2^t, coefficient h of X^(-a) v is f_h(a / 2^t) for a < n and -f_h(a / 2^t - n') beyond"""
    p = 12289
    rng = random.Random(n)
    for t in range(4):
        nprime = n >> t
        fs = [[rng.randrange(p) for _ in range(nprime)] for _ in range(1 << t)]
        v = interleave(fs, n, t)
        for a in range(0, 2 * n, 1 << t):
            rotated = source(v, (2 * n - a) % (2 * n), p, "rotate")          # X^(-a) v
            m = a >> t
            for h in range(1 << t):
                want = fs[h][m] if a < n else (-fs[h][m - nprime]) % p
                assert rotated[h] == want, (n, t, a, h)
        # the extraction of `count` indices is `count` single extractions, row after row
        k = 2
        glwe = [[rng.randrange(p) for _ in range(n)] for _ in range(k + 1)]
        for count in (1, 2, 7, 8, 9, n):
            got = model_extract_many(glwe, count, p)
            assert len(got) == count * (k * n + 1)
            for h in range(count):
                assert got[h * (k * n + 1):(h + 1) * (k * n + 1)] == model_extract(glwe, h, p), (n, count, h)


def noise_free_keys(rng, p, n, k, s_lwe, pbs, ks):
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    return S, bsk(rng, p, s_lwe, S, n, *pbs), fpksk(rng, p, S, n, *ks)


@pytest.mark.parametrize("Lc", [3, 4])
def test_one_rotation_circuit_bootstrap_is_exact_and_drives_the_tree(Lc):
    """n = 16, L = 3, k = 1, t = 2, PM64 with the PBS gadget (16, 4) = W and the selector gadget (64 / 4, Lc): every u[b][l] has the
    phase exactly 0 / G_l, and the selectors of three bits drive the model tree to every entry at M = 8.  The keyswitch gadget (16, 4)
    fills W, so the selector rows are exact and the tree's only error is the rounding of its own decomposition, s = W - 16 Lc bits: at
    most (1 + k n) 2^(s - 1) per CMux (tests/test_prime_pbs_model.py), three stages; nothing at Lc = 4.  Two of the three LWE key bits
    are set, so three switched words enter the exponent: it is off by less than 1.5 coarse steps, inside the margin n / 2^(t + 1) = 2."""
    p, n, L, k, t = PM64, 16, 3, 1, 2
    pbs, ks, cbs = (16, 4), (16, 4), (16, Lc)
    rng = random.Random(290 + Lc)
    s_lwe = [1, 0, 1]
    S, B, F = noise_free_keys(rng, p, n, k, s_lwe, pbs, ks)
    s_in = flatten(S)
    sel = {}
    for bit in (0, 1):
        for _ in range(3):
            lwe = lwe_encrypt(rng, p, s_lwe, bit * ((p + 1) // 2), noise=p >> 12)
            us = model_u_manylut(lwe, B, p, L, k, n, *pbs, cbs[0], Lc, t)
            assert len(us) == Lc
            for l, u in enumerate(us, start=1):
                assert len(u) == k * n + 1 and lwe_phase(u, s_in, p) == bit * G(p, cbs[0], l) % p, (bit, l)
        sel[bit] = model_circuit_bootstrap_manylut(lwe, B, F, p, L, k, n, *pbs, *ks, *cbs, t)
    entries = [[rng.randrange(8) for _ in range(n)] for _ in range(8)]
    lut = [[m * (p // 8) for m in row] for row in entries]
    s = wbits(p) - cbs[0] * Lc
    bound = 3 * (1 + k * n) * (1 << (s - 1)) if s else 0
    for a in range(8):
        sels = sel[a & 1] + sel[(a >> 1) & 1] + sel[a >> 2]
        ph = phase(model_tree(lut, sels, p, 8, k, n, *cbs), S, p)
        assert [((16 * x + p) // (2 * p)) % 8 for x in ph] == entries[a], a
        assert all(min((x - y) % p, (y - x) % p) <= bound for x, y in zip(ph, lut[a])), a


def test_t_zero_is_the_circuit_bootstrap_of_cntt_prime_cbs_h():
    p, n, L, k = 12289, 16, 2, 1
    pbs, ks, cbs = (7, 2), (7, 2), (5, 1)
    rng = random.Random(5)
    s_lwe = [1, 1]
    S, B, F = noise_free_keys(rng, p, n, k, s_lwe, pbs, ks)
    lwe = lwe_encrypt(rng, p, s_lwe, (p + 1) // 2, noise=3)
    assert model_circuit_bootstrap_manylut(lwe, B, F, p, L, k, n, *pbs, *ks, *cbs, 0) == \
        model_circuit_bootstrap(lwe, B, F, p, L, k, n, *pbs, *ks, *cbs)
    assert cbs_table(p, k, n, 5, 1, 0)[k] == [(p - (1 << (14 - 5 - 1))) % p] * n


# -- the shape of the GPU test's decoding case, run on the model alone (tests/test_gpu_prime_manylut.py imports these) -----------------------
MANY = dict(p=PM64, n=128, k=1, L=2, pbs=(32, 2), t=2, key_noise=15, in_noise=1 << 20)


def many_f(h, m):
    """function h of a 3-bit message"""
    return (m * (2 * h + 1) + h) & 7


def many_enc(m, p):
    return (2 * m * p + 16) // 32             # round(m p / 16): 3 bits under one padding bit


def many_table(p, k, n, t):
    """function h at the coefficients c 2^t + h: boxes of n' / 8 coarse steps per message, shifted by half a box"""
    nprime = n >> t
    half = nprime // 16
    fs = []
    for h in range(1 << t):
        f = []
        for c in range(nprime):
            s = c + half
            v = many_enc(many_f(h, (s % nprime) // (nprime // 8)), p)
            f.append(v if s < nprime else (-v) % p)
        fs.append(f)
    return [[0] * n for _ in range(k)] + [interleave(fs, n, t)]


def many_bound(n, k, L, pbs):
    """cntt_prime_manylut.h: L (k + 1) n pbs_levels 2^(pbs_base_log - 1) E_k with E_k = 2^4"""
    return L * (k + 1) * n * pbs[1] * (1 << (pbs[0] - 1)) * 16


def test_many_lut_bootstrap_decodes_every_table_under_noisy_keys_on_the_model():
    p, n, k, L, pbs, t = (MANY[x] for x in ("p", "n", "k", "L", "pbs", "t"))
    rng = random.Random(2900)
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    s_lwe = [1] * L                                                   # every switched word enters: the worst drift
    B = bsk(rng, p, s_lwe, S, n, *pbs, noise=MANY["key_noise"])
    lut = many_table(p, k, n, t)
    s_in = flatten(S)
    worst = 0
    assert (L + 1) / 2 + (MANY["in_noise"] + 1) * (2 * (n >> t)) / p <= (n >> t) // 16
    for m in range(8):
        lwe = lwe_encrypt(rng, p, s_lwe, many_enc(m, p), noise=MANY["in_noise"])
        rows = model_bootstrap_manylut(lwe, lut, B, p, L, k, n, *pbs, t, 1 << t)
        for h in range(1 << t):
            ph = lwe_phase(rows[h * (k * n + 1):(h + 1) * (k * n + 1)], s_in, p)
            assert ((32 * ph + p) // (2 * p)) % 16 == many_f(h, m), (m, h)
            err = (ph - many_enc(many_f(h, m), p)) % p
            worst = max(worst, min(err, p - err))
    assert worst < many_bound(n, k, L, pbs) == 1 << 45


def test_header_formulas_are_the_models():
    flat = re.sub(r"[\s*]+", " ", open(HEADER).read())
    for text in ("ms_t(x) = 2^t (floor((2 x 2n' + p) / (2 p)) mod 2n')", "ms_0 = ms, word for word", "v[m 2^t + h]",
                 "up((L + 1) batch 4) + up((k + 1) n wb) + up(batch (k + 1) pbs_levels n wb) + up(batch (k + 1) n wb) + up(E R 4) + up(S (k + 1) E (k + 1) n wb)",
                 "v[m 2^t + h] = p - H_(h+1) for h < Lc, 0 for Lc <= h < 2^t", "Lc <= 2^t <= n / 2", "batch (k + 1) pbs_levels >= 2^32",
                 "n / 2^(t + 1) steps of the coarse switch", "L (k + 1) n pbs_levels 2^(pbs_base_log - 1) E_k",
                 "profiles/r29_prime_manylut.txt"):
        assert text in flat, text
    # one rotation: everything but the keyswitch half is per input bit
    assert cbs_manylut_workspace_bytes(32, 8, 3, 1, 2, 3, 2, 3) == 256 + 512 + 3072 + 1536 + 2560 + 12288
    assert cbs_manylut_workspace_bytes(32, 8, 3, 1, 2, 3, 1, 3) == cbs_workspace_bytes(32, 8, 3, 1, 2, 3, 1, 3) - 1536 + 512
