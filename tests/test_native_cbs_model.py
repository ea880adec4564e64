"""The plain-int model of include/cntt_cbs.h (tests/native_cbs_model.py) against the header's statements, for w = 32, 64, 128: with
noise-free keys and gadgets that fill the word the phase of every selector row is exactly M_q * bit * G_l; with a keyswitch gadget that
rounds, the rounding part stays within the header's bound; the keyswitch half equals the public packing recipe on (u, 0); the digits are
those of the native gadget model, both ways of taking them.  No GPU needed."""
import random

import pytest

from native_cbs_model import (G, bsk, flatten, fpksk, lwe_encrypt, lwe_phase, model_keyswitch_rows, model_pack_rows, model_u)
from native_cmux_model import digits, digits_by_offset, negacyclic, phase

N, K, L = 8, 1, 3            # the model needs no transform, so n is free; (L + 1) / 2 < n / 2: the drift of ms() crosses no quadrant
GADGETS = {32: ((8, 4), (8, 4), (5, 2)), 64: ((16, 4), (16, 4), (9, 3)), 128: ((32, 4), (16, 8), (21, 2))}   # pbs, ks (both fill w), cbs


def keys(w, seed, ks=None):
    rng = random.Random(seed)
    pbs, ks_full, cbs = GADGETS[w]
    ks = ks or ks_full
    S = [[rng.randrange(2) for _ in range(N)] for _ in range(K)]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    return rng, S, s_lwe, bsk(rng, w, s_lwe, S, N, *pbs), fpksk(rng, w, S, N, *ks), pbs, ks, cbs


def want_phase(S, q, value, w):
    """the polynomial M_q * value: -S_q * value for q < k, the constant `value` for q = k"""
    M = 1 << w
    return [value % M] + [0] * (N - 1) if q == K else [(-c * value) % M for c in S[q]]


@pytest.mark.parametrize("w", [32, 64, 128])
def test_noise_free_rows_have_exactly_the_phase_of_the_selector_convention(w):
    rng, S, s_lwe, B, F, pbs, ks, cbs = keys(w, 100 + w)
    for bit in (0, 1):
        lwe = lwe_encrypt(rng, w, s_lwe, bit << (w - 1))
        for l in range(1, cbs[1] + 1):
            u = model_u(lwe, B, w, L, K, N, *pbs, cbs[0], l)
            assert lwe_phase(u, flatten(S), w) == bit * G(w, cbs[0], l), (w, bit, l)      # step 2: 0 or G_l
            rows = model_keyswitch_rows(u, F, w, K, N, *ks)
            for q in range(K + 1):
                assert phase(rows[q], S, w) == want_phase(S, q, bit * G(w, cbs[0], l), w), (w, bit, l, q)


@pytest.mark.parametrize("w,ks", [(32, (7, 3)), (64, (11, 2)), (128, (25, 3))])
def test_rounding_part_stays_within_the_bound_of_the_header(w, ks):
    """ks_base_log * Lk < w: phase(row q) - M_q bit G_l = M_q c with ONE integer |c| <= (Lin + 1) 2^(s - 1) for all q"""
    rng, S, s_lwe, B, F, pbs, ks, cbs = keys(w, 200 + w, ks)
    M, s = 1 << w, w - ks[0] * ks[1]
    assert s > 0
    bound = (K * N + 1) << (s - 1)
    seen = 0
    for bit in (0, 1, 0, 1, 0, 1):       # c is a multiple of 2^s made of Lin + 1 roundings: often 0, so several samples
        lwe = lwe_encrypt(rng, w, s_lwe, bit << (w - 1))
        u = model_u(lwe, B, w, L, K, N, *pbs, cbs[0], 1)
        rows = model_keyswitch_rows(u, F, w, K, N, *ks)
        body = phase(rows[K], S, w)
        c = (body[0] - bit * G(w, cbs[0], 1)) % M
        c = c - M if c >= M // 2 else c
        assert abs(c) <= bound and not any(body[1:]), (w, bit, c, bound)
        seen = max(seen, abs(c))
        for q in range(K):
            assert phase(rows[q], S, w) == want_phase(S, q, bit * G(w, cbs[0], 1) + c, w), (w, bit, q)
    assert seen > 0          # the cases do round


@pytest.mark.parametrize("w", [32, 64, 128])
def test_keyswitch_half_equals_the_public_packing_recipe_on_u_and_zero(w):
    """random words: the statement is arithmetic, not cryptography; ks gadgets with and without rounding, Lk = 1 included"""
    rng = random.Random(300 + w)
    M = 1 << w
    for ks in ((min(31, w // 2), 2), (7, 3), (31, 1)):
        R = (K * N + 1) * ks[1]
        u = [rng.randrange(M) for _ in range(K * N + 1)]
        u[0], u[1] = 0, M - 1
        F = [rng.randrange(M) for _ in range((K + 1) * R * (K + 1) * N)]
        assert model_keyswitch_rows(u, F, w, K, N, *ks) == model_pack_rows(u, F, w, K, N, *ks), (w, ks)


@pytest.mark.parametrize("w", [32, 64, 128])
def test_digits_are_those_of_the_native_gadget_model(w):
    rng = random.Random(400 + w)
    M = 1 << w
    for beta, ell in ((31, 1), (31, w // 31), (22, 1), (11, 2), (1, 5), (8, w // 8)):
        s = w - beta * ell
        edge = (M - (1 << (w - 1))) % M                                            # 2^(w - 1): d_1 = -B / 2 with every lower level zero
        for x in [0, 1, M - 1, M // 2, M // 2 - 1, edge] + [rng.randrange(M) for _ in range(200)]:
            d = digits(x, w, beta, ell)
            assert d == digits_by_offset(x, w, beta, ell) and all(-(1 << (beta - 1)) <= v < (1 << (beta - 1)) for v in d)
            r = sum(v << (w - beta * (j + 1)) for j, v in enumerate(d)) % M        # r_i 2^s of the header
            e = (r - x) % M
            assert min(e, M - e) <= ((1 << (s - 1)) if s else 0), (w, beta, ell, x)


def test_scalar_digit_times_polynomial_is_the_negacyclic_product_with_a_constant():
    """why step 3 involves no transform"""
    rng = random.Random(5)
    for w in (32, 64, 128):
        M = 1 << w
        f = [rng.randrange(M) for _ in range(N)]
        for d in (-(1 << 30), -1, 3, (1 << 30) - 1):
            assert negacyclic([d % M] + [0] * (N - 1), f, w) == [(d * x) % M for x in f]
