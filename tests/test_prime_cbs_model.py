"""The plain-int model of include/cntt_prime_cbs.h (tests/prime_cbs_model.py) against the header's statements: with noise-free keys u is
exactly 0 or G_l, every output row has the phase M_q bit G_l within the keyswitch rounding bound, the model's selectors drive the model
tree to every entry; the identity the design rests on -- fwd of a constant is that constant in every slot, and the slot-wise sum equals
the composed public pipeline -- against the CPU oracle; and the header's formulas against the model.  No GPU needed."""
import random
import re

import numpy as np
import pytest

from oracle import pyoracle

from prime_cbs_model import (G, HEADER, cbs_workspace_bytes, fpksk, bsk, grid, lwe_encrypt, lwe_phase, flatten, model_circuit_bootstrap,
                             model_keyswitch_rows, model_u, shape)
from prime_cmux_model import model_tree, phase, selector_polys
from test_prime_pbs_model import P30, P62, PM64, negacyclic, signed_digits, wbits

P61 = 1152921504606830593


def lifted(x, p):
    return x if x <= p // 2 else x - p


def keys(rng, p, n, k, L, pbs, ks):
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    return S, s_lwe, bsk(rng, p, s_lwe, S, n, *pbs), fpksk(rng, p, S, n, *ks)


@pytest.mark.parametrize("p,k,pbs,ks,cbs", [(PM64, 1, (16, 4), (22, 2), (32, 2)), (12289, 2, (7, 2), (4, 3), (7, 2)), (P62, 1, (31, 2), (20, 3), (5, 1))])
def test_noise_free_keys_give_exact_u_and_rows_within_the_rounding_bound(p, k, pbs, ks, cbs):
    """n = 16; PM64 and 12289 with cbs_base_log * Lc = W (H_Lc = (p + 1) / 2); nothing is rounded in the rotation (pbs gadget fills W)"""
    rng = random.Random(p + k)
    n, L, W = 16, 3, wbits(p)
    assert pbs[0] * pbs[1] == W
    S, s_lwe, B, F = keys(rng, p, n, k, L, pbs, ks)
    s_in, lin = flatten(S), k * n
    s = W - ks[0] * ks[1]
    bound = (lin + 1) * (1 << s) // 2
    for bit in (0, 1):
        lwe = lwe_encrypt(rng, p, s_lwe, bit * ((p + 1) // 2), noise=p >> 12)
        for l in range(1, cbs[1] + 1):
            u = model_u(lwe, B, p, L, k, n, *pbs, cbs[0], l)
            assert len(u) == lin + 1 and lwe_phase(u, s_in, p) == bit * G(p, cbs[0], l) % p, (p, bit, l)
            rows = model_keyswitch_rows(u, F, p, k, n, *ks)
            for q in range(k + 1):
                ph = phase(rows[q], S, p)
                Mq = [1] + [0] * (n - 1) if q == k else [(-c) % p for c in S[q]]
                off = [lifted((x - bit * G(p, cbs[0], l) * m) % p, p) for x, m in zip(ph, Mq)]
                # M_q times a constant c with |c| <= (Lin + 1) 2^(s - 1): recover c from M_k = 1, bound the others by n |c|
                assert all(abs(x) <= (bound if q == k else n * bound) for x in off), (p, bit, l, q)
                if q == k:
                    assert all(x == 0 for x in off[1:])


@pytest.mark.parametrize("p,k", [(12289, 1), (12289, 2)])
def test_model_selectors_drive_the_model_tree_to_every_entry(p, k):
    """M = 4 at n = 16: two circuit-bootstrapped bits per address; gadgets that fill W = 14, so nothing is rounded anywhere"""
    rng = random.Random(p * 3 + k)
    n, L, m = 16, 2, 4
    pbs, ks, cbs = (7, 2), (7, 2), (7, 2)
    S, s_lwe, B, F = keys(rng, p, n, k, L, pbs, ks)
    lut = [[rng.randrange(p) for _ in range(n)] for _ in range(m)]
    sel = {bit: model_circuit_bootstrap(lwe_encrypt(rng, p, s_lwe, bit * ((p + 1) // 2), noise=p >> 10), B, F, p, L, k, n, *pbs, *ks, *cbs)
           for bit in (0, 1)}
    assert len(sel[0]) == selector_polys(k, cbs[1]) * n
    for a in range(m):
        sels = sel[a & 1] + sel[a >> 1]
        assert phase(model_tree(lut, sels, p, m, k, n, *cbs), S, p) == lut[a], (p, k, a)


@pytest.mark.parametrize("p,n", [(P62, 16), (PM64, 32), (P61, 16), (P30, 32)])
def test_constant_polynomials_transform_to_constants_and_the_pipeline_collapses(p, n):
    """against the CPU oracle: fwd(c X^0) = c in all n slots, and fwd / mul_accumulate / inv / fwd / normalize of constant digit
    polynomials against K_ntt = n^-1 fwd(K) equals the slot-wise sum of d_i K_ntt[i], word for word"""
    bits = 64 if p >= 1 << 32 else 32
    plan = pyoracle.Plan.try_new(n, p, bits)
    assert plan is not None
    rng = random.Random(p + n)

    def arr(words):
        return np.array(words, dtype=plan.dtype)

    def fwd_const(c):
        buf = arr([c] + [0] * (n - 1))
        plan.fwd(buf)
        return buf

    for c in (0, 1, p - 1, rng.randrange(p)):
        assert fwd_const(c).tolist() == [c] * n
    rows, beta = 5, min(31, wbits(p))
    K_ntt = []
    for _ in range(rows):
        f = arr([rng.randrange(p) for _ in range(n)])
        plan.fwd(f)
        plan.normalize(f)
        K_ntt.append(f)
    d = [signed_digits(rng.randrange(p), p, beta, 1)[0] for _ in range(rows)]
    acc = arr([0] * n)
    for di, kn in zip(d, K_ntt):
        plan.mul_accumulate(acc, fwd_const((-di) % p), kn)                                # the packing keyswitch's negated digits
    plan.inv(acc)
    plan.fwd(acc)
    plan.normalize(acc)
    composed = acc.tolist()
    slotwise = [(-sum(di * int(kn[c]) for di, kn in zip(d, K_ntt))) % p for c in range(n)]
    assert composed == slotwise


def test_header_formulas_are_the_models():
    flat = re.sub(r"[\s*]+", " ", open(HEADER).read())
    for text in ("cols = ceil((k + 1) n / (256 16 / wb))", "tiles = ceil(E / 8)", "S0 = max(1, min(ceil(R / 64), floor(2048 / ((k + 1) cols tiles))))",
                 "rows = ceil(R / S0), S = ceil(R / rows)",
                 "up((L + 1) E 4) + up(E (k + 1) n wb) + up(E (k + 1) pbs_levels n wb) + up(E (k + 1) n wb) + up(E R 4) + up(S (k + 1) E (k + 1) n wb)",
                 "Q4 = floor((p + 2) / 4)", "H_l = G_l 2^-1 mod p", "lwe_dim_in = Lin + 1, lwe_count = 1", "M_q = -S_q for q < k and M_k = 1",
                 "|c| <= (Lin + 1) 2^(s - 1)", "ks_base_log <= 31", "one per item up to 8 per CU of a 256-CU part", "profiles/r24_prime_cbs.txt"):
        assert text in flat, text
    # the slab rule at the headline shape and at its edges
    assert shape(1024, 8, 1, 2049, 4) == (4, 1, 63, 33)        # S0 = min(33, 256) = 33 -> rows 63, 33 slabs
    assert shape(1024, 8, 1, 2049, 128) == (4, 16, 129, 16)    # 16 tiles: S0 = 2048 / 128 = 16
    assert shape(16, 8, 1, 17, 8195) == (1, 1025, 17, 1)       # more work items than the cap: one slab
    assert shape(64, 8, 1, 65, 11) == (1, 2, 33, 2)
    assert cbs_workspace_bytes(32, 8, 3, 1, 2, 3, 2, 3) == 256 + 3072 + 6144 + 3072 + 2560 + 12288
    assert grid(0, 10, 8) == 1 and grid(7, 10, 8) == 7 and grid(2048, 4, 4) == 2048 and grid(5000, 14, 8) == 2048
