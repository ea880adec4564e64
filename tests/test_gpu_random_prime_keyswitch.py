"""Seeded random sweep of the prime plans' LWE keyswitch (include/cntt_prime_keyswitch.h): seeds 0 .. 31 of the `primeks` family of
tests/random_prime_keyswitch_cases.py -- random primes of every bit length on both word types, random digits, shapes and strides -- each
bit-exact against the plain-int model of tests/test_prime_keyswitch_abi.py; and, without a GPU, the corners those 32 seeds reach."""
import random

import numpy as np
import pytest

import random_prime_keyswitch_cases as pk
from concrete_ntt_amd import prime32, prime64
from test_prime_keyswitch_abi import KS_ROWS, chunk_words, model_keyswitch
from test_prime_pbs_model import edge_words

CASES = {}


def case(seed):
    if seed not in CASES:
        CASES[seed] = pk.case_primeks(seed)
    return CASES[seed]


def test_generator_is_pure_and_every_case_is_valid():
    assert pk.SEEDS == 32 and (pk.KS_ROWS, pk.chunk_words(3, 5), pk.chunk_words(31, 2)) == (KS_ROWS, chunk_words(3, 5), chunk_words(31, 2))
    random.seed(1)
    for seed in range(pk.SEEDS):
        c = case(seed)
        assert c == pk.case_primeks(seed)                        # no state, no global random numbers
        p, W = c["p"], c["p"].bit_length()
        assert c["bits"] in (32, 64) and W <= c["bits"] and (p - 1) % (2 * pk.PLAN_N[c["bits"]]) == 0
        assert 1 <= c["base_log"] <= 31 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W
        assert chunk_words(c["base_log"], c["levels"]) >= 1
        assert c["lin"] >= 0 and c["lout"] >= 0 and c["batch"] >= 1 and c["pad"] >= 0
        assert c["batch"] * c["lin"] * c["levels"] * (c["lout"] + 1) <= pk.CAP


def test_corners_the_32_seeds_reach():
    cs = [case(s) for s in range(pk.SEEDS)]

    def some(cond, bits=None):
        return any(cond(c) for c in cs if bits in (None, c["bits"]))

    W = lambda c: c["p"].bit_length()
    kc = lambda c: chunk_words(c["base_log"], c["levels"])
    for bits in (32, 64):
        assert some(lambda c: True, bits)
        assert some(lambda c: c["lin"] == 0, bits) and some(lambda c: c["lout"] == 0, bits)
        assert some(lambda c: c["base_log"] >= 30, bits)
        assert some(lambda c: c["base_log"] * c["levels"] == W(c), bits)
        assert some(lambda c: W(c) == bits, bits)                                              # the whole word
        assert some(lambda c: min(KS_ROWS, 1 << (32 - c["base_log"])) % c["levels"] != 0, bits)  # levels that do not divide the chunk rows
        assert some(lambda c: c["lin"] > kc(c) and c["lin"] % kc(c) != 0, bits)                # past one chunk, with a tail
        assert some(lambda c: c["batch"] > pk.TILE_B, bits) and some(lambda c: c["lout"] + 1 > pk.TILE_C, bits)
        assert some(lambda c: c["pad"] > 0 and c["lin"] > 0, bits)
    assert some(lambda c: kc(c) == 1) or some(lambda c: c["levels"] > KS_ROWS // 4)            # few words per chunk
    assert len({W(c) for c in cs}) >= 20                                                       # many bit lengths, from 12 bits up
    assert min(W(c) for c in cs) <= 13 and some(lambda c: 32 < W(c) < 62)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(pk.SEEDS))
def test_random_prime_keyswitch(seed):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    c = case(seed)
    p, bits, beta, ell, lin, lout, batch = c["p"], c["bits"], c["base_log"], c["levels"], c["lin"], c["lout"], c["batch"]
    dtype = np.uint64 if bits == 64 else np.uint32
    plan = (prime64 if bits == 64 else prime32).Plan.try_new(pk.PLAN_N[bits], p)
    assert plan is not None, c
    stride = lout + 1 + c["pad"]
    rng = np.random.default_rng(c["data_seed"])
    lwe = rng.integers(0, p, size=batch * (lin + 1), dtype=np.uint64).astype(dtype)
    for j, e in enumerate(edge_words(p, beta, ell)):             # random canonical words mixed with the digit rule's edges
        if 3 * j < lwe.size:
            lwe[3 * j] = e
    ksk = rng.integers(0, p, size=max(lin * ell * stride - c["pad"], 0), dtype=np.uint64).astype(dtype)
    want = np.array(model_keyswitch(lwe.tolist(), ksk.tolist(), p, lin, lout, stride, beta, ell, batch), dtype=dtype)
    to = lambda a: torch.from_numpy(a.view(np.int64 if bits == 64 else np.int32)).cuda()
    out = to(np.full(batch * (lout + 1), 7, dtype=dtype))
    plan.keyswitch_batch(out, to(lwe), to(ksk), lin, lout, beta, ell, row_stride=stride)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(dtype)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (c, bad[:8], got[bad[:4]], want[bad[:4]])
