"""The `primeringpack` case generator (tests/random_prime_ring_pack_cases.py) without a GPU: it is pure, every case is valid and within
the cap on the model's integer products, and seeds 0 .. 31 reach every corner of the ring-packing calls on both word types."""
import random

import random_prime_ring_pack_cases as pr

CASES = {}


def case(seed):
    if seed not in CASES:
        CASES[seed] = pr.case_primeringpack(seed)
    return CASES[seed]


def test_generator_is_pure_and_every_case_is_valid():
    assert pr.SEEDS == 32
    random.seed(1)
    state = random.getstate()
    for seed in range(pr.SEEDS + 16):
        c = case(seed)
        assert c == pr.case_primeringpack(seed)                      # no state, no global random numbers
        p, W, n, m = c["p"], c["p"].bit_length(), c["n"], c["lwe_count"]
        assert c["bits"] in (32, 64) and W <= c["bits"] and n >= pr.MIN_N[c["bits"]] and (p - 1) % (2 * n) == 0
        assert (c["bits"] == 64) == (p >= 1 << 32)                   # the modulus tells the word type
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W
        assert c["t"] % 2 == 1 and 1 <= c["t"] < 2 * n and 0 <= c["shift"] < 2 * n
        assert 1 <= m <= n and m & (m - 1) == 0
        assert 0 <= c["k"] <= 4 and 1 <= c["batch"] <= 3
        assert c["batch"] * c["k"] * c["levels"] * (c["k"] + 1) * n * n <= pr.CAP, c
    assert random.getstate() == state


def test_corners_the_32_seeds_reach():
    cs = [case(s) for s in range(pr.SEEDS)]

    def some(cond, bits=None):
        return any(cond(c) for c in cs if bits in (None, c["bits"]))

    W = lambda c: c["p"].bit_length()
    for bits in (32, 64):
        assert sum(c["bits"] == bits for c in cs) == 16
        assert some(lambda c: c["lwe_count"] == 1, bits) and some(lambda c: c["lwe_count"] == c["n"], bits)       # the trace alone; no trace
        assert some(lambda c: c["lwe_count"] == 2, bits) and some(lambda c: 2 < c["lwe_count"] < c["n"], bits)    # one stage; both buffers
        assert some(lambda c: c["shift"] == 0, bits) and some(lambda c: c["shift"] == c["n"], bits)
        assert some(lambda c: c["shift"] == c["n"] - 1, bits) and some(lambda c: c["shift"] == 2 * c["n"] - 1, bits)
        assert some(lambda c: c["shift"] % 4 and c["shift"] not in (c["n"] - 1, 2 * c["n"] - 1), bits)            # an unaligned rotated read
        assert some(lambda c: c["k"] == 0, bits) and some(lambda c: c["k"] == 4, bits)          # no key at all; five outputs: the composed path
        assert some(lambda c: 1 <= c["k"] <= 3, bits)                                           # the fused chain
        assert some(lambda c: W(c) == bits, bits)                                               # the whole word
        assert some(lambda c: c["base_log"] * c["levels"] == W(c), bits)
        assert some(lambda c: c["base_log"] * c["levels"] < W(c), bits)
        assert some(lambda c: c["levels"] >= 5, bits) and some(lambda c: c["levels"] == 1, bits)
        assert some(lambda c: c["batch"] > 1, bits) and some(lambda c: c["batch"] == 1, bits)
        assert some(lambda c: c["n"] == pr.MIN_N[bits], bits) and some(lambda c: c["n"] == 256, bits)
        assert some(lambda c: c["workspace"], bits) and some(lambda c: not c["workspace"], bits)
    assert len({W(c) for c in cs}) >= 12                                                        # many bit lengths
    assert some(lambda c: W(c) <= 20) and some(lambda c: 32 < W(c) < 62)
