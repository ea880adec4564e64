"""The `primeautom` case generator (tests/random_prime_automorphism_cases.py) without a GPU: it is pure, every case is valid and within
the cap on the model's integer products, and seeds 0 .. 31 reach every corner of the automorphism calls on both word types."""
import random

import random_prime_automorphism_cases as pa

CASES = {}


def case(seed):
    if seed not in CASES:
        CASES[seed] = pa.case_primeautom(seed)
    return CASES[seed]


def test_generator_is_pure_and_every_case_is_valid():
    assert pa.SEEDS == 32
    random.seed(1)
    state = random.getstate()
    for seed in range(pa.SEEDS + 16):
        c = case(seed)
        assert c == pa.case_primeautom(seed)                         # no state, no global random numbers
        p, W, n = c["p"], c["p"].bit_length(), c["n"]
        assert c["bits"] in (32, 64) and W <= c["bits"] and n >= pa.MIN_N[c["bits"]] and (p - 1) % (2 * n) == 0
        assert (c["bits"] == 64) == (p >= 1 << 32)                   # the modulus tells the word type
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W
        assert c["t"] % 2 == 1 and 1 <= c["t"] < 2 * n and 0 <= c["steps"] <= n.bit_length() - 1
        assert 0 <= c["k"] <= 4 and 1 <= c["batch"] <= 3
        assert c["batch"] * c["k"] * c["levels"] * (c["k"] + 1) * n * n <= pa.CAP, c
    assert random.getstate() == state


def test_corners_the_32_seeds_reach():
    cs = [case(s) for s in range(pa.SEEDS)]

    def some(cond, bits=None):
        return any(cond(c) for c in cs if bits in (None, c["bits"]))

    W = lambda c: c["p"].bit_length()
    logn = lambda c: c["n"].bit_length() - 1
    for bits in (32, 64):
        assert sum(c["bits"] == bits for c in cs) == 16
        assert some(lambda c: c["t"] == 2 * c["n"] - 1, bits) and some(lambda c: c["t"] == 1, bits)
        assert some(lambda c: c["t"] == c["n"] + 1, bits) and some(lambda c: c["t"] == c["n"] // 2 + 1, bits)
        assert some(lambda c: c["t"] not in (1, c["n"] + 1, c["n"] // 2 + 1, 2 * c["n"] - 1), bits)
        assert some(lambda c: c["steps"] == logn(c), bits) and some(lambda c: c["steps"] == 0, bits)
        assert some(lambda c: 0 < c["steps"] < logn(c), bits)
        assert some(lambda c: c["k"] == 0, bits) and some(lambda c: c["k"] == 4, bits)          # no key at all; five outputs: the composed path
        assert some(lambda c: 1 <= c["k"] <= 3, bits)                                           # the fused chain
        assert some(lambda c: W(c) == bits, bits)                                               # the whole word
        assert some(lambda c: c["base_log"] * c["levels"] == W(c), bits)
        assert some(lambda c: c["base_log"] * c["levels"] < W(c), bits)
        assert some(lambda c: c["levels"] >= 5, bits) and some(lambda c: c["levels"] == 1, bits)
        assert some(lambda c: c["batch"] > 1, bits) and some(lambda c: c["batch"] == 1, bits)
        assert some(lambda c: c["n"] == pa.MIN_N[bits], bits) and some(lambda c: c["n"] == 256, bits)
        assert some(lambda c: c["add_input"], bits) and some(lambda c: not c["add_input"], bits)
        assert some(lambda c: c["workspace"], bits) and some(lambda c: not c["workspace"], bits)
    assert len({W(c) for c in cs}) >= 12                                                        # many bit lengths
    assert some(lambda c: W(c) <= 16) and some(lambda c: 32 < W(c) < 62)
