"""The `primepack` case generator (tests/random_prime_pack_cases.py) without a GPU: it is pure, every case is valid and within the cap
on the model's integer products, seeds 0 .. 31 reach every corner of the packing keyswitch on both word types, and the big-integer
model applies -- by the probe of tests/random_cases.py on the CPU oracle -- to at least three quarters of them."""
import random

import prime_pack_model as ppm
import random_cases as rc
import random_prime_pack_cases as pp

CASES = {}


def case(seed):
    if seed not in CASES:
        CASES[seed] = pp.case_primepack(seed)
    return CASES[seed]


def cost(c):
    return c["batch"] * c["m"] * c["lin"] * c["levels"] * (c["k"] + 1) * c["n"]


def test_generator_is_pure_and_every_case_is_valid():
    assert pp.SEEDS == 32 and (pp.PACK_TERMS, pp.TT, pp.TI) == (ppm.PACK_TERMS, ppm.TT, ppm.TI) and pp.chunk(3) == ppm.C(3)
    random.seed(1)
    state = random.getstate()
    for seed in range(pp.SEEDS + 16):                               # beyond the suite's seeds, where the soak tool runs
        c = case(seed)
        assert c == pp.case_primepack(seed)                         # no state, no global random numbers
        p, W, n = c["p"], c["p"].bit_length(), c["n"]
        assert c["bits"] in (32, 64) and W <= c["bits"] and n >= pp.MIN_N[c["bits"]] and (p - 1) % (2 * n) == 0
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W
        assert 1 <= c["m"] <= n and c["lin"] >= 0 and 1 <= c["batch"] <= 3 and 1 <= c["k"] <= 5
        assert c["m"] * c["lin"] * c["levels"] * (c["k"] + 1) * n <= cost(c) <= pp.CAP, c
    assert random.getstate() == state


def test_corners_the_32_seeds_reach():
    cs = [case(s) for s in range(pp.SEEDS)]

    def some(cond, bits=None):
        return any(cond(c) for c in cs if bits in (None, c["bits"]))

    W = lambda c: c["p"].bit_length()
    C = lambda c: pp.chunk(c["levels"])
    for bits in (32, 64):
        assert sum(c["bits"] == bits for c in cs) == 16
        assert some(lambda c: c["lin"] == 0, bits)
        assert some(lambda c: W(c) == bits, bits)                                              # the whole word
        assert some(lambda c: c["base_log"] * c["levels"] == W(c), bits)
        assert some(lambda c: c["base_log"] * c["levels"] < W(c), bits)
        assert some(lambda c: c["base_log"] >= 30, bits)
        assert some(lambda c: c["levels"] >= 9, bits)                                          # few words per chunk
        assert some(lambda c: c["k"] == 5, bits) and some(lambda c: c["k"] == 4, bits)         # five and six outputs: the composed path
        assert some(lambda c: c["k"] <= 3, bits)                                               # the fused chain
        assert some(lambda c: c["m"] == 1, bits) and some(lambda c: c["m"] == c["n"], bits)
        assert some(lambda c: 1 < c["m"] < c["n"] and c["m"] not in (pp.TT - 1, pp.TT + 1), bits)
        assert some(lambda c: c["m"] == pp.TT - 1, bits) and some(lambda c: c["m"] == pp.TT + 1, bits)
        assert some(lambda c: c["lin"] > C(c) and c["lin"] % C(c) != 0, bits)                  # past one chunk, with a tail
        assert some(lambda c: c["lin"] > 2 * C(c), bits)                                       # three external products
        assert some(lambda c: 0 < c["lin"] < pp.TI, bits) and some(lambda c: c["lin"] > pp.TI, bits)
        assert some(lambda c: c["batch"] > 1, bits) and some(lambda c: c["batch"] == 1, bits)
        assert some(lambda c: c["n"] == pp.MIN_N[bits], bits) and some(lambda c: c["n"] == 256, bits)
        assert some(lambda c: c["workspace"], bits) and some(lambda c: not c["workspace"], bits)
    assert some(lambda c: c["base_log"] > 31, 64)                                              # a digit wider than the keyswitch's 31 bits
    assert len({W(c) for c in cs}) >= 16                                                       # many bit lengths
    assert some(lambda c: W(c) <= 16) and some(lambda c: 32 < W(c) < 62)


def test_big_integer_model_applies_to_three_quarters_of_the_cases(oracle):
    cs = [case(s) for s in range(pp.SEEDS)]
    applies = [rc.model_applies(oracle, c["p"], c["bits"]) for c in cs]
    assert 4 * sum(applies) >= 3 * len(cs), [c["seed"] for c, a in zip(cs, applies) if not a]
