"""The corners the 32 seeds of tests/random_prime_multibit_cases.py reach, asserted on the generator alone: no GPU, no library."""
from random_prime_multibit_cases import CAP, MIN_N, SEEDS, case_primemultibit, rot_of, wraps

CASES = [case_primemultibit(s) for s in range(SEEDS)]


def test_cases_are_valid_and_reproducible():
    assert SEEDS == 32 and CASES == [case_primemultibit(s) for s in range(SEEDS)]
    for c in CASES:
        W = c["p"].bit_length()
        assert c["bits"] in (32, 64) and W <= c["bits"] and (c["p"] - 1) % (2 * c["n"]) == 0 and c["n"] >= MIN_N[c["bits"]], c
        assert 1 <= c["g"] <= 4 and c["lwe_dim"] == c["groups"] * c["g"] and c["lwe_dim"] % c["g"] == 0, c
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W, c
        assert c["batch"] * c["groups"] * (1 << c["g"]) * (c["k"] + 1) ** 2 * c["levels"] * c["n"] <= CAP or c["levels"] == 1, c
        rot = rot_of(c)
        assert len(rot) == (c["lwe_dim"] + 1) * c["batch"] and all(0 <= a < 2 * c["n"] for a in rot), c


def test_the_seeds_reach_the_corners():
    for bits in (32, 64):
        mine = [c for c in CASES if c["bits"] == bits]
        assert {c["g"] for c in mine} == {1, 2, 3, 4}, bits                                          # every grouping
        assert any(c["base_log"] * c["levels"] == c["p"].bit_length() for c in mine), bits           # no rounding: s = 0
        assert any(c["p"].bit_length() == bits - 1 for c in mine), bits                              # the strict range
        assert any(c["k"] + 1 > 4 for c in mine), bits                                               # nout past four
        assert any(wraps(c) for c in mine), bits                                                     # a subset sum that wraps 2n
        assert any(c["n"] == MIN_N[bits] for c in mine), bits
        assert len({c["p"].bit_length() for c in mine}) >= 6, bits                                   # primes of many bit lengths
        assert any(c["p"].bit_length() == bits for c in mine), bits
        assert {c["per_element"] for c in mine} == {False, True} and {c["workspace"] for c in mine} == {False, True}, bits
    assert any(c["n"] == 16 for c in CASES)                                                          # 64-bit words only
    assert any(c["g"] == 4 and c["k"] + 1 > 4 for c in CASES) or any(c["g"] >= 3 and c["k"] + 1 > 4 for c in CASES)
