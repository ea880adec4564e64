"""The corners the 32 seeds of tests/random_native_multibit_cases.py reach, asserted on the generator alone: no GPU, no library."""
from random_native_multibit_cases import CAP, KINDS, LAZY, SEEDS, WBITS, case_nativemultibit, rot_of, wraps

CASES = [case_nativemultibit(s) for s in range(SEEDS)]


def test_cases_are_valid_and_reproducible():
    assert SEEDS == 32 and CASES == [case_nativemultibit(s) for s in range(SEEDS)]
    for c in CASES:
        assert c["kind"] in KINDS and c["w"] == WBITS[c["kind"]] and c["n"] in (32, 64), c
        assert 1 <= c["g"] <= 4 and c["lwe_dim"] == c["groups"] * c["g"], c
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= c["w"], c
        assert c["batch"] * c["groups"] * (1 << c["g"]) * (c["k"] + 1) ** 2 * c["levels"] * c["n"] <= CAP, c
        rot = rot_of(c)
        assert len(rot) == (c["lwe_dim"] + 1) * c["batch"] and all(0 <= a < 2 * c["n"] for a in rot), c


def test_the_seeds_reach_the_corners():
    for kind in KINDS:
        mine = [c for c in CASES if c["kind"] == kind]
        assert {c["g"] for c in mine} == {1, 2, 3, 4}, kind                                          # every grouping on every kind
        assert any(c["base_log"] * c["levels"] == c["w"] for c in mine), kind                        # no rounding: s = 0
        assert any(c["levels"] == 1 for c in mine), kind                                             # one wide level
        assert any(c["k"] == 2 for c in mine), kind                                                  # nout = 3
        assert any(c["n"] == 32 for c in mine), kind
    J = {(c["k"] + 1) * c["levels"] for c in CASES}
    assert any(j < LAZY for j in J) and any(j == LAZY for j in J) and any(j > LAZY and j % LAZY for j in J) and any(j >= 2 * LAZY for j in J)
    assert any(wraps(c) for c in CASES if c["g"] >= 2) and {c["n"] for c in CASES} == {32, 64}
    assert {c["per_element"] for c in CASES} == {False, True} and {c["workspace"] for c in CASES} == {False, True}
    assert any(c["batch"] > 1 for c in CASES) and any(c["groups"] > 1 for c in CASES)
