"""tests/shared_plan_cases.py on the CPU: the rows reach what the shared-plan tests promise to cover, the inputs are reproducible and
inside each call's contract, and the expected words of every row come out of the models with the output's shape (so a wiring mistake in
the helper shows here and not on the GPU)."""
import numpy as np
import pytest

import shared_plan_cases as spc
from test_prime_pbs_model import model_extract, model_modswitch, source

NCU = 256


def test_rows_cover_the_families_widths_classes_kinds_and_workspace_modes():
    fams = {r["fam"] for r in spc.ROWS}
    assert fams == {"prime_ext", "product_ext", "prime_pbs", "prime_kspbs", "prime_pack", "prime_mb", "prime_trace", "native_ext",
                    "native_dec", "native_pbs", "native_kspbs", "native_pack", "native_mb"}
    primes = {spc.prime_of(r, k) for r in spc.ROWS if "p" in r for k in range(spc.SETS)}
    assert {spc.P62, spc.P30} <= primes and {spc.P63, spc.P31} <= primes             # lazy and strict, both widths
    assert {spc.P50, spc.P32} <= primes and spc.PM64 in primes                       # doubles (both widths) and 2^64 - c
    assert spc.PM64 == 2 ** 64 - 2 ** 32 + 1 and 2 ** 62 <= spc.P63 < 2 ** 63 and 2 ** 30 <= spc.P31 < 2 ** 31 and spc.P50 < 2 ** 50 and spc.P32 > 2 ** 31
    kinds = {r["kind"] for r in spc.ROWS if "kind" in r}
    assert {"native32_plan32", "native64_plan32", "native128_plan32"} <= kinds and any(k.endswith("plan52") for k in kinds)
    assert {r["ws"] for r in spc.ROWS if r["fam"].startswith("prime_") and r["fam"] != "prime_ext"} == {True, False}
    assert {r["ws"] for r in spc.ROWS if r["fam"] in ("native_pbs", "native_kspbs", "native_pack", "native_mb")} == {True, False}
    assert {r["g"] for r in spc.ROWS if r["fam"] == "prime_mb"} == {2, 3}
    # the three variants of the prime external product: fused (nout <= 4), composed (nout = 5), and the 16384 pair
    ext = [r for r in spc.ROWS if r["fam"] == "prime_ext"]
    assert any(r["n"] <= 4096 and r["O"] <= 4 for r in ext) and any(r["O"] == 5 for r in ext)
    pair = [r for r in ext if r["n"] == 16384]
    assert len(pair) == 1 and pair[0]["O"] in (3, 4) and pair[0]["p"] == spc.P62 and pair[0]["p_odd"] == spc.P50
    assert any(r["fam"] == "native_ext" and r["n"] == 16384 for r in spc.ROWS)


def test_shapes_stay_small():
    big = [r["n"] for r in spc.ROWS if r["n"] not in (64, 1024)]
    assert sorted(big) == [4096, 16384, 16384]
    for r in spc.ROWS:
        assert r.get("L", 0) <= 16 and r.get("k", 0) <= 2 and r.get("ell", 0) <= 3, r["name"]
        assert len(spc.sampled(spc.batch_of(r, "small", NCU))) == 3
        assert r["per_wg"] >= 1 and spc.batch_of(r, "large", NCU) == 2 * NCU * r["per_wg"] + 5
        assert (r["name"], "small") in spc.REGIMES and (r["name"], "large") in spc.REGIMES
    assert len({r["name"] for r in spc.ROWS}) == len(spc.ROWS)
    assert spc.sampled(1) == [0] and spc.sampled(2) == [0, 1] and spc.sampled(9) == [0, 1, 8]
    assert spc.product_modulus() < 2 ** 64 and all(q % (2 * 64) == 1 for q in spc.PRODUCT_PRIMES)


@pytest.mark.parametrize("row", spc.ROWS, ids=lambda r: r["name"])
def test_inputs_are_reproducible_independent_and_in_contract(row):
    batch = row["small"]
    shared, sets = spc.inputs(row, batch)
    again_shared, again = spc.inputs(row, batch)
    count = spc.in_out_words(row, batch)[0]
    assert len(sets) == spc.SETS
    for k in range(spc.SETS):
        assert sets[k]["in"].size == count and np.array_equal(sets[k]["in"], again[k]["in"])
        for j in range(k):
            assert not np.array_equal(sets[k]["in"], sets[j]["in"])
        if "p" in row:
            p = spc.prime_of(row, k)
            assert sets[k]["in"].dtype == spc.pdt(p) and int(sets[k]["in"].max()) < p
            assert all(int(a.max()) < p for a in shared[spc.plan_index(k)].values())
        if "rot" in sets[k]:
            assert sets[k]["rot"].size == batch and int(sets[k]["rot"].max()) < 2 * row["n"]
    for name in shared[0]:
        if name != "planes":
            assert np.array_equal(shared[0][name], again_shared[0][name])
    if "p_odd" in row:
        assert shared[0]["key"].dtype == shared[1]["key"].dtype and not np.array_equal(shared[0]["key"], shared[1]["key"])
    else:
        assert shared[0] is shared[1]


@pytest.mark.parametrize("row", spc.ROWS, ids=lambda r: r["name"])
def test_expected_words_have_the_shape_of_the_output(oracle, row):
    batch = row["small"]
    shared, sets = spc.inputs(row, batch)
    per = spc.in_out_words(row, batch)[1]
    for k, b in ((0, 0), (3, batch - 1)):
        w = spc.want(oracle, row, shared[spc.plan_index(k)], sets[k], b, batch, k)
        assert isinstance(w, np.ndarray) and w.size == per and w.dtype == sets[k]["in"].dtype, row["name"]
        assert w.any()
        if "p" in row:
            assert int(w.max()) < spc.prime_of(row, k)
    # two elements of one set differ, and so do the same elements of two sets
    assert not np.array_equal(spc.want(oracle, row, shared[0], sets[0], 0, batch, 0), spc.want(oracle, row, shared[0], sets[1], 0, batch, 1))


def test_bootstrap_without_mask_words_is_the_extracted_rotated_table(oracle):
    """the wiring of the prime bootstrap model: with lwe_dim = 0 it is model_extract(X^(-ms(body)) lut)"""
    row = dict(spc.BY_NAME["prime_bootstrap"], L=0)
    shared = spc.shared_inputs(row)
    lwe = spc.set_inputs(row, 3, 0)
    p, n = row["p"], row["n"]
    for b in range(3):
        rot = model_modswitch([int(lwe["in"][b])], 0, 1, p, 6)
        lut = shared["lut"].tolist()
        acc = [source(lut[q * n:(q + 1) * n], rot[0], p, "rotate") for q in range(2)]
        assert spc.want(oracle, row, shared, lwe, b, 3).tolist() == model_extract(acc, 0, p)


def test_keyswitch_bootstrap_with_a_zero_key_bootstraps_the_body(oracle):
    """the wiring of the combined models: a zero keyswitch key leaves (0, ..., 0, body)"""
    for name in ("prime_ks_bootstrap", "native_ks_bootstrap"):
        row = spc.BY_NAME[name]
        shared = dict(spc.shared_inputs(row))
        shared["ksk"] = np.zeros_like(shared["ksk"])
        s = spc.set_inputs(row, 2, 0)
        big = row["k"] * row["n"]
        plain = dict(row, fam=row["fam"].replace("kspbs", "pbs"))
        body = s["in"].reshape(2, big + 1)[:, big]
        lwe = np.zeros((2, row["L"] + 1), dtype=s["in"].dtype)
        lwe[:, row["L"]] = body
        for b in range(2):
            assert np.array_equal(spc.want(oracle, row, shared, s, b, 2), spc.want(oracle, plain, shared, {"in": lwe.reshape(-1)}, b, 2)), name


def test_native_workspace_bytes_grow_with_the_batch():
    """the shapes of the regrow and the graph tests: a workspace exists from the first product on and grows with every batch of the
    test's schedule (up to one workgroup per compute unit for the parked tiles)"""
    for kind, n in (("native128_plan32", 16384), ("native64_plan52", 1024)):
        sizes = [spc.native_workspace_bytes(kind, n, NCU, b) for b in (1, 2, 3, 4, 9, 10, 33, 34, 129, 130)]
        assert sizes[0] > 0 and all(x < y for x, y in zip(sizes, sizes[1:])), (kind, sizes)
    assert spc.native_workspace_bytes("native128_plan32", 16384, NCU, 1) == 9 * 16384 * 4
    assert spc.native_workspace_bytes("native128_plan32", 16384, NCU, 10 * NCU) == NCU * 9 * 16384 * 4
    assert spc.native_workspace_bytes("native64_plan52", 1024, NCU, 5) == 2 * 3 * 5 * 1024 * 8
