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
    assert fams == {"prime_ext", "product_ext", "prime_pbs", "prime_kspbs", "prime_pack", "prime_mb", "prime_trace", "prime_ring_pack",
                    "prime_merge", "prime_autoks", "native_ext", "native_dec", "native_pbs", "native_kspbs", "native_pack", "native_mb"}
    # ring packing with a trace after the tree, with the last merge writing the output (m = n) and without a tree (m = 1)
    packs = {r["name"]: r for r in spc.ROWS if r["fam"] == "prime_ring_pack"}
    assert {(r["m"], r["k"], r["ws"], spc.is64(r["p"])) for r in packs.values()} == {(8, 1, False, True), (64, 1, True, False), (1, 2, False, True)}
    assert packs["prime_ring_pack_full"]["m"] == packs["prime_ring_pack_full"]["n"]
    merge, autoks = spc.BY_NAME["prime_merge"], spc.BY_NAME["prime_autoks"]
    assert 0 < merge["shift"] < 2 * merge["n"] and merge["shift"] % 4 and merge["t"] == 2 ** 2 + 1 and not merge["ws"]
    assert autoks["t"] == autoks["n"] + 1 and autoks["k"] == 2 and autoks["p"] == spc.P63 and autoks["ws"]
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


# -- the ring-pack, merge and Galois-keyswitch rows ------------------------------------------------------------------------------------------
PACK_ROWS = ["prime_ring_pack", "prime_ring_pack_full", "prime_ring_pack_single", "prime_merge", "prime_autoks"]
_expected = {}


def expected_words(oracle, name):
    """(shared, sets, words[k][b]) of a row at its small batch: the model's words of every sampled element of every set, computed once"""
    if name not in _expected:
        row = spc.BY_NAME[name]
        batch = row["small"]
        shared, sets = spc.inputs(row, batch)
        words = [{b: spc.want(oracle, row, shared[0], sets[k], b, batch, k) for b in spc.sampled(batch)} for k in range(spc.SETS)]
        _expected[name] = (shared[0], sets, words)
    return _expected[name]


def differing(a, b):
    return int(np.count_nonzero(a != b))


@pytest.mark.parametrize("name", PACK_ROWS)
def test_a_mix_up_of_sets_or_elements_changes_the_expected_words(oracle, name):
    """what keeps the GPU tests from passing vacuously: the four input sets differ pairwise, and so do their expected outputs in every
    sampled element and the sampled elements of one set -- not in a word or two but in more than half the words (the outputs are
    sums of products with random key words, uniform mod p >= 2^30), so one stream's words in the other's output, or one element's in
    another's, cannot go unseen"""
    row = spc.BY_NAME[name]
    _, sets, words = expected_words(oracle, name)
    per = spc.in_out_words(row, row["small"])[1]
    for k in range(spc.SETS):
        for j in range(k):
            assert differing(sets[k]["in"], sets[j]["in"]) > sets[k]["in"].size // 2, (name, k, j)
            for b in spc.sampled(row["small"]):
                assert words[k][b].size == per and differing(words[k][b], words[j][b]) > per // 2, (name, "sets", k, j, "element", b)
        elems = spc.sampled(row["small"])
        for i, b in enumerate(elems):
            for c in elems[:i]:
                assert differing(words[k][b], words[k][c]) > per // 2, (name, "set", k, "elements", b, c)


def test_single_ring_pack_is_the_full_trace_of_the_embedding(oracle):
    """the wiring of the ring-pack model at m = 1: no tree, log2 n trace steps on the embedded ciphertext"""
    from prime_automorphism_model import model_trace
    from prime_ring_pack_model import embed
    row = spc.BY_NAME["prime_ring_pack_single"]
    shared, sets, words = expected_words(oracle, row["name"])
    p, n, k, batch = row["p"], row["n"], row["k"], row["small"]
    lwe = sets[2]["in"].reshape(batch, k * n + 1)
    for b in spc.sampled(batch):
        want = model_trace(embed(lwe[b].tolist(), p, k, n), shared["key"].tolist(), p, n.bit_length() - 1, k, n, row["beta"], row["ell"])
        assert words[2][b].tolist() == want, b


def test_merge_is_one_node_of_the_ring_pack_model(oracle):
    """the wiring of the merge row (glwe_even of the whole batch, then glwe_odd; the order of shift and t): with the embeddings of two LWE
    rows as E and O, shift = n / 2, t = 3 and the last trace key, want() is stage 1 of the ring-pack model at m = 2, whose remaining
    log2 n - 1 trace steps then give model_ring_pack"""
    from prime_automorphism_model import model_trace
    from prime_ring_pack_model import embed, model_ring_pack, stage_params
    base = spc.BY_NAME["prime_merge"]
    p, n, k, beta, ell, batch = base["p"], base["n"], base["k"], base["beta"], base["ell"], 2
    logn = n.bit_length() - 1
    (h, shift, t, r), = stage_params(n, 2)
    assert (h, shift, t, r) == (1, n // 2, 3, logn - 1)
    row = dict(base, shift=shift, t=t)
    rng = np.random.default_rng(spc.seed("one-node"))
    per = k * ell * (k + 1) * n
    keys = rng.integers(0, p, size=logn * per, dtype=np.uint64).astype(spc.pdt(p))
    lwe = rng.integers(0, p, size=(batch, 2, k * n + 1), dtype=np.uint64).astype(spc.pdt(p))
    emb = np.array([[embed(lwe[b, j].tolist(), p, k, n) for b in range(batch)] for j in range(2)], dtype=spc.pdt(p))    # even, then odd
    one_set, shared = {"in": emb.reshape(-1)}, {"key": keys[r * per:(r + 1) * per]}
    assert one_set["in"].size == spc.in_out_words(row, batch)[0]
    for b in range(batch):
        node = spc.want(oracle, row, shared, one_set, b, batch).tolist()
        packed = model_ring_pack([lwe[b, 0].tolist(), lwe[b, 1].tolist()], keys.tolist(), p, 2, k, n, beta, ell)
        assert model_trace(node, keys.tolist(), p, logn - 1, k, n, beta, ell) == packed, b


@pytest.mark.parametrize("name", PACK_ROWS)
def test_large_batch_walks_the_widest_grid_more_than_twice(name):
    """per_wg against the exported grid rules: at 256 CUs the widest kernel of the row has more than twice the workgroups the rule
    grants and the last round is ragged; per_wg is the smallest count that does it, ceil(cap / (CUs * polynomials per element))"""
    import concrete_ntt_amd as cntt
    row = spc.BY_NAME[name]
    L = cntt.lib()
    logn, word = row["n"].bit_length() - 1, 8 if spc.is64(row["p"]) else 4
    rules = {"prime_ring_pack": [L.cntt_prime_ring_pack_grid],
             "prime_merge": [L.cntt_prime_ring_pack_grid, L.cntt_prime_automorphism_grid],          # the kernel's own rule, and the one asked for
             "prime_autoks": [L.cntt_prime_automorphism_grid]}[row["fam"]]
    if row["fam"] == "prime_ring_pack" and row["m"] == 1:
        rules.append(L.cntt_prime_automorphism_grid)                                               # the keyswitches of the trace
    each = spc.widest_polys(row)
    assert each == {"prime_ring_pack": 8, "prime_ring_pack_full": 64, "prime_ring_pack_single": 3, "prime_merge": 2, "prime_autoks": 3}[name]
    polys = spc.batch_of(row, "large", NCU) * each
    for rule in rules:
        cap = rule(1 << 40, logn, word)
        assert cap == 8 * NCU and rule(polys, logn, word) == cap
        assert polys > 2 * cap and polys % cap, (name, polys, cap)
        assert row["per_wg"] == -(-cap // (NCU * each)), (name, row["per_wg"])
    # the small batch stays a handful of elements
    assert 3 <= row["small"] <= 5
    # and the operands of the large batch stay below 256 MiB: four input sets, REPS * SETS + SETS outputs, five caller workspaces
    batch = spc.batch_of(row, "large", NCU)
    win, wout = spc.in_out_words(row, batch)
    ws = 0
    if row["ws"] and row["fam"] == "prime_ring_pack":
        from prime_ring_pack_model import ring_pack_workspace_bytes
        ws = ring_pack_workspace_bytes(row["n"], word, row["m"], row["k"], row["ell"], batch)
    elif row["ws"]:
        from prime_automorphism_model import autoks_workspace_bytes
        ws = autoks_workspace_bytes(row["n"], word, row["k"], row["ell"], batch)
    assert spc.SETS * win * word + (spc.REPS + 1) * spc.SETS * batch * wout * word + (spc.SETS + 1) * ws < 256 << 20, name


def test_native_workspace_bytes_grow_with_the_batch():
    """the shapes of the regrow and the graph tests: a workspace exists from the first product on and grows with every batch of the
    test's schedule (up to one workgroup per compute unit for the parked tiles)"""
    for kind, n in (("native128_plan32", 16384), ("native64_plan52", 1024)):
        sizes = [spc.native_workspace_bytes(kind, n, NCU, b) for b in (1, 2, 3, 4, 9, 10, 33, 34, 129, 130)]
        assert sizes[0] > 0 and all(x < y for x, y in zip(sizes, sizes[1:])), (kind, sizes)
    assert spc.native_workspace_bytes("native128_plan32", 16384, NCU, 1) == 9 * 16384 * 4
    assert spc.native_workspace_bytes("native128_plan32", 16384, NCU, 10 * NCU) == NCU * 9 * 16384 * 4
    assert spc.native_workspace_bytes("native64_plan52", 1024, NCU, 5) == 2 * 3 * 5 * 1024 * 8
