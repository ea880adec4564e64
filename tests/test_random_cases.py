"""The case generators of tests/random_cases.py, checked without a GPU: every (family, seed) yields a valid case, the first SEEDS seeds
of every family -- the ones tests/test_gpu_random_fhe.py runs -- reach the corners listed here (a condition on the committed SEEDS and
draw probabilities, asserted line by line), and the integer models the sweep compares with satisfy their own identities on the drawn
cases.  Also here: the rule that decides for which primes the big-integer product model applies, against the EXACT list of
tests/test_gpu_prime_pbs.py."""
import random

import numpy as np
import pytest

import random_cases as rc
import test_gpu_native_external_product as tex
import test_gpu_native_gadget as tg
import test_gpu_native_keyswitch as tks
import test_gpu_native_pack as tpk
import test_gpu_prime_pbs as tpp
import test_native_keyswitch_abi as ksabi
import test_prime_pbs_model as pm


@pytest.fixture(scope="module")
def cases(oracle):
    return {f: [rc.case(f, s) for s in range(rc.SEEDS)] for f in rc.FAMILIES}


def some(cs, cond):
    return any(cond(c) for c in cs)


def test_seeds_constant_is_in_range():
    assert 16 <= rc.SEEDS <= 32


def test_generators_are_pure_and_never_yield_no_case(cases):
    for f in rc.FAMILIES:
        for s, c in enumerate(cases[f]):
            assert isinstance(c, dict) and c["family"] == f and c["seed"] == s
            assert rc.case(f, s) == c                                   # the same dict again: nothing but (family, seed) enters
    state = random.getstate()
    rc.case("keyswitch", 5)
    assert random.getstate() == state                                   # the global generator is not touched
    for f in rc.FAMILIES:                                               # beyond the suite's seeds, where the soak tool runs
        for s in range(rc.SEEDS, rc.SEEDS + (40 if f != "primepbs" else 12)):
            validate(rc.case(f, s))


def test_max_terms_restatement_equals_the_library():
    for kind, cls in tex.KINDS.items():
        for n in rc.FUSED_N + rc.BIG_N:
            plan = cls.try_new(n)
            assert plan is not None and plan.max_terms() == rc.max_terms(kind, n), (kind, n)
            assert 8 * plan.WORD == rc.wbits(kind) and bool(plan.BINARY) == rc.is_binary(kind)
    assert rc.KINDS == sorted(tex.KINDS, key=rc.KINDS.index) and set(rc.FUSED_KINDS) == set(tg.FUSED) and rc.FUSED_N == tex.FUSED_N
    assert rc.PACK_TERMS == tpk.PACK_TERMS and rc.PACK_TI == tpk.TI and rc.KS_TILE_B == tks.TILE_B and rc.KS_ROWS == tks.ROWS


# -- validity --------------------------------------------------------------------------------------------------------------------------------
def validate(c):
    f = c["family"]
    if f == "ext":
        assert c["kind"] in rc.KINDS and c["n"] in rc.FUSED_N + rc.BIG_N
        assert 1 <= c["nterms"] <= min(9, rc.max_terms(c["kind"], c["n"])) and 1 <= c["nout"] <= 5 and c["batch"] >= 1
        assert c["n"] <= 4096 or c["batch"] == 1
    elif f == "gadget":
        w = rc.wbits(c["kind"])
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= w
        assert c["npolys"] * c["levels"] <= rc.max_terms(c["kind"], c["n"])
        assert 1 <= c["npolys"] <= 4 and 1 <= c["nout"] <= 4 and c["mode"] in rc.MODES
        assert not c["fused"] or c["base_log"] <= 31
        assert len(c["rot"]) == c["batch"] >= 1 and all(0 <= a < 2 * c["n"] for a in c["rot"])
    elif f == "nativepbs":
        assert c["w"] in (32, 64, 128) and c["n"] in (32, 64, 256, 1024) and 1 <= c["k"] <= 3 and 0 <= c["L"] <= 6 and 1 <= c["batch"] <= 40
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= c["w"]
        assert (c["k"] + 1) * c["levels"] <= rc.max_terms(c["kind"], c["n"]) and 0 <= c["index"] < c["n"]
    elif f == "keyswitch":
        w = c["w"]
        assert 1 <= c["base_log"] <= 31 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= w and c["levels"] <= rc.KS_ROWS
        kc = rc.KS_ROWS // c["levels"]
        assert 0 <= c["lin"] <= 4 * kc and 0 <= c["lout"] <= 2 * 128 + 49 and 0 <= c["pad"] <= 7
        assert 1 <= c["batch"] <= 2 * rc.KS_TILE_B[w] + 3
        assert c["batch"] * c["lin"] * c["levels"] * (c["lout"] + 1) <= rc.KEYSWITCH_CAP
    elif f == "pack":
        w, n = c["w"], c["n"]
        assert n in (32, 64, 128, 256, 512, 1024) and 1 <= c["k"] <= 2 and 1 <= c["m"] <= n and 1 <= c["batch"] <= 3 and c["lin"] >= 0
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= w and c["levels"] <= rc.max_terms(c["kind"], n)
        assert c["C"] == max(1, min(rc.max_terms(c["kind"], n), rc.PACK_TERMS) // c["levels"])
        assert c["batch"] * c["m"] * c["lin"] * c["levels"] * (c["k"] + 1) * n <= rc.PACK_CAP[w]
    else:
        p, n, W = c["p"], c["n"], c["W"]
        assert p % (2 * n) == 1 and p > 2 * n and W == p.bit_length() <= c["bits"] and all(p % q for q in range(3, 2000, 2) if q < p)
        assert pow(3, p - 1, p) == 1 and pow(2, p - 1, p) == 1                         # a Fermat check on top of the oracle's search
        assert n in ({64: 16, 32: 32}[c["bits"]], 64, 1024)
        assert c["base_log"] >= 1 and c["levels"] >= 1 and c["base_log"] * c["levels"] <= W
        assert 1 <= c["k"] <= 4 and 0 <= c["L"] <= 5 and 1 <= c["batch"] <= 40 and 0 <= c["index"] < n and 1 <= c["npolys"] <= 3


def test_every_case_is_valid(cases):
    for f in rc.FAMILIES:
        assert len(cases[f]) == rc.SEEDS
        for c in cases[f]:
            validate(c)


# -- the corners the first SEEDS seeds must reach -------------------------------------------------------------------------------------------
def test_keyswitch_corners(cases):
    cs = cases["keyswitch"]
    kc = lambda c: rc.KS_ROWS // c["levels"]
    for w in (32, 64, 128):
        assert some(cs, lambda c: c["w"] == w and 128 % c["levels"] and c["lin"] > kc(c) and c["lin"] % kc(c)), w
    assert some(cs, lambda c: kc(c) == 1 and c["lin"] >= 2)
    assert some(cs, lambda c: c["lin"] == 0) and some(cs, lambda c: c["lout"] == 0)
    assert some(cs, lambda c: c["base_log"] == 31)
    assert some(cs, lambda c: c["base_log"] * c["levels"] == c["w"])
    assert some(cs, lambda c: c["batch"] > rc.KS_TILE_B[c["w"]] and c["lin"] > 0)
    assert some(cs, lambda c: c["lout"] + 1 > 128 and c["lin"] > 0)
    assert sum(c["levels"] > 16 for c in cs) >= rc.SEEDS // 4 - 1
    assert some(cs, lambda c: c["w"] == 128 and c["levels"] >= 64)
    assert some(cs, lambda c: c["pad"] > 0 and c["lin"] > 0)


def test_pack_corners(cases):
    cs = cases["pack"]
    for w in (32, 64, 128):
        ws = [c for c in cs if c["w"] == w]
        assert some(ws, lambda c: c["m"] == c["n"] and c["lin"] > 0), w
        assert some(ws, lambda c: c["m"] < 64 and c["lin"] > 0), w
        assert some(ws, lambda c: c["m"] % 64 and c["m"] > 64), w
        assert some(ws, lambda c: c["lin"] > c["C"]), w
        assert some(ws, lambda c: c["base_log"] > 31 and c["lin"] > 0), w
        assert some(ws, lambda c: abs(c["lin"] - rc.PACK_TI[w]) <= 2), w
        assert some(ws, lambda c: c["n"] >= 256 and c["lin"] > 0) and some(ws, lambda c: c["m"] > 128 and c["lin"] > 0), w
    assert some(cs, lambda c: c["workspace"]) and some(cs, lambda c: not c["workspace"])


def prime_class(c):
    """the classes of the issue, told from the prime's value and the word type alone"""
    p, bits, out = c["p"], c["bits"], set()
    if bits == 64:
        if p >= (1 << 64) - (1 << 32):
            out.add("solinas")
        elif p >= 1 << 63:
            out.add("montgomery")
        elif p >= 1 << 62:
            out.add("strict")
        elif p < 1 << 50:
            out.add("fp50")
        elif p < 1 << 51:
            out.add("fp51")
        else:
            out.add("lazy")
    else:
        out.add("top" if p >= 1 << 31 else "strict" if p >= 1 << 30 else "lazy")
    if "lazy" in out and rc.above_pow2(p):
        out.add("above_pow2")
    return out


def test_primepbs_corners(cases):
    cs = cases["primepbs"]
    for name, bits, lo, end, fallback in rc.PRIME_CLASSES:
        assert fallback % 2048 == 1 and lo <= fallback < end and name in prime_class({"p": fallback, "bits": bits}), (name, bits)
        assert some(cs, lambda c: c["bits"] == bits and c["cls"] == name and name in prime_class(c)), (name, bits)
    assert len({c["W"] for c in cs}) >= 8
    assert some(cs, lambda c: c["W"] == 64 and (c["base_log"], c["levels"]) == (16, 4))
    assert some(cs, lambda c: (c["base_log"], c["levels"]) == (c["W"], 1))
    assert some(cs, lambda c: c["base_log"] * c["levels"] == c["W"] and c["levels"] > 1)
    assert some(cs, lambda c: c["k"] + 1 == 5 and c["L"] > 0)
    assert some(cs, lambda c: c["levels"] > 8 and c["L"] > 0)
    assert {c["n"] for c in cs} == {16, 32, 64, 1024} and {c["bits"] for c in cs} == {32, 64}
    assert some(cs, lambda c: c["batch"] == 33) and some(cs, lambda c: c["L"] == 0)


def test_ext_and_gadget_corners(cases):
    for f in ("ext", "gadget"):
        cs = cases[f]
        assert {c["kind"] for c in cs} == set(rc.KINDS), f
        assert {c["n"] for c in cs} >= set(rc.FUSED_N), f
        assert some(cs, lambda c: c["n"] > 4096), f
    assert some(cases["ext"], lambda c: c["nout"] == 5) and {c["switch"] for c in cases["ext"]} == {0, 1}
    assert {c["accumulate"] for c in cases["ext"]} == {False, True} and some(cases["ext"], lambda c: c["nterms"] == 9)
    g = cases["gadget"]
    assert {c["mode"] for c in g} == set(rc.MODES) and {c["fused"] for c in g} == {False, True}
    assert {(c["kind"]) for c in g if c["fused"]} == set(rc.FUSED_KINDS)
    assert sum(c["base_log"] * c["levels"] == rc.wbits(c["kind"]) for c in g) >= rc.SEEDS // 4
    assert some(g, lambda c: c["levels"] > 8) and all(c["npolys"] * c["levels"] * c["nout"] * c["n"] <= max(rc.WIDE_KEY_WORDS, 8 * 16 * c["n"]) for c in g)
    fixed = lambda c: {0, 1, c["n"] - 1, c["n"], c["n"] + 1, 2 * c["n"] - 1}
    assert some(g, lambda c: set(c["rot"]) & fixed(c)) and some(g, lambda c: set(c["rot"]) - fixed(c))


def test_nativepbs_corners(cases):
    cs = cases["nativepbs"]
    assert {(c["w"], c["n"]) for c in cs} == {(w, n) for w in (32, 64, 128) for n in (32, 64, 256, 1024)}
    assert {c["k"] for c in cs} == {1, 2, 3} and some(cs, lambda c: c["L"] == 0) and some(cs, lambda c: c["L"] == 6)
    assert some(cs, lambda c: c["batch"] == 33) and {c["per_element"] for c in cs} == {False, True} == {c["workspace"] for c in cs}
    assert some(cs, lambda c: c["n"] == 1024 and c["batch"] > 32 and c["L"] > 0) and some(cs, lambda c: c["levels"] > 4 and c["L"] > 0)


# -- the models against their own identities, on the drawn cases ---------------------------------------------------------------------------
def test_digits_reconstruct_the_rounded_word(cases):
    """native digits: sum d_l B^(levels - l) = the rounded word mod B^levels; prime digits: the integer identity of the header"""
    for f in ("gadget", "nativepbs", "keyswitch", "pack"):
        for c in cases[f]:
            w = c["w"] if "w" in c else rc.wbits(c["kind"])
            beta, ell = c["base_log"], c["levels"]
            rng = random.Random(c["data_seed"])
            for x in rc.special_words(rng, w, 12) + tg.sample_words(np.random.default_rng(c["seed"]), w, beta, ell, 12):
                ds = tg.digits(x, w, beta, ell)
                assert ds == tks.digits(x, w, beta, ell) == tpk.digits(x, w, beta, ell)
                assert all(-(1 << beta) // 2 <= d < (1 << beta) // 2 for d in ds)
                assert sum(d << (beta * (ell - 1 - j)) for j, d in enumerate(ds)) % (1 << (beta * ell)) == ksabi.rounded(x, w, beta, ell), c
    for c in cases["primepbs"]:
        p, W, beta, ell = c["p"], c["W"], c["base_log"], c["levels"]
        s = W - beta * ell
        rng = random.Random(c["data_seed"])
        for x in pm.edge_words(p, beta, ell) + [rng.randrange(p) for _ in range(12)]:
            d = pm.signed_digits(x, p, beta, ell)
            xp = pm.lift(x, p)
            assert sum(v << (W - beta * (l + 1)) for l, v in enumerate(d)) == (((xp + (1 << (s - 1))) >> s) << s if s else xp), c
            assert pm.kernel_form_digits(x, p, beta, ell, c["bits"]) == pm.digits(x, p, beta, ell), c


def test_keyswitch_model_equals_the_literal_triple_loop(cases):
    ran = 0
    for c in cases["keyswitch"] + [rc.case("keyswitch", s) for s in range(rc.SEEDS, rc.SEEDS + 40)]:
        w, beta, ell, lin, lout, batch = c["w"], c["base_log"], c["levels"], c["lin"], c["lout"], c["batch"]
        if batch * lin * ell * (lout + 1) >= 10 ** 4:
            batch = max(1, 10 ** 4 // max(1, lin * ell * (lout + 1)))
            if batch * lin * ell * (lout + 1) >= 10 ** 4:
                continue
        rng = random.Random(c["data_seed"])
        stride = lout + 1 + c["pad"]
        lwe = rc.special_words(rng, w, batch * (lin + 1))
        ksk = [rng.getrandbits(w) for _ in range(tks.key_len(lin, ell, lout, stride))]
        want = [x for b in range(batch) for x in ksabi.model_keyswitch(lwe[b * (lin + 1):(b + 1) * (lin + 1)], ksk, lin, lout, stride, w, beta, ell)]
        assert tks.model_keyswitch_batch(lwe, ksk, lin, lout, stride, w, beta, ell, batch) == want, c
        ran += 1
    assert ran >= 8


def test_pack_wrapping_model_equals_the_integer_model(cases):
    """w = 32 / 64: the sweep uses the model on wrapping numpy words; the same function on Python ints says the same on the small cases"""
    ran = 0
    for c in cases["pack"]:
        w, n, k, m, lin, beta, ell = c["w"], c["n"], c["k"], c["m"], c["lin"], c["base_log"], c["levels"]
        if w == 128 or m * lin * ell * (k + 1) * n > 10 ** 6:
            continue
        rng = random.Random(c["data_seed"])
        lwe = rc.special_words(rng, w, m * (lin + 1))
        key = [rng.getrandbits(w) for _ in range(lin * ell * (k + 1) * n)]
        fast = tpk.model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1, dtype={32: np.uint32, 64: np.uint64}[w])
        assert fast == tpk.model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1), c
        ran += 1
    assert ran >= 4


# -- for which primes the big-integer product model applies -----------------------------------------------------------------------------------
def test_exact_list_of_the_prime_bootstrap_tests_follows_the_probe(oracle):
    assert tpp.EXACT == [p for p in tpp.ALL if rc.model_applies(oracle, p, 64 if p >= 1 << 32 else 32)]
    assert pm.P62 in tpp.EXACT and len(tpp.ALL) == 13 and tpp.PW63 not in tpp.EXACT and tpp.PW31 not in tpp.EXACT
    for p in tpp.ALL:
        assert p % 8192 == 1 and tpp.max_logn(p) >= 12, p          # n = 4096: the largest size the decomposition and rotation tests use
