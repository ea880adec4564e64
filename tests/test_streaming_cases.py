"""The shape calculator of the streaming tests (tests/streaming_cases.py) without a GPU.  These assertions are the proof of reach of
tests/test_gpu_prime_streaming.py: every full call sits on the first batch at which its launch passes STREAM_BYTES -- one batch element
fewer does not stream -- so it takes the STREAM = true kernels, and no launch of any reference call streams, so the references take the
other form.  Also: a case holds at most MEM_CAP bytes on the device, and the calls' own argument checks accept it."""
import streaming_cases as sc
from test_prime_pbs_model import P30, P62


def streamed(launches):
    return [label for label, nbytes in launches if sc.streams(nbytes)]


def test_constant_and_formulas_are_those_of_the_launch_sites():
    assert sc.STREAM_BYTES == 384 << 20 == 402653184 and sc.MEM_CAP == 4 << 30
    # the factor 2 of automorphism_device; nct, not batch, in the merge; k + 1 polynomials in the set-up
    assert sc.autom_bytes(3, 1024, 8) == 2 * 3 * 1024 * 8
    assert sc.digit_bytes(5, 2, 15, 1024, 4) == 5 * 2 * 15 * 1024 * 4
    assert sc.acc_bytes(7, 1, 1024, 8) == 7 * 2 * 1024 * 8
    assert sc.ring_pack_launches(1024, 8, 4, 1, 15, 3) == [("tree level 1 (leaf)", sc.digit_bytes(6, 1, 15, 1024, 8)),
                                                          ("tree level 2", sc.digit_bytes(3, 1, 15, 1024, 8))] + \
        [("trace step %d" % r, sc.digit_bytes(3, 1, 15, 1024, 8)) for r in range(8)]
    assert sc.first_streaming(8192) * 8192 > sc.STREAM_BYTES >= (sc.first_streaming(8192) - 1) * 8192


def test_the_batches_are_the_ones_the_shapes_give():
    got = {c["name"]: (c["p"], c["n"], c["k"], c["base_log"], c["levels"], c["batch"]) for c in sc.CASES}
    assert got == {"autom-p62-1024": (P62, 1024, 0, 0, 0, 24577), "autom-p30-1024": (P30, 1024, 0, 0, 0, 49153),
                   "autom-p62-16384": (P62, 16384, 0, 0, 0, 1537),
                   "autoks-p62-k1": (P62, 1024, 1, 4, 15, 3277), "autoks-p30-k2": (P30, 1024, 2, 2, 15, 3277),
                   "trace-p62-k1": (P62, 1024, 1, 4, 15, 3277),
                   "merge-p62-k1": (P62, 1024, 1, 4, 15, 3277), "merge-p30-k2": (P30, 1024, 2, 2, 15, 3277),
                   "ringpack-p62-m2": (P62, 1024, 1, 4, 15, 3277), "ringpack-p62-m4": (P62, 1024, 1, 4, 15, 1639),
                   "multibit-setup-p62": (P62, 1024, 1, 7, 3, 24577), "multibit-setup-native64": (None, 1024, 1, 7, 3, 24577)}
    assert len(set(c["name"] for c in sc.CASES)) == len(sc.CASES)
    assert sc.BY_NAME["trace-p62-k1"]["steps"] == 2 and sc.BY_NAME["trace-p62-k1"]["ts"] == [1025, 513]
    assert sc.BY_NAME["ringpack-p62-m2"]["lwe_count"] == 2 and sc.BY_NAME["ringpack-p62-m4"]["lwe_count"] == 4
    # staging: 16 KiB and 4 KiB polynomials are staged under autom_lds = 1; 128 KiB ones never are (the launcher's fallback)
    assert sc.BY_NAME["autom-p62-16384"]["lds"] == (1,) and 16384 * 8 > 64 << 10 >= 2 * 1024 * 8
    assert sum(len(c["lds"]) for c in sc.CASES) <= 30          # GPU cases in tests/test_gpu_prime_streaming.py


def test_every_full_call_sits_on_its_first_streaming_batch():
    for c in sc.CASES:
        assert streamed(c["launches"]), (c["name"], "the full call does not stream")
        assert not streamed(c["below"]), (c["name"], "one batch element fewer streams too", streamed(c["below"]))
        assert [label for label, _ in c["launches"]] == [label for label, _ in c["below"]]
    # which launches of one call stream
    for name in ("autom-p62-1024", "autom-p30-1024", "autom-p62-16384", "autoks-p62-k1", "autoks-p30-k2", "merge-p62-k1", "merge-p30-k2",
                 "multibit-setup-p62", "multibit-setup-native64"):
        assert len(sc.BY_NAME[name]["launches"]) == 1
    assert streamed(sc.BY_NAME["trace-p62-k1"]["launches"]) == ["keyswitch step 0", "keyswitch step 1"]
    m2, m4 = sc.BY_NAME["ringpack-p62-m2"], sc.BY_NAME["ringpack-p62-m4"]
    # M = 2: the one tree level is a leaf level and streams, and so does each of the nine trace steps after it
    assert [label for label, _ in m2["launches"]] == ["tree level 1 (leaf)"] + ["trace step %d" % r for r in range(9)]
    assert streamed(m2["launches"]) == [label for label, _ in m2["launches"]]
    # M = 4: the leaf level holds 2 * batch ciphertexts and streams; the level above it and the eight trace steps do not
    assert [label for label, _ in m4["launches"]] == ["tree level 1 (leaf)", "tree level 2"] + ["trace step %d" % r for r in range(8)]
    assert streamed(m4["launches"]) == ["tree level 1 (leaf)"]
    assert dict(m4["launches"])["tree level 1 (leaf)"] == sc.digit_bytes(2 * m4["batch"], 1, 15, 1024, 8)


def test_no_reference_call_streams_at_any_launch():
    for c in sc.CASES:
        assert c["references"], c["name"]
        for r in c["references"]:
            assert r["launches"] and 1 <= r["batch"] < c["batch"], (c["name"], r["call"])
            assert not streamed(r["launches"]), (c["name"], r["call"], r["batch"], streamed(r["launches"]))
    # the references that split the batch cover it
    for c in sc.CASES:
        split = [r["batch"] for r in c["references"] if r["call"].endswith("(half)") or r["call"].endswith("(half), step 0") or r["call"] == "ring_pack (chunk)"]
        assert sum(split) == c["batch"], (c["name"], split)
    # ring packing: every tree level and every trace step of both references, on every chunk
    for name, m in (("ringpack-p62-m2", 2), ("ringpack-p62-m4", 4)):
        c = sc.BY_NAME[name]
        assert sum(c["chunks"]) == c["batch"]
        for r in c["references"]:
            assert r["batch"] in c["chunks"] and len(r["launches"]) == 10          # log2 M tree levels + log2 n - log2 M trace steps


def test_every_case_stays_within_the_memory_cap():
    for c in sc.CASES:
        assert c["device_bytes"] == sum(nbytes for _, nbytes in c["device_buffers"])
        assert all(nbytes >= 0 for _, nbytes in c["device_buffers"])
        assert sc.STREAM_BYTES < c["device_bytes"] <= sc.MEM_CAP, (c["name"], c["device_bytes"])


def test_the_calls_accept_every_case():
    for c in sc.CASES:
        assert sc.refusals(c) == [], (c["name"], sc.refusals(c))
        if c["p"]:
            assert c["base_log"] * c["levels"] <= c["p"].bit_length() and (c["p"] - 1) % (2 * c["n"]) == 0
        for t in c["ts"]:
            assert t % 2 == 1 and t < 2 * c["n"]
    # the largest level count the primes take at these digit widths, capped at 15
    assert 4 * 15 <= P62.bit_length() == 62 < 4 * 16 and 2 * 15 == P30.bit_length() == 30
    # t in {3, n + 1, 2n - 1} is spread over the cases of each call that takes an exponent
    for call in ("automorphism", "autoks", "merge"):
        seen = {(t - 1) % c["n"] if t != 2 * c["n"] - 1 else -1 for c in sc.CASES if c["call"] == call for t in c["ts"]}
        assert seen == {2, 0, -1}, (call, seen)
    assert sc.BY_NAME["merge-p62-k1"]["shifts"] == [1, 512]
    # the checks do refuse: a case bent out of shape is caught
    bent = dict(sc.BY_NAME["autoks-p30-k2"], base_log=3)
    assert sc.refusals(bent) and sc.refusals(dict(bent, base_log=2, ts=[4])) and sc.refusals(dict(bent, base_log=2, ts=[2049]))
