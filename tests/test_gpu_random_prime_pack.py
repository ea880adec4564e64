"""Seeded random sweep of the prime plans' packing keyswitch (include/cntt_prime_pack.h): seeds 0 .. 31 of the `primepack` family of
tests/random_prime_pack_cases.py -- random primes of every bit length on both word types, random digits and shapes -- each bit-exact
against the sequence of public calls the header states, none left out, and against the plain-int model of tests/prime_pack_model.py
wherever the probe of tests/random_cases.py says the big-integer model applies to the prime.  tests/test_random_prime_pack_cases.py
asserts, without a GPU, the corners those seeds reach."""
import numpy as np
import pytest

import random_cases as rc
import random_prime_pack_cases as pp
import test_gpu_prime_pack as tgp
from test_gpu_prime_pbs import make_plan
from test_prime_pbs_model import edge_words

pytestmark = pytest.mark.gpu

_applies = {}


def model_applies(oracle, p, bits):
    if (p, bits) not in _applies:
        _applies[(p, bits)] = rc.model_applies(oracle, p, bits)
    return _applies[(p, bits)]


def check_primepack(oracle, c):
    torch = tgp._torch()
    p, bits, n, k, m, lin, beta, ell, batch = (c[x] for x in ("p", "bits", "n", "k", "m", "lin", "base_log", "levels", "batch"))
    dtype = np.uint64 if bits == 64 else np.uint32
    plan = make_plan(p, n)
    rng = np.random.default_rng(c["data_seed"])
    lwe = rng.integers(0, p, size=batch * m * (lin + 1), dtype=np.uint64).astype(dtype)
    for j, e in enumerate(edge_words(p, beta, ell)):               # random canonical words mixed with the digit rule's edges
        if 3 * j < lwe.size:
            lwe[3 * j] = e
    key = rng.integers(0, p, size=lin * ell * (k + 1) * n, dtype=np.uint64).astype(dtype)
    got = tgp.run_pack(torch, plan, p, "device", lwe, key, lin, m, k, beta, ell, batch, with_ws=c["workspace"])
    want = tgp.compose(torch, plan, p, lwe, key, lin, m, k, beta, ell, batch)
    assert np.array_equal(got, want), ("public calls", tgp.first_difference(got, want), c)
    if model_applies(oracle, p, bits):
        want = tgp.model(p, lwe, key, lin, m, k, n, beta, ell, batch)
        assert np.array_equal(got, want), ("model", tgp.first_difference(got, want), c)


@pytest.mark.parametrize("seed", range(pp.SEEDS))
def test_random_prime_pack(oracle, seed):
    check_primepack(oracle, pp.case_primepack(seed))
