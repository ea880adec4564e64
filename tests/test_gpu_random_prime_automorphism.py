"""Seeded random sweep of the prime plans' automorphism calls (include/cntt_prime_automorphism.h): seeds 0 .. 31 of the `primeautom`
family of tests/random_prime_automorphism_cases.py -- random primes of every bit length on both word types, random exponents, digits,
dimensions and steps -- none left out.  Per case, bit-exact: calls 1 and 2 against the numpy model; call 3 against the sequence of
public calls the header states and, wherever the probe of tests/random_cases.py says the big-integer model applies to the prime,
against the plain-int model of tests/prime_automorphism_model.py; call 4 against `steps` calls of 3.
tests/test_random_prime_automorphism_cases.py asserts, without a GPU, the corners those seeds reach."""
import numpy as np
import pytest

import random_cases as rc
import random_prime_automorphism_cases as pa
import test_gpu_prime_automorphism as tga
from prime_automorphism_model import autom_gather_np, model_autoks_batch, ntt_permutation
from test_gpu_prime_pbs import dev, dt, host, make_plan
from test_prime_pbs_model import edge_words

pytestmark = pytest.mark.gpu

_applies = {}


def model_applies(oracle, p, bits):
    if (p, bits) not in _applies:
        _applies[(p, bits)] = rc.model_applies(oracle, p, bits)
    return _applies[(p, bits)]


def check_primeautom(oracle, c):
    torch = tga._torch()
    p, bits, n, k, t, steps, beta, ell, batch = (c[x] for x in ("p", "bits", "n", "k", "t", "steps", "base_log", "levels", "batch"))
    add, with_ws = c["add_input"], c["workspace"]
    dtype = dt(p)
    assert np.dtype(dtype).itemsize * 8 == bits, c                  # the helpers pick the plan by the modulus
    plan = make_plan(p, n)
    rng = np.random.default_rng(c["data_seed"])
    ct = rng.integers(0, p, size=batch * (k + 1) * n, dtype=np.uint64).astype(dtype)
    for j, e in enumerate(edge_words(p, beta, ell)):               # random canonical words mixed with the digit rule's edges
        if 3 * j < ct.size:
            ct[3 * j] = e
    kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=max(steps, 1))
    one = kt[:k * ell * (k + 1) * n] if k else None
    # calls 1 and 2
    a, b = dev(torch, tga.poison(p, ct.size)), dev(torch, tga.poison(p, ct.size))
    plan.automorphism_batch(a, dev(torch, ct), t)
    plan.automorphism_ntt_batch(b, dev(torch, ct), t)
    assert np.array_equal(host(a, dtype), autom_gather_np(ct.reshape(-1, n), t, p).reshape(-1)), ("automorphism", c)
    assert np.array_equal(host(b, dtype), ct.reshape(-1, n)[:, ntt_permutation(t, n)].reshape(-1)), ("automorphism_ntt", c)
    # call 3
    got = tga.run_autoks(torch, plan, p, "device", ct, one, t, k, beta, ell, add, batch, with_ws)
    want = tga.compose(torch, plan, p, ct, one, t, k, beta, ell, add, batch)
    assert np.array_equal(got, want), ("public calls", tga.first_difference(got, want), c)
    if model_applies(oracle, p, bits):
        per = k * ell * (k + 1) * n
        want = np.array(model_autoks_batch(ct.tolist(), kw[:per].tolist(), p, t, k, n, beta, ell, add, batch), dtype=dtype)
        assert np.array_equal(got, want), ("model", tga.first_difference(got, want), c)
    # call 4
    keys = kt[:steps * k * ell * (k + 1) * n] if k and steps else None
    got = tga.run_trace(torch, plan, p, "device", ct, keys, steps, k, beta, ell, batch, with_ws)
    want = tga.steps_of_call_3(torch, plan, p, ct, kt, steps, k, beta, ell, batch)
    assert np.array_equal(got, want), ("trace", tga.first_difference(got, want), c)


@pytest.mark.parametrize("seed", range(pa.SEEDS))
def test_random_prime_automorphism(oracle, seed):
    check_primeautom(oracle, pa.case_primeautom(seed))
