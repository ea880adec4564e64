"""Seeded random sweep of the prime plans' ring-packing calls (include/cntt_prime_ring_pack.h): seeds 0 .. 31 of the `primeringpack`
family of tests/random_prime_ring_pack_cases.py -- random primes of every bit length on both word types, random rotations, exponents,
digits, dimensions and counts -- none left out.  Per case, bit-exact: call 1 against the numpy model; call 2 against the sequence of
public calls the header states and, wherever the probe of tests/random_cases.py says the big-integer model applies to the prime, against
the plain-int model of tests/prime_ring_pack_model.py; call 3 against call 1, one call 2 per stage and the trace.
tests/test_random_prime_ring_pack_cases.py asserts, without a GPU, the corners those seeds reach."""
import numpy as np
import pytest

import random_prime_ring_pack_cases as pr
import test_gpu_prime_automorphism as tga
import test_gpu_prime_ring_pack as trp
from prime_ring_pack_model import embed_np, model_merge
from test_gpu_prime_pbs import dt, make_plan
from test_gpu_random_prime_automorphism import model_applies
from test_prime_pbs_model import edge_words

pytestmark = pytest.mark.gpu


def check_primeringpack(oracle, c):
    torch = tga._torch()
    p, bits, n, k, m, shift, t, beta, ell, batch = (c[x] for x in ("p", "bits", "n", "k", "lwe_count", "shift", "t", "base_log", "levels", "batch"))
    with_ws = c["workspace"]
    dtype = dt(p)
    assert np.dtype(dtype).itemsize * 8 == bits, c                  # the helpers pick the plan by the modulus
    plan = make_plan(p, n)
    rng = np.random.default_rng(c["data_seed"])
    logn = n.bit_length() - 1
    kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    per = k * ell * (k + 1) * n

    def words(count):
        w = rng.integers(0, p, size=count, dtype=np.uint64).astype(dtype)
        for j, e in enumerate(edge_words(p, beta, ell)):           # random canonical words mixed with the digit rule's edges
            if 3 * j < w.size:
                w[3 * j] = e
        return w
    # call 1
    lwe = words(batch * m * (k * n + 1))
    got = trp.run_embed(torch, plan, p, "device", lwe, k)
    assert np.array_equal(got, embed_np(lwe.reshape(-1, k * n + 1), p, k, n).reshape(-1)), ("embed", c)
    # call 2
    E, O = words(batch * (k + 1) * n), words(batch * (k + 1) * n)
    one = kt[:per] if k else None
    got = trp.run_merge(torch, plan, p, "device", E, O, one, shift, t, k, beta, ell, with_ws)
    want = trp.compose_merge(torch, plan, p, E, O, one, shift, t, k, beta, ell)
    assert np.array_equal(got, want), ("public calls", tga.first_difference(got, want), c)
    if model_applies(oracle, p, bits):
        ct = (k + 1) * n
        want = [w for b in range(batch) for w in model_merge(E[b * ct:(b + 1) * ct].tolist(), O[b * ct:(b + 1) * ct].tolist(), kw[:per].tolist(), p,
                                                             shift, t, k, n, beta, ell)]
        assert np.array_equal(got, np.array(want, dtype=dtype)), ("model", c)
    # call 3
    got = trp.run_pack(torch, plan, p, "device", lwe, kt, m, k, beta, ell, batch, with_ws)
    want = trp.compose_pack(torch, plan, p, lwe, kt, m, k, beta, ell, batch)
    assert np.array_equal(got, want), ("pack", tga.first_difference(got, want), c)


@pytest.mark.parametrize("seed", range(pr.SEEDS))
def test_random_prime_ring_pack(oracle, seed):
    check_primeringpack(oracle, pr.case_primeringpack(seed))
