"""The seeded sweep of the prime plans' multi-bit blind rotation (tests/random_prime_multibit_cases.py: random primes of every bit
length on both word types, every grouping, nout up to 5, wrapping subset sums): cntt_prime*_multibit_blind_rotate_batch, bit-exact
against the ring model of tests/prime_multibit_model.py with exact negacyclic products.  The model applies to EVERY prime, the
strict-range ones included: the call's products are exact."""
import random

import numpy as np
import pytest

from prime_multibit_model import model_multibit_rotate
from random_prime_multibit_cases import SEEDS, case_primemultibit, rot_of
from concrete_ntt_amd import prime32, prime64
from test_gpu_prime_pbs import _torch, dev, host, key_ntt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_multibit_blind_rotate(seed):
    torch = _torch()
    c = case_primemultibit(seed)
    p, n, k, g, L, beta, ell, batch = c["p"], c["n"], c["k"], c["g"], c["lwe_dim"], c["base_log"], c["levels"], c["batch"]
    d = np.uint64 if c["bits"] == 64 else np.uint32
    plan = (prime64 if c["bits"] == 64 else prime32).Plan.try_new(n, p)             # the word type is the case's, whatever the prime's size
    assert plan is not None, c
    rng = random.Random("primemultibit/data/%d" % c["data_seed"])
    lut = [rng.randrange(p) for _ in range((batch if c["per_element"] else 1) * (k + 1) * n)]
    key = [rng.randrange(p) for _ in range((c["groups"] * (k + 1) * ell * (k + 1) << g) * n)]
    key[:3], lut[:3] = [0, 1, p - 1], [p - 1, 0, 1]
    rot = rot_of(c)
    ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch), dtype=torch.uint8, device="cuda") if c["workspace"] else None
    acc = dev(torch, np.zeros(batch * (k + 1) * n, dtype=d))
    plan.multibit_blind_rotate_batch(acc, dev(torch, np.array(lut, dtype=d)), dev(torch, np.array(rot, dtype=np.uint32)),
                                     key_ntt(torch, plan, np.array(key, dtype=d)), L, k, beta, ell, g, workspace=ws,
                                     lut_per_element=c["per_element"])
    torch.cuda.synchronize()
    want = model_multibit_rotate(lut, rot, key, p, n, L, k, beta, ell, g, batch, c["per_element"])
    assert [int(x) for x in host(acc, d)] == want, c
