"""The seeded sweep of the native plans' multi-bit blind rotation (tests/random_native_multibit_cases.py: every Plan32 kind with every
grouping, nout up to 3, J on both sides of the kernel's chunk of four, wrapping subset sums): cntt_native_multibit_blind_rotate_batch,
bit-exact against the ring model of tests/native_multibit_model.py with exact negacyclic products."""
import numpy as np
import pytest

from native_multibit_model import model_multibit_rotate
from random_native_multibit_cases import SEEDS, case_nativemultibit, rot_of
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, random_key_words, random_words, to_array, to_ints

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SEEDS))
def test_random_multibit_blind_rotate(seed):
    torch = _torch()
    c = case_nativemultibit(seed)
    n, k, g, L, beta, ell, batch, w = c["n"], c["k"], c["g"], c["lwe_dim"], c["base_log"], c["levels"], c["batch"], c["w"]
    plan = KINDS[c["kind"]].try_new(n)
    rng = np.random.default_rng(c["data_seed"])
    lut = to_ints(plan, random_words(rng, plan, (batch if c["per_element"] else 1) * (k + 1) * n))
    key = to_ints(plan, random_key_words(rng, plan, (c["groups"] * (k + 1) * ell * (k + 1)) << g))
    top = 1 if plan.BINARY else (1 << w) - 1
    key[:3], lut[:3] = [0, 1, top], [(1 << w) - 1, 0, 1]
    rot = rot_of(c)
    ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch), dtype=torch.uint8, device="cuda") if c["workspace"] else None
    acc = dev(torch, to_array(plan, [0] * (batch * (k + 1) * n)))
    plan.multibit_blind_rotate_batch(acc, dev(torch, to_array(plan, lut)), dev(torch, np.array(rot, dtype=np.uint32)),
                                     key_planes(torch, plan, to_array(plan, key)), L, k, beta, ell, g, workspace=ws,
                                     lut_per_element=c["per_element"])
    torch.cuda.synchronize()
    want = model_multibit_rotate(lut, rot, key, w, n, L, k, beta, ell, g, batch, c["per_element"])
    assert to_ints(plan, host(acc, plan.word_dtype)) == want, c
