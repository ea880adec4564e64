"""tests/test_gpu_footprint.py continued for the multi-bit calls of include/cntt_prime_multibit.h on prime64 and prime32 plans at n = 64:
cntt_prime*_multibit_accumulate_batch, _blind_rotate_batch and _bootstrap_batch with a workspace of exactly
cntt_prime*_multibit_pbs_workspace_bytes.  Every operand is an exact-size slice of a guard-band arena (tests/guard_arena.py, as it is):
the output and the workspace written, terms, key, exponents and the look-up table read only.  Each case runs 16-byte aligned and again
one word past a 16-byte boundary (the workspace stays aligned, as the header wants it), asserts the written slice against the model
or the public calls on plain tensors, and check()s every arena: every band word and every read-only operand byte for byte.

What is live here.  The accumulate kernel stores and loads 16-byte vectors at the word's own alignment, gathers rot_rows per element
and the key per pattern; the bootstrap carves digits | rot_t | acc out of the caller's workspace, so its last store sits on the last
word of that slice."""
import numpy as np
import pytest

from guard_arena import GuardArena
from prime_multibit_model import model_accumulate
from test_gpu_footprint import _dev, guard
from test_gpu_prime_multibit import composition, group_rows, psi_of, rot_table, special_words
from test_gpu_prime_pbs import dt, host, key_ntt, make_plan, random_words
from test_prime_pbs_model import P30, P62

pytestmark = pytest.mark.gpu

N, L, K, BETA, ELL, G, BATCH = 64, 4, 1, 7, 2, 2, 3
CASES = [(p, odd) for p in (P62, P30) for odd in (False, True)]
IDS = ["%s-%s" % ("prime64" if p == P62 else "prime32", "odd" if odd else "aligned") for (p, odd) in CASES]


def bits_of(p):
    return 64 if p == P62 else 32


@pytest.mark.parametrize("p,odd", CASES, ids=IDS)
def test_multibit_accumulate_footprint(p, odd):
    """out_ntt written; terms_ntt, key_group and rot_rows (a uint32 arena of its own) read; against the big-integer model, g = 1 .. 4"""
    plan = make_plan(p, N)
    for g, nterms, nout, batch in ((1, 1, 1, 1), (2, 4, 2, 3), (3, 3, 5, 2), (4, 2, 1, 5)):
        rng = np.random.default_rng(200 + g)
        terms = special_words(rng, p, batch * nterms * N)
        key = special_words(rng, p, (nterms * nout << g) * N)
        rows = group_rows(rng, N, g, batch)
        ar = GuardArena(dt(p), True, 20 + g, odd).take("terms", terms).take("out", batch * nout * N, written=True, guard=guard(bits_of(p), N))
        ar.take("key", key).build()
        ra = GuardArena(np.uint32, True, 30 + g, odd).take("rot_rows", rows).build()
        plan.multibit_accumulate_batch(ar["out"], ar["terms"], ra["rot_rows"], ar["key"], nterms, nout, g)
        got = ar.check()["out"]
        ra.check()
        want = model_accumulate(terms.tolist(), key.tolist(), rows.tolist(), psi_of(plan), N, p, nterms, nout, g, batch)
        assert [int(x) for x in got] == want, (p, odd, g)


def rotation_operands(torch, plan, p, odd, seed):
    rng = np.random.default_rng(seed)
    lut = random_words(rng, p, (K + 1) * N)
    key = host(key_ntt(torch, plan, random_words(rng, p, ((L // G) * (K + 1) * ELL * (K + 1) << G) * N)), dt(p))
    wsb = plan.multibit_pbs_workspace_bytes(L, K, ELL, G, BATCH)
    assert wsb % np.dtype(dt(p)).itemsize == 0
    return rng, lut, key, wsb // np.dtype(dt(p)).itemsize


@pytest.mark.parametrize("p,odd", CASES, ids=IDS)
def test_multibit_blind_rotate_footprint(p, odd):
    """acc and the workspace (exactly multibit_pbs_workspace_bytes) written; lut, rot_t and bsk_mb read; against the public calls,
    group by group, on plain tensors"""
    import torch
    plan = make_plan(p, N)
    rng, lut, key, ws_words = rotation_operands(torch, plan, p, odd, 301)
    rot = rot_table(rng, N, L, BATCH)
    ar = GuardArena(dt(p), True, 41, odd).take("lut", lut).take("acc", BATCH * (K + 1) * N, written=True, guard=guard(bits_of(p), N))
    ar.take("bsk", key).take("ws", ws_words, written=True, guard=guard(bits_of(p), N), aligned=True).build()
    ra = GuardArena(np.uint32, True, 42, odd).take("rot_t", rot).build()
    plan.multibit_blind_rotate_batch(ar["acc"], ar["lut"], ra["rot_t"], ar["bsk"], L, K, BETA, ELL, G, workspace=ar["ws"], lut_per_element=False)
    got = ar.check()["acc"]
    ra.check()
    want = composition(torch, plan, p, N, _dev(torch, lut), _dev(torch, rot), _dev(torch, key), L, K, BETA, ELL, G, BATCH)
    torch.cuda.synchronize()
    assert got.any() and np.array_equal(got, host(want, dt(p))), (p, odd)


@pytest.mark.parametrize("p,odd", CASES, ids=IDS)
def test_multibit_bootstrap_footprint(p, odd):
    """lwe_out and the workspace (digits | rot_t | acc, exactly multibit_pbs_workspace_bytes) written; lwe_in, lut and bsk_mb read;
    against lwe_modswitch_batch, multibit_blind_rotate_batch, sample_extract_batch on plain tensors"""
    import torch
    plan = make_plan(p, N)
    rng, lut, key, ws_words = rotation_operands(torch, plan, p, odd, 302)
    lwe = random_words(rng, p, BATCH * (L + 1))
    ar = GuardArena(dt(p), True, 43, odd).take("lwe_in", lwe).take("lwe_out", BATCH * (K * N + 1), written=True, guard=guard(bits_of(p), N))
    ar.take("lut", lut).take("bsk", key).take("ws", ws_words, written=True, guard=guard(bits_of(p), N), aligned=True).build()
    plan.multibit_bootstrap_batch(ar["lwe_out"], ar["lwe_in"], ar["lut"], ar["bsk"], L, K, BETA, ELL, G, workspace=ar["ws"])
    got = ar.check()["lwe_out"]
    lwe_t, lut_t, key_t = _dev(torch, lwe), _dev(torch, lut), _dev(torch, key)
    rot_t = torch.zeros((L + 1) * BATCH, dtype=torch.int32, device="cuda")
    acc, steps = torch.zeros(BATCH * (K + 1) * N, dtype=lwe_t.dtype, device="cuda"), torch.zeros(BATCH * (K * N + 1), dtype=lwe_t.dtype, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    plan.multibit_blind_rotate_batch(acc, lut_t, rot_t, key_t, L, K, BETA, ELL, G)
    plan.sample_extract_batch(steps, acc, K, 0)
    torch.cuda.synchronize()
    assert got.any() and np.array_equal(got, host(steps, dt(p))), (p, odd)
