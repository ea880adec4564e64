"""tests/test_gpu_footprint_multibit.py continued for the multi-bit calls of include/cntt_multibit.h on native32 and native64 plans at
n = 64: cntt_native_multibit_accumulate_batch, _blind_rotate_batch and _bootstrap_batch with a workspace of exactly
cntt_native_multibit_pbs_workspace_bytes.  Every operand is an exact-size slice of a guard-band arena (tests/guard_arena.py, as it is):
the words (accumulator, table, ciphertexts) in an arena of the word type, the residue planes, the exponents and the workspace in a
uint32 arena; outputs and workspace written, everything else read only.  Each case runs 16-byte aligned and again one word past a
16-byte boundary (the workspace stays aligned, as the header wants it), asserts the written slices against the model or the public
calls on plain tensors, and check()s every arena: every band word and every read-only operand byte for byte.

What is live here.  The accumulate kernel stores and loads 16-byte vectors at the residue's own 4-byte alignment on every plane,
gathers rot_rows per element and the key per pattern; the rotation carves digits | term planes | output planes (and the bootstrap
rot_t | acc behind them) out of the caller's workspace, so its last store sits on the last word of that slice."""
import numpy as np
import pytest

from guard_arena import GuardArena
from native_multibit_model import PRIMES32, fast_accumulate_plane
from test_gpu_footprint import _dev, guard_both
from test_gpu_native_multibit import composed_rotate, psis_of
from test_gpu_native_pbs import KINDS, _torch, host, key_planes, random_words, to_ints

pytestmark = pytest.mark.gpu

N, L, K, BETA, ELL, G, BATCH = 64, 4, 1, 7, 2, 2, 3
CASES = [(kind, odd) for kind in ("native64_plan32", "native32_plan32") for odd in (False, True)]
IDS = ["%s-%s" % (kind.split("_")[0], "odd" if odd else "aligned") for (kind, odd) in CASES]


@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_multibit_accumulate_footprint(kind, odd):
    """every out plane written; the terms and key planes and rot_rows read; against the per-prime model, g = 1 .. 4"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    psis, NP = psis_of(torch, plan), plan.NPRIMES
    for g, nterms, nout, batch in ((1, 1, 1, 1), (2, 4, 2, 3), (3, 5, 3, 2), (4, 9, 1, 5)):
        rng = np.random.default_rng(500 + g)
        T = [rng.integers(0, PRIMES32[i], size=batch * nterms * N, dtype=np.uint32) for i in range(NP)]
        Kp = [rng.integers(0, PRIMES32[i], size=(nterms * nout << g) * N, dtype=np.uint32) for i in range(NP)]
        rows = rng.integers(0, 2 * N, size=g * batch, dtype=np.uint32)
        rows[0] = 2 * N - 1
        ar = GuardArena(np.uint32, True, 60 + g, odd)
        for i in range(NP):
            ar.take("terms%d" % i, T[i]).take("out%d" % i, batch * nout * N, written=True, guard=guard_both(N)).take("key%d" % i, Kp[i])
        ar.take("rot_rows", rows).build()
        plan.multibit_accumulate_batch([ar["out%d" % i] for i in range(NP)], [ar["terms%d" % i] for i in range(NP)], ar["rot_rows"],
                                       [ar["key%d" % i] for i in range(NP)], nterms, nout, g)
        got = ar.check()
        for i in range(NP):
            want = fast_accumulate_plane(T[i], Kp[i], rows, psis[i], N, PRIMES32[i], nterms, nout, g, batch)
            assert np.array_equal(got["out%d" % i], want), (kind, odd, g, i)


def operands(torch, plan, seed):
    rng = np.random.default_rng(seed)
    lut = random_words(rng, plan, (K + 1) * N)
    key_words = random_words(rng, plan, ((L // G) * (K + 1) * ELL * (K + 1) << G) * N)
    planes = [host(x, np.uint32) for x in key_planes(torch, plan, key_words)]
    wsb = plan.multibit_pbs_workspace_bytes(L, K, ELL, G, BATCH)
    assert wsb % 4 == 0
    return rng, lut, planes, wsb // 4


def plane_arena(plan, planes, ws_words, seed, odd, extra=None):
    ar = GuardArena(np.uint32, True, seed, odd)
    for i, p in enumerate(planes):
        ar.take("bsk%d" % i, p)
    if extra is not None:
        ar.take("rot_t", extra)
    return ar.take("ws", ws_words, written=True, guard=guard_both(N), aligned=True).build()


@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_multibit_blind_rotate_footprint(kind, odd):
    """acc and the workspace (exactly multibit_pbs_workspace_bytes) written; lut, rot_t and the bsk_mb planes read; against the public
    calls, group by group, on plain tensors"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    rng, lut, planes, ws_words = operands(torch, plan, 601)
    rot = rng.integers(0, 2 * N, size=(L + 1) * BATCH, dtype=np.uint32)
    rot[0], rot[BATCH] = 2 * N - 1, N
    ar = GuardArena(plan.word_dtype, True, 71, odd).take("lut", lut).take("acc", BATCH * (K + 1) * N, written=True, guard=guard_both(N)).build()
    pa = plane_arena(plan, planes, ws_words, 72, odd, rot)
    plan.multibit_blind_rotate_batch(ar["acc"], ar["lut"], pa["rot_t"], [pa["bsk%d" % i] for i in range(plan.NPRIMES)], L, K, BETA, ELL, G,
                                     workspace=pa["ws"], lut_per_element=False)
    got = ar.check()["acc"]
    pa.check()
    want = composed_rotate(torch, plan, lut, rot, [_dev(torch, p) for p in planes], L, K, BETA, ELL, G, BATCH)
    assert got.any() and to_ints(plan, got) == want, (kind, odd)


@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_multibit_bootstrap_footprint(kind, odd):
    """lwe_out and the workspace (digits | terms | outputs | rot_t | acc, exactly multibit_pbs_workspace_bytes) written; lwe_in, lut and
    the bsk_mb planes read; against lwe_modswitch_batch, multibit_blind_rotate_batch, sample_extract_batch on plain tensors"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    rng, lut, planes, ws_words = operands(torch, plan, 602)
    lwe = random_words(rng, plan, BATCH * (L + 1))
    ar = GuardArena(plan.word_dtype, True, 73, odd).take("lwe_in", lwe).take("lwe_out", BATCH * (K * N + 1), written=True, guard=guard_both(N))
    ar.take("lut", lut).build()
    pa = plane_arena(plan, planes, ws_words, 74, odd)
    plan.multibit_bootstrap_batch(ar["lwe_out"], ar["lwe_in"], ar["lut"], [pa["bsk%d" % i] for i in range(plan.NPRIMES)], L, K, BETA, ELL, G,
                                  workspace=pa["ws"])
    got = ar.check()["lwe_out"]
    pa.check()
    lwe_t, lut_t, key_t = _dev(torch, lwe), _dev(torch, lut), [_dev(torch, p) for p in planes]
    rot_t = torch.zeros((L + 1) * BATCH, dtype=torch.int32, device="cuda")
    acc, steps = torch.zeros(BATCH * (K + 1) * N, dtype=lwe_t.dtype, device="cuda"), torch.zeros(BATCH * (K * N + 1), dtype=lwe_t.dtype, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    plan.multibit_blind_rotate_batch(acc, lut_t, rot_t, key_t, L, K, BETA, ELL, G)
    plan.sample_extract_batch(steps, acc, K, 0)
    torch.cuda.synchronize()
    assert got.any() and np.array_equal(got, host(steps, plan.word_dtype)), (kind, odd)
