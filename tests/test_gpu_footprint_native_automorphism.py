"""tests/test_gpu_footprint_native_cmux.py continued for include/cntt_automorphism.h on a 32-, a 64- and a 128-bit native kind: the
automorphism, the Galois keyswitch and the trace.  The words -- the input, the output -- are exact-size slices of a guard-band arena
(tests/guard_arena.py, as it is) of the word type, the residue planes of the keys and the caller's workspace slices of a uint32 arena;
the output and the workspace written, everything else read only.  The 32- and 64-bit kinds run 16-byte aligned and again one word past
a 16-byte boundary, the least their words promise; a 128-bit word promises 16 bytes itself, so that kind runs aligned only.  The
workspace stays 16-byte aligned, as the header wants it, and is exactly cntt_native_*_workspace_bytes long or absent.  Each case asserts
the written slice bit-exact against the call on plain tensors (which tests/test_gpu_native_automorphism.py pins to the public calls) and
check()s both arenas: every band word, the input and the keys byte for byte what they were, and the workspace written within the
formula's bytes.

What is live at these shapes.  One workgroup serves one polynomial with 16-byte stores and gathers whose index is masked to the
polynomial, so at n = 32 at least 224 of its 256 threads own no vector and only the loop bound keeps them from reaching behind the
operand; the staging loads are 16-byte ones too.  The trace's second ciphertext is the END of the workspace, and with an even number of
steps the first stage writes it."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_native_automorphism as tna
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_native_pbs import KINDS, _torch, host, per, seed

pytestmark = pytest.mark.gpu

CASES = [(kind, odd) for kind in ("native32_plan32", "native64_plan32") for odd in (False, True)] + [("native128_plan32", False)]
IDS = ["%s-%s" % (kind.split("_")[0], "odd" if odd else "aligned") for (kind, odd) in CASES]
N = 32


def word_arena(plan, seed_, odd):
    """the arena of the words; a 128-bit word is two arena words"""
    return GuardArena(np.uint64 if plan.WORD == 16 else plan.word_dtype, True, seed_, odd)


def plane_arena(plan, kr, ws_bytes, seed_, odd):
    if not kr and not ws_bytes:
        return None
    ar = GuardArena(np.uint32, True, seed_, odd)
    for i, p in enumerate(kr or []):
        ar.take("key%d" % i, host(p, np.uint32))
    if ws_bytes:
        ar.take("ws", ws_bytes // 4, written=True, guard=MIN_GUARD_POLYS * N, aligned=True)
    return ar.build()


@pytest.mark.parametrize("lds", [1, 0], ids=["staged", "global"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_automorphism_footprint(kind, odd, lds):
    """call 1"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    rng = np.random.default_rng(seed("fp-native-autom", kind, odd))
    a = tna.random_words(rng, plan, 3 * N)
    for t in (N + 1, 2 * N - 1):
        ar = word_arena(plan, 211, odd)
        ar.take("out", a.size, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("in", a)
        ar.build()
        with cntt.debug_switches(autom_lds=lds):
            plan.automorphism_batch(ar["out"], ar["in"], t)
        got = ar.check()["out"]
        assert got.any() and np.array_equal(got, tna.sigma(plan, a, t)), (kind, odd, lds, t)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_autoks_footprint(kind, odd, with_ws):
    """call 3 with k = 0, 1 and 2, with and without add_input"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    for k, beta, ell, batch, add in ((0, 4, 2, 3, True), (1, 5, 3, 3, False), (2, 6, 2, 1, True)):
        rng = np.random.default_rng(seed("fp-native-autoks", kind, k, odd))
        kr = tna.ak_planes(torch, plan, rng, k, ell) if k else None
        torch.cuda.synchronize()
        ct = tna.ciphertexts(rng, plan, batch * (k + 1), beta, ell)
        wsb = plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch)
        assert wsb % 16 == 0 and (wsb > 0) == (k > 0)
        ar = word_arena(plan, 221 + k, odd)
        ar.take("glwe_out", ct.size, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("glwe_in", ct)
        ar.build()
        pa = plane_arena(plan, kr, wsb if with_ws else 0, 231 + k, odd)
        plan.glwe_automorphism_keyswitch_batch(ar["glwe_out"], ar["glwe_in"], [pa["key%d" % i] for i in range(plan.NPRIMES)] if k else None, 2 * N - 3, k,
                                               beta, ell, add, workspace=pa["ws"] if with_ws and wsb else None)
        got = ar.check()["glwe_out"]
        if pa is not None:
            pa.check()
        want = tna.run_autoks(torch, plan, "device", ct, kr, 2 * N - 3, k, beta, ell, add)
        assert got.any() and np.array_equal(got, want), (kind, k, odd, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_trace_footprint(kind, odd, with_ws):
    """call 4 with steps = 0 (a copy, no workspace touched), 1, 2 (the first stage writes the end of the workspace) and log2 n"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    k, beta, ell, batch = 1, 5, 2, 3
    rng = np.random.default_rng(seed("fp-native-trace", kind, odd))
    for steps in (0, 1, 2, 5):
        kr = tna.ak_planes(torch, plan, rng, k, ell, steps) if steps else None
        torch.cuda.synchronize()
        ct = tna.ciphertexts(rng, plan, batch * (k + 1), beta, ell)
        wsb = plan.glwe_trace_workspace_bytes(k, ell, batch)
        assert wsb % 16 == 0 and wsb > 0
        ar = word_arena(plan, 241 + steps, odd)
        ar.take("glwe_out", ct.size, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("glwe_in", ct)
        ar.build()
        pa = plane_arena(plan, kr, wsb if with_ws else 0, 251 + steps, odd)
        plan.glwe_trace_batch(ar["glwe_out"], ar["glwe_in"], [pa["key%d" % i] for i in range(plan.NPRIMES)] if steps else None, steps, k, beta, ell,
                              workspace=pa["ws"] if with_ws else None)
        got = ar.check()["glwe_out"]
        if pa is not None:
            pa.check()
        want = tna.run_trace(torch, plan, ct, kr, steps, k, beta, ell, False) if steps else ct
        assert got.any() and np.array_equal(got, want), (kind, steps, odd, with_ws)
