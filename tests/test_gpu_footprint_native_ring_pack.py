"""tests/test_gpu_footprint_native_automorphism.py continued for include/cntt_ring_pack.h on a 32-, a 64- and a 128-bit native kind: the
embedding, the merge and the pack.  The words -- the LWE rows, the ciphertexts, the output -- are exact-size slices of a guard-band arena
(tests/guard_arena.py, as it is) of the word type, the residue planes of the keys and the caller's workspace slices of a uint32 arena;
the output and the workspace written, everything else read only.  The 32- and 64-bit kinds run 16-byte aligned and again one word past
a 16-byte boundary; the 128-bit kind runs aligned only.  The workspace stays 16-byte aligned and is exactly
cntt_native_*_workspace_bytes long or absent.  Each case asserts the written slice bit-exact against the call on plain tensors (which
tests/test_gpu_native_ring_pack.py pins to the public calls) and check()s both arenas: every band word, the inputs and the keys byte for
byte what they were, and the workspace written within the formula's bytes.  A refused call writes nothing.

What is live at these shapes.  LWE rows of k n + 1 words end one word after a polynomial boundary, so the leaf reads of the last row end
at the last word of lwe_in; the leaf stage reads `odd` h rows after `even`, up to the end of the operand; the pack's two buffers are the
END of the workspace, and which one the last stage writes depends on the parity of log2 M."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_native_automorphism as tna
import test_gpu_native_ring_pack as trp
from concrete_ntt_amd._lib import Panic
from guard_arena import MIN_GUARD_POLYS
from test_gpu_footprint_native_automorphism import CASES, IDS, N, plane_arena, word_arena
from test_gpu_native_pbs import KINDS, _torch, per, seed

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_embed_footprint(kind, odd):
    """call 1 with k = 0, 1 and 2"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    for k, batch in ((0, 3), (1, 3), (2, 2)):
        rng = np.random.default_rng(seed("fp-native-embed", kind, k, odd))
        lwe = tna.random_words(rng, plan, batch * (k * N + 1))
        ar = word_arena(plan, 311 + k, odd)
        ar.take("glwe_out", batch * (k + 1) * pe, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("lwe_in", lwe)
        ar.build()
        plan.glwe_embed_batch(ar["glwe_out"], ar["lwe_in"], k)
        got = ar.check()["glwe_out"]
        assert got.any() and np.array_equal(got, trp.embed_rows(torch, plan, lwe, k)), (kind, k, odd)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_merge_footprint(kind, odd, with_ws):
    """call 2 with k = 0, 1 and 2, both settings of the switch"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    for k, beta, ell, batch, lds in ((0, 4, 2, 3, 1), (1, 5, 3, 3, 0), (2, 6, 2, 1, 1)):
        rng = np.random.default_rng(seed("fp-native-merge", kind, k, odd))
        kr = tna.ak_planes(torch, plan, rng, k, ell) if k else None
        torch.cuda.synchronize()
        even, odd_ct = tna.random_words(rng, plan, batch * (k + 1) * N), tna.random_words(rng, plan, batch * (k + 1) * N)
        wsb = plan.glwe_merge_workspace_bytes(k, ell, batch)
        assert wsb % 16 == 0 and (wsb > 0) == (k > 0)
        ar = word_arena(plan, 321 + k, odd)
        ar.take("glwe_out", even.size, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("glwe_even", even)
        ar.take("glwe_odd", odd_ct)
        ar.build()
        pa = plane_arena(plan, kr, wsb if with_ws else 0, 331 + k, odd)
        with cntt.debug_switches(autom_lds=lds):
            plan.glwe_merge_batch(ar["glwe_out"], ar["glwe_even"], ar["glwe_odd"], [pa["key%d" % i] for i in range(plan.NPRIMES)] if k else None,
                                  N + 3, 2 * N - 3, k, beta, ell, workspace=pa["ws"] if with_ws and wsb else None)
        got = ar.check()["glwe_out"]
        if pa is not None:
            pa.check()
        want = trp.run_merge(torch, plan, "device", even, odd_ct, kr, N + 3, 2 * N - 3, k, beta, ell)
        assert got.any() and np.array_equal(got, want), (kind, k, odd, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_ring_pack_footprint(kind, odd, with_ws):
    """call 3 with M = 1 (the embedding into the workspace, then the full trace), 2 (the leaf stage alone, then the trace) and n (the
    last merge writes glwe_out)"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    k, beta, ell, batch = 1, 5, 2, 2
    rng = np.random.default_rng(seed("fp-native-ring-pack", kind, odd))
    kr = tna.ak_planes(torch, plan, rng, k, ell, 5)
    torch.cuda.synchronize()
    for m in (1, 2, N):
        lwe = tna.random_words(rng, plan, batch * m * (k * N + 1))
        wsb = plan.ring_pack_workspace_bytes(m, k, ell, batch)
        assert wsb % 16 == 0 and wsb > 0
        ar = word_arena(plan, 341 + m, odd)
        ar.take("glwe_out", batch * (k + 1) * pe, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("lwe_in", lwe)
        ar.build()
        pa = plane_arena(plan, kr, wsb if with_ws else 0, 351 + m, odd)
        plan.ring_pack_batch(ar["glwe_out"], ar["lwe_in"], [pa["key%d" % i] for i in range(plan.NPRIMES)], m, k, beta, ell,
                             workspace=pa["ws"] if with_ws else None)
        got = ar.check()["glwe_out"]
        pa.check()
        want = trp.run_pack(torch, plan, "device", lwe, kr, m, k, beta, ell, False)
        assert got.any() and np.array_equal(got, want), (kind, m, odd, with_ws)


@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_refused_calls_write_nothing(kind, odd):
    """an even exponent, a shift of 2n and a lwe_count that is no power of two: CNTT_EINVAL, and neither the output nor the workspace nor
    any band word changes"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    k, beta, ell, batch, m = 1, 5, 2, 2, 4
    rng = np.random.default_rng(seed("fp-native-ring-refused", kind, odd))
    kr = tna.ak_planes(torch, plan, rng, k, ell, 5)
    torch.cuda.synchronize()
    ct = tna.random_words(rng, plan, batch * (k + 1) * N)
    lwe = tna.random_words(rng, plan, batch * m * (k * N + 1))
    ar = word_arena(plan, 361, odd)
    ar.take("glwe_out", ct.size, written=True, guard=MIN_GUARD_POLYS * pe)
    ar.take("glwe_even", ct)
    ar.take("glwe_odd", ct.copy())
    ar.take("lwe_in", lwe)
    ar.build()
    pa = plane_arena(plan, kr, plan.ring_pack_workspace_bytes(m, k, ell, batch), 371, odd)
    keys = [pa["key%d" % i] for i in range(plan.NPRIMES)]
    one = [p[:k * ell * (k + 1) * N] for p in keys]
    for call in (lambda: plan.glwe_merge_batch(ar["glwe_out"], ar["glwe_even"], ar["glwe_odd"], one, 3, 4, k, beta, ell, workspace=pa["ws"]),
                 lambda: plan.glwe_merge_batch(ar["glwe_out"], ar["glwe_even"], ar["glwe_odd"], one, 2 * N, 3, k, beta, ell, workspace=pa["ws"]),
                 lambda: plan.ring_pack_batch(ar["glwe_out"], ar["lwe_in"][:3 * batch * (k * N + 1) * trp.cw(plan)], keys, 3, k, beta, ell, workspace=pa["ws"]),
                 lambda: plan.ring_pack_batch(ar["glwe_out"], ar["lwe_in"], keys, m, k, 33 * plan.WORD, ell, workspace=pa["ws"])):
        with pytest.raises(Panic):
            call()
    ar.check(unchanged=("glwe_out",))
    pa.check(unchanged=("ws",))
