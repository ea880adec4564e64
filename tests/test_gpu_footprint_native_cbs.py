"""tests/test_gpu_footprint_native_cmux.py continued for include/cntt_cbs.h on a 32-, a 64- and a 128-bit native kind.  The words -- lwe_in
and the functional key -- are exact-size slices of a guard-band arena (tests/guard_arena.py, as it is) of the word type; the output
planes, the planes of the bootstrapping key and the caller's workspace are slices of a uint32 arena; every output plane and the
workspace written, everything else read only.  The 32- and 64-bit kinds run 16-byte aligned and again one word past a 16-byte boundary
(fpksk and the workspace stay 16-byte aligned, as the header wants them); a 128-bit word promises 16 bytes itself, so that kind runs
aligned only.  The workspace is exactly cntt_native_circuit_bootstrap_workspace_bytes long or absent.  Each case asserts the written
planes bit-exact against the call on plain tensors (which tests/test_gpu_native_cbs.py pins to the public calls) and check()s both arenas:
every band word and every input byte for byte what it was, and the workspace written within the formula's bytes.

What is live at these shapes.  At n = 32, k = 1 a key row is 16 (64-bit words: 32, 128-bit: 64) vectors of 16 bytes, so at least 192 of the
256 threads of the product own no column and only the bound keeps them from reading behind the key; 11 elements are one full tile and
one of 3, whose five missing elements are neither read nor stored; the selector words are the LAST part of the workspace, so its end is
the end of the caller's buffer."""
import numpy as np
import pytest

import test_gpu_native_cbs as tcb
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_native_pbs import KINDS, _torch, host, per, seed, wbits

pytestmark = pytest.mark.gpu

CASES = [(kind, odd) for kind in ("native32_plan32", "native64_plan32") for odd in (False, True)] + [("native128_plan32", False)]
IDS = ["%s-%s" % (kind.split("_")[0], "odd" if odd else "aligned") for (kind, odd) in CASES]
N = 32


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_circuit_bootstrap_footprint(kind, odd, with_ws):
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    for k, L, batch, Lk, Lc in ((1, 4, 11, 3, 1), (0, 0, 3, 1, 2), (2, 3, 2, 1, 2)):
        gad = tcb.gadgets(wbits(plan), Lk, Lc)
        pb, pl, kb, kl, cb, cl = gad
        rng = np.random.default_rng(seed("fp-native-cbs", kind, k, odd))
        lwe, bsk_planes, fk = tcb.random_case(torch, plan, rng, L, k, gad, batch)
        torch.cuda.synchronize()
        wsb = plan.circuit_bootstrap_workspace_bytes(L, k, pl, kl, cl, batch)
        count = batch * tcb.sizes(k, N, kl, cl)[2] * N
        assert wsb % 16 == 0 and wsb > 0
        ar = GuardArena(np.uint64 if plan.WORD == 16 else plan.word_dtype, True, 151 + k, odd)
        ar.take("lwe_in", lwe)
        ar.take("fpksk", fk, aligned=True)
        ar.build()
        pa = GuardArena(np.uint32, True, 161 + k, odd)
        for i in range(plan.NPRIMES):
            pa.take("out%d" % i, count, written=True, guard=MIN_GUARD_POLYS * N)
            if L:
                pa.take("bsk%d" % i, host(bsk_planes[i], np.uint32))
        if with_ws:
            pa.take("ws", wsb // 4, written=True, guard=MIN_GUARD_POLYS * N, aligned=True)
        pa.build()
        plan.circuit_bootstrap_batch([pa["out%d" % i] for i in range(plan.NPRIMES)], ar["lwe_in"], [pa["bsk%d" % i] for i in range(plan.NPRIMES)] if L else None,
                                     ar["fpksk"], L, k, pb, pl, kb, kl, cb, cl, workspace=pa["ws"] if with_ws else None)
        ar.check()
        got = pa.check()
        want = tcb.run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
        assert all(np.array_equal(got["out%d" % i], want[i]) for i in range(plan.NPRIMES)), (kind, k, odd, with_ws)
        assert any(w_.any() for w_ in want), (kind, k)
