"""tests/test_gpu_footprint_automorphism.py continued for include/cntt_prime_ring_pack.h: the embedding, one tree node and the whole
packing.  Every operand -- the inputs, the key, the output, the caller's workspace -- is an exact-size slice of ONE guard-band arena
(tests/guard_arena.py) at the word's own alignment (16-byte aligned, and one word past a 16-byte boundary), the workspace exactly
cntt_prime*_..._workspace_bytes long and 16-byte aligned.  Each case asserts the written slice bit-exact against the call on plain
tensors (which tests/test_gpu_prime_ring_pack.py pins to the model and the public calls) and check() on the arena: every band word, and
the inputs and the key, byte for byte what they were.

What is live at these shapes.  One workgroup serves one output polynomial with 16-byte stores, so at n = 16 (64-bit words) and n = 32
(32-bit words) 248 of its 256 threads own no vector and only the loop bound keeps them from storing behind the operand.  The LWE rows are
k n + 1 words long, so the last row of lwe_in ends on a word that no vector load may straddle.  The packing's stages and trace steps
alternate between the two ciphertext buffers at the END of the workspace: the widest stage fills the first to its last byte, and with
M >= 4 the second stage fills the second, whose end is the end of the caller's workspace."""
import numpy as np
import pytest

import test_gpu_prime_automorphism as tga
import test_gpu_prime_ring_pack as trp
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint_automorphism import CASES, IDS
from test_gpu_prime_pbs import dt, host, make_plan, min_n

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_embed_footprint(p, odd, device):
    """call 1 with k = 0, 1, 2: glwe_out written, lwe_in read; batch 3"""
    torch = tga._torch()
    for n in (min_n(p), 64):
        plan = make_plan(p, n)
        for k in (0, 1, 2):
            rng = np.random.default_rng(tga.seed("fp-embed", p, n, k, odd))
            lwe = tga.words_with_zeros(rng, p, 3 * (k * n + 1))
            ar = GuardArena(dt(p), device, 61 + k, odd).take("glwe_out", 3 * (k + 1) * n, written=True, guard=MIN_GUARD_POLYS * n).take("lwe_in", lwe).build()
            plan.glwe_embed_batch(ar["glwe_out"], ar["lwe_in"], k)
            got = ar.check()["glwe_out"]
            assert got.any() and np.array_equal(got, trp.run_embed(torch, plan, p, "device", lwe, k)), (p, n, k, odd, device)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_merge_footprint(p, odd, device, with_ws):
    """call 2 with k = 0 (no key, no workspace), 1 and 2"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    for n in (min_n(p), 64):
        plan = make_plan(p, n)
        for k, beta, ell, batch in ((0, 4, 2, 3), (1, 5, 3, 3), (2, 6, 2, 1)):
            rng = np.random.default_rng(tga.seed("fp-merge", p, n, k, odd))
            kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n)
            torch.cuda.synchronize()
            E, O = (tga.words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
            shift, t = n + 3, n // 2 + 1
            wsb = plan.glwe_merge_workspace_bytes(k, ell, batch)
            assert wsb % isz == 0 and (wsb == 0) == (k == 0)
            ar = GuardArena(dt(p), device, 71 + k, odd).take("glwe_out", E.size, written=True, guard=MIN_GUARD_POLYS * n).take("even", E).take("odd", O)
            if k:
                ar.take("ak_ntt", host(kt, dt(p)))
            if with_ws and wsb:
                ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
            ar.build()
            plan.glwe_merge_batch(ar["glwe_out"], ar["even"], ar["odd"], ar["ak_ntt"] if k else None, shift, t, k, beta, ell,
                                  workspace=ar["ws"] if with_ws and wsb else None)
            got = ar.check()["glwe_out"]
            want = trp.run_merge(torch, plan, p, "device", E, O, kt, shift, t, k, beta, ell)
            assert got.any() and np.array_equal(got, want), (p, n, k, odd, device, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_ring_pack_footprint(p, odd, device, with_ws):
    """call 3 with M = 1 (the embedding and the trace), 2 (one stage), 8 (both buffers filled) and n (the last stage writes glwe_out)"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    logn = n.bit_length() - 1
    plan = make_plan(p, n)
    k, beta, ell, batch = 1, 5, 2, 3
    rng = np.random.default_rng(tga.seed("fp-ring-pack", p, odd))
    kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    torch.cuda.synchronize()
    for m in (1, 2, 8, n):
        lwe = tga.words_with_zeros(rng, p, batch * m * (k * n + 1))
        wsb = plan.ring_pack_workspace_bytes(m, k, ell, batch)
        assert wsb % isz == 0
        ar = GuardArena(dt(p), device, 81 + m, odd).take("glwe_out", batch * (k + 1) * n, written=True, guard=MIN_GUARD_POLYS * n).take("lwe_in", lwe)
        ar.take("ak_ntt", host(kt, dt(p)))
        if with_ws:
            ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
        ar.build()
        plan.ring_pack_batch(ar["glwe_out"], ar["lwe_in"], ar["ak_ntt"], m, k, beta, ell, workspace=ar["ws"] if with_ws else None)
        got = ar.check()["glwe_out"]
        want = trp.run_pack(torch, plan, p, "device", lwe, kt, m, k, beta, ell, batch)
        assert got.any() and np.array_equal(got, want), (p, m, odd, device, with_ws)
