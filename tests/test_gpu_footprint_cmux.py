"""tests/test_gpu_footprint_ring_pack.py continued for include/cntt_prime_cmux.h: one CMux and the whole tree.  Every operand -- the
inputs, the selectors, the output, the caller's workspace -- is an exact-size slice of ONE guard-band arena (tests/guard_arena.py) at the
word's own alignment (16-byte aligned, and one word past a 16-byte boundary), the workspace exactly cntt_prime*_..._workspace_bytes long
and 16-byte aligned.  Each case asserts the written slice bit-exact against the call on plain tensors (which
tests/test_gpu_prime_cmux.py pins to the model and the public calls) and check() on the arena: every band word, and the inputs and the
selectors, byte for byte what they were.

What is live at these shapes.  One workgroup serves one output polynomial with 16-byte loads and stores, so at n = 16 (64-bit words) and
n = 32 (32-bit words) 248 of its 256 threads own no vector and only the loop bound keeps them from reaching behind the operand.  The leaf
stage writes `levels` digit polynomials per ciphertext where the later stages write (k + 1) * levels: the digits part of the workspace
is the larger of the two, filled to its last byte by one of them.  The stages alternate between the two ciphertext buffers at the END of
the workspace: stage 1 fills the first to its last byte, and with M >= 4 stage 2 fills the second, whose end is the end of the caller's
workspace.  M = 1 writes the trivial ciphertext and touches no workspace at all."""
import numpy as np
import pytest

import test_gpu_prime_automorphism as tga
import test_gpu_prime_cmux as tpc
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint_automorphism import CASES, IDS
from test_gpu_prime_pbs import dt, host, make_plan, min_n

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_cmux_footprint(p, odd, device, with_ws):
    """call 1 with k = 0, 1 and 2"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    for n in (min_n(p), 64):
        plan = make_plan(p, n)
        for k, beta, ell, batch in ((0, 4, 2, 3), (1, 5, 3, 3), (2, 6, 2, 1)):
            rng = np.random.default_rng(tga.seed("fp-cmux", p, n, k, odd))
            kw, kt = tpc.selectors(torch, plan, p, rng, k, ell, n)
            torch.cuda.synchronize()
            c0, c1 = (tga.words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
            wsb = plan.glwe_cmux_workspace_bytes(k, ell, batch)
            assert wsb % isz == 0 and wsb > 0
            ar = GuardArena(dt(p), device, 91 + k, odd).take("glwe_out", c0.size, written=True, guard=MIN_GUARD_POLYS * n).take("glwe0", c0).take("glwe1", c1)
            ar.take("ggsw_ntt", host(kt, dt(p)))
            if with_ws:
                ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
            ar.build()
            plan.glwe_cmux_batch(ar["glwe_out"], ar["glwe0"], ar["glwe1"], ar["ggsw_ntt"], k, beta, ell, workspace=ar["ws"] if with_ws else None)
            got = ar.check()["glwe_out"]
            want = tpc.run_cmux(torch, plan, p, "device", c0, c1, kt, k, beta, ell)
            assert got.any() and np.array_equal(got, want), (p, n, k, odd, device, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_cmux_tree_footprint(p, odd, device, with_ws):
    """call 2 with M = 1 (the trivial ciphertext, no selector, no workspace), 2 (the leaf stage writes glwe_out), 4 (both kinds of
    stage) and 16 (both buffers filled twice); k = 1, where the later stages need the larger digits part, and k = 0, where the leaf stage
    does"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    plan = make_plan(p, n)
    beta, ell, batch = 5, 2, 3
    for k in (1, 0):
        rng = np.random.default_rng(tga.seed("fp-cmux-tree", p, odd, k))
        for m in (1, 2, 4, 16):
            depth = m.bit_length() - 1
            kt = tpc.selectors(torch, plan, p, rng, k, ell, n, depth)[1] if depth else None
            torch.cuda.synchronize()
            lut = tga.words_with_zeros(rng, p, batch * m * n)
            wsb = plan.cmux_tree_workspace_bytes(m, k, ell, batch)
            assert wsb % isz == 0 and (wsb == 0) == (m == 1)
            ar = GuardArena(dt(p), device, 101 + m, odd).take("glwe_out", batch * (k + 1) * n, written=True, guard=MIN_GUARD_POLYS * n).take("lut_in", lut)
            if depth:
                ar.take("ggsw_ntt", host(kt, dt(p)))
            if with_ws and wsb:
                ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
            ar.build()
            plan.cmux_tree_batch(ar["glwe_out"], ar["lut_in"], ar["ggsw_ntt"] if depth else None, m, k, beta, ell,
                                 workspace=ar["ws"] if with_ws and wsb else None)
            got = ar.check()["glwe_out"]
            want = tpc.run_tree(torch, plan, p, "device", lut, kt, m, k, beta, ell, batch)
            assert got.any() and np.array_equal(got, want), (p, m, k, odd, device, with_ws)
