"""tests/test_gpu_footprint_cmux.py continued for include/cntt_cmux.h on a 32-, a 64- and a 128-bit native kind: one CMux and the whole
tree.  The words -- the inputs, the output -- are exact-size slices of a guard-band arena (tests/guard_arena.py, as it is) of the word
type, the residue planes of the selectors and the caller's workspace slices of a uint32 arena; glwe_out and the workspace written,
everything else read only.  The 32- and 64-bit kinds run 16-byte aligned and again one word past a 16-byte boundary, the least their
words promise; a 128-bit word promises 16 bytes itself, so that kind runs aligned only.  The workspace stays 16-byte aligned, as the
header wants it, and is exactly cntt_native_*_workspace_bytes long or absent.  Each case asserts the written slice bit-exact against the
call on plain tensors (which tests/test_gpu_native_cmux.py pins to the public calls) and check()s both arenas: every band word, the
inputs and the selectors byte for byte what they were, and the workspace written within the formula's bytes.

What is live at these shapes.  One workgroup serves one output polynomial with 16-byte loads and stores, so at n = 32 at least 224 of
its 256 threads own no vector and only the loop bound keeps them from reaching behind the operand.  The leaf stage writes `levels` digit
polynomials per ciphertext where the later stages write (k + 1) * levels: the digits part of the workspace is the larger of the two.
The stages alternate between the two ciphertext buffers at the END of the workspace: with M >= 4 stage 2 fills the second, whose end is
the end of the caller's workspace.  M = 1 writes the trivial ciphertext and touches no workspace at all."""
import numpy as np
import pytest

import test_gpu_native_cmux as tnc
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
    if not kr and not ws_bytes:             # one table entry: neither selectors nor a workspace
        return None
    ar = GuardArena(np.uint32, True, seed_, odd)
    for i, p in enumerate(kr or []):
        ar.take("sel%d" % i, host(p, np.uint32))
    if ws_bytes:
        ar.take("ws", ws_bytes // 4, written=True, guard=MIN_GUARD_POLYS * N, aligned=True)
    return ar.build()


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_cmux_footprint(kind, odd, with_ws):
    """call 1 with k = 0, 1 and 2"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    for k, beta, ell, batch in ((0, 4, 2, 3), (1, 5, 3, 3), (2, 6, 2, 1)):
        rng = np.random.default_rng(seed("fp-native-cmux", kind, k, odd))
        kr = tnc.selectors(torch, plan, rng, k, ell)
        torch.cuda.synchronize()
        c0, c1 = (tnc.words_with_zeros(rng, plan, batch * (k + 1)) for _ in range(2))
        wsb = plan.glwe_cmux_workspace_bytes(k, ell, batch)
        assert wsb % 16 == 0 and wsb > 0
        ar = word_arena(plan, 111 + k, odd)
        ar.take("glwe_out", c0.size, written=True, guard=MIN_GUARD_POLYS * pe)
        ar.take("glwe0", c0)
        ar.take("glwe1", c1)
        ar.build()
        pa = plane_arena(plan, kr, wsb if with_ws else 0, 121 + k, odd)
        plan.glwe_cmux_batch(ar["glwe_out"], ar["glwe0"], ar["glwe1"], [pa["sel%d" % i] for i in range(plan.NPRIMES)], k, beta, ell,
                             workspace=pa["ws"] if with_ws else None)
        got = ar.check()["glwe_out"]
        pa.check()
        want = tnc.run_cmux(torch, plan, "device", c0, c1, kr, k, beta, ell)
        assert got.any() and np.array_equal(got, want), (kind, k, odd, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_cmux_tree_footprint(kind, odd, with_ws):
    """call 2 with M = 1 (the trivial ciphertext, no selector, no workspace), 2 (the leaf stage writes glwe_out), 4 (both kinds of
    stage) and 16 (both buffers filled twice); k = 1, where the later stages need the larger digits part, and k = 0, where the leaf stage
    does"""
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pe = per(plan)
    beta, ell, batch = 5, 2, 3
    for k in (1, 0):
        rng = np.random.default_rng(seed("fp-native-cmux-tree", kind, odd, k))
        for m in (1, 2, 4, 16):
            depth = m.bit_length() - 1
            kr = tnc.selectors(torch, plan, rng, k, ell, depth) if depth else None
            torch.cuda.synchronize()
            lut = tnc.words_with_zeros(rng, plan, batch * m)
            wsb = plan.cmux_tree_workspace_bytes(m, k, ell, batch)
            assert wsb % 16 == 0 and (wsb == 0) == (m == 1)
            ar = word_arena(plan, 131 + m, odd)
            ar.take("glwe_out", batch * (k + 1) * pe, written=True, guard=MIN_GUARD_POLYS * pe)
            ar.take("lut_in", lut)
            ar.build()
            pa = plane_arena(plan, kr, wsb if with_ws else 0, 141 + m, odd)
            plan.cmux_tree_batch(ar["glwe_out"], ar["lut_in"], [pa["sel%d" % i] for i in range(plan.NPRIMES)] if depth else None, m, k, beta, ell,
                                 workspace=pa["ws"] if with_ws and wsb else None)
            got = ar.check()["glwe_out"]
            if pa is not None:
                pa.check()
            want = tnc.run_tree(torch, plan, "device", lut, kr, m, k, beta, ell, batch)
            assert got.any() and np.array_equal(got, want), (kind, m, k, odd, with_ws)
