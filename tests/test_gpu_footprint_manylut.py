"""tests/test_gpu_footprint_cbs.py continued for include/cntt_prime_manylut.h.  Every operand of the four calls is an exact-size slice of
ONE guard-band arena (tests/guard_arena.py) at the word's own alignment (16-byte aligned, and one word past a 16-byte boundary), the
workspace exactly cntt_prime*_pbs_workspace_bytes / cntt_prime*_circuit_bootstrap_manylut_workspace_bytes long and 16-byte aligned.  Each
case asserts the written slice bit-exact against the call on plain tensors (which tests/test_gpu_prime_manylut.py pins to the model and
the public calls) and check() on the arena: every band word, and every input, byte for byte what it was.

What is live at these shapes.  A row of the extraction has k n + 1 words, so in every arena its 16-byte stores start at the word's
alignment only, and in the odd arena so do the 16-byte loads of the window; count = 9 leaves a chunk of one row whose seven absent rows
store nothing, and the last row ends at the end of the operand.  In the circuit bootstrap the shared table is one ciphertext however
large the batch, 3 x 3 elements are a ragged tile of the product, and the slab sums -- the LAST part of the workspace -- end at the end
of the caller's buffer."""
import numpy as np
import pytest

import test_gpu_prime_automorphism as tga
import test_gpu_prime_cbs as tcb
import test_gpu_prime_manylut as tml
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint_automorphism import CASES, IDS
from test_gpu_prime_pbs import dt, host, make_plan, min_n, random_words

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_modswitch_and_extraction_footprint(p, odd, device):
    torch = tga._torch()
    n = min_n(p)
    plan = make_plan(p, n)
    rng = np.random.default_rng(tga.seed("fp-ml-ext", p, odd))
    for k, L, batch, t, count in ((1, 3, 3, 2, 9), (2, 5, 9, 1, n), (0, 0, 3, 0, 2)):
        lwe = random_words(rng, p, batch * (L + 1))
        glwe = random_words(rng, p, batch * (k + 1) * n)
        ar = GuardArena(dt(p), device, 131 + k, odd).take("ext", batch * count * (k * n + 1), written=True, guard=MIN_GUARD_POLYS * n)
        ar.take("glwe", glwe).take("lwe", lwe).build()
        plan.sample_extract_many_batch(ar["ext"], ar["glwe"], k, count)
        got = ar.check()["ext"]
        want = tml.dev(torch, tcb.poison(p, got.size))
        plan.sample_extract_many_batch(want, tml.dev(torch, glwe), k, count)
        torch.cuda.synchronize()
        assert np.array_equal(got, host(want, dt(p))), (p, k, count, odd, device)
        # rot_t is uint32: an arena of its own word type, the LWE input beside it as bytes of that type
        ra = GuardArena(np.uint32, device, 137 + k, False).take("rot_t", batch * (L + 1), written=True)
        ra.take("lwe", lwe.view(np.uint32), aligned=True).build()
        lwe_slice = ra["lwe"].view(torch.int64 if dt(p) == np.uint64 else torch.int32) if device else ra["lwe"].view(dt(p))
        plan.lwe_modswitch_manylut_batch(ra["rot_t"], lwe_slice, L, t)
        got_r = ra.check()["rot_t"]
        want_r = torch.full((batch * (L + 1),), -1, dtype=torch.int32, device="cuda")
        plan.lwe_modswitch_manylut_batch(want_r, tml.dev(torch, lwe), L, t)
        torch.cuda.synchronize()
        assert np.array_equal(got_r, host(want_r, np.uint32)), (p, L, batch, t, device)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_bootstrap_manylut_footprint(p, odd, device, with_ws):
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    plan = make_plan(p, n)
    gad = (tml.wbits(p) // 4, 4)
    for k, L, batch, t, count in ((1, 3, 3, 2, 3), (2, 2, 3, 4, 9)):
        rng = np.random.default_rng(tga.seed("fp-ml-boot", p, k, odd))
        lwe, lut = random_words(rng, p, batch * (L + 1)), random_words(rng, p, (k + 1) * n)
        bsk = random_words(rng, p, L * (k + 1) * gad[1] * (k + 1) * n)
        wsb = plan.pbs_workspace_bytes(L, k, gad[1], batch)
        assert wsb % isz == 0 and wsb > 0
        ar = GuardArena(dt(p), device, 141 + k, odd).take("out", batch * count * (k * n + 1), written=True, guard=MIN_GUARD_POLYS * n)
        ar.take("lwe_in", lwe).take("lut", lut).take("bsk_ntt", bsk)
        if with_ws:
            ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
        ar.build()
        plan.bootstrap_manylut_batch(ar["out"], ar["lwe_in"], ar["lut"], ar["bsk_ntt"], L, k, *gad, t, count, workspace=ar["ws"] if with_ws else None)
        got = ar.check()["out"]
        want = tml.run_boot(torch, plan, p, "device", lwe, lut, tml.dev(torch, bsk), L, k, gad, t, count)
        assert got.any() and np.array_equal(got, want), (p, k, L, odd, device, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_circuit_bootstrap_manylut_footprint(p, odd, device, with_ws):
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    plan = make_plan(p, n)
    for k, L, batch, Lc, Lk, t in ((1, 3, 3, 3, 1, 2), (2, 2, 3, 2, 3, 1)):
        gad = tml.gadgets(p, Lk, Lc)
        rng = np.random.default_rng(tga.seed("fp-ml-cbs", p, k, odd))
        lwe, bsk_t, fk_t = tml.random_case(torch, plan, p, rng, L, k, gad, batch)
        torch.cuda.synchronize()
        wsb = plan.circuit_bootstrap_manylut_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch)
        assert wsb % isz == 0 and wsb > 0
        ar = GuardArena(dt(p), device, 151 + k, odd).take("out", batch * tcb.sizes(k, n, Lk, Lc)[2] * n, written=True, guard=MIN_GUARD_POLYS * n)
        ar.take("lwe_in", lwe).take("fpksk_ntt", host(fk_t, dt(p))).take("bsk_ntt", host(bsk_t, dt(p)))
        if with_ws:
            ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
        ar.build()
        plan.circuit_bootstrap_manylut_batch(ar["out"], ar["lwe_in"], ar["bsk_ntt"], ar["fpksk_ntt"], L, k, *gad, t,
                                             workspace=ar["ws"] if with_ws else None)
        got = ar.check()["out"]
        want = tml.run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t)
        assert got.any() and np.array_equal(got, want), (p, k, L, odd, device, with_ws)
