"""tests/test_gpu_footprint_native_cbs.py continued for include/cntt_manylut.h on a 32-, a 64- and a 128-bit native kind.  The words are
exact-size slices of a guard-band arena (tests/guard_arena.py, as it is) of the word type; rot_t, the output planes, the planes of the
bootstrapping key and the caller's workspace are slices of a uint32 arena; every output and the workspace written, everything else read
only.  The 32- and 64-bit kinds run 16-byte aligned and again one word past a 16-byte boundary (fpksk and the workspace stay 16-byte
aligned, as the header wants them); a 128-bit word promises 16 bytes itself, so that kind runs aligned only.  The workspace is exactly
cntt_native_pbs_workspace_bytes / cntt_native_circuit_bootstrap_manylut_workspace_bytes long or absent.  Each case asserts the written
slices bit-exact against the call on plain tensors (which tests/test_gpu_native_manylut.py pins to the model and the public calls) and
check()s the arenas: every band word and every input byte for byte what it was.  The modulus switch, the extraction and the bootstrap run
on the device path and on the host path, the circuit bootstrap on the device path, as its neighbour.

What is live at these shapes.  A row of the extraction has k n + 1 words, so in every arena its 16-byte stores start at the word's
alignment only, and in the odd arena so do the 16-byte loads of the window; count = 9 leaves a chunk of one row whose seven absent rows
store nothing, and the last row ends at the end of the operand.  In the circuit bootstrap the shared table is one ciphertext however
large the batch, 3 x 3 elements are a ragged tile of the product, and the selector words -- the LAST part of the workspace -- end at the
end of the caller's buffer."""
import numpy as np
import pytest

import test_gpu_native_cbs as tcb
import test_gpu_native_manylut as tml
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint_native_cbs import CASES, IDS
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, per, random_words, seed, wbits

pytestmark = pytest.mark.gpu

N = 32


def word_arena(plan, device, stamp, odd):
    return GuardArena(np.uint64 if plan.WORD == 16 else plan.word_dtype, device, stamp, odd)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_modswitch_and_extraction_footprint(kind, odd, device):
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pw = 2 if plan.WORD == 16 else 1
    rng = np.random.default_rng(seed("fp-nml-ext", kind, odd))
    for k, L, batch, t, count in ((1, 3, 3, 2, 9), (2, 5, 9, 1, N), (0, 0, 3, 0, 2)):
        lwe = random_words(rng, plan, batch * (L + 1))
        glwe = random_words(rng, plan, batch * (k + 1) * N)
        ar = word_arena(plan, device, 131 + k, odd).take("ext", batch * count * (k * N + 1) * pw, written=True, guard=MIN_GUARD_POLYS * N)
        ar.take("glwe", glwe).take("lwe", lwe).build()
        plan.sample_extract_many_batch(ar["ext"], ar["glwe"], k, count)
        ra = GuardArena(np.uint32, device, 137 + k, False).take("rot_t", batch * (L + 1), written=True)
        ra.build()
        plan.lwe_modswitch_manylut_batch(ra["rot_t"], ar["lwe"], L, t)
        got = ar.check()["ext"]
        got_r = ra.check()["rot_t"]
        want = dev(torch, np.full(got.size, 0x5A, dtype=got.dtype))
        plan.sample_extract_many_batch(want, dev(torch, glwe), k, count)
        want_r = torch.full((batch * (L + 1),), -1, dtype=torch.int32, device="cuda")
        plan.lwe_modswitch_manylut_batch(want_r, dev(torch, lwe), L, t)
        torch.cuda.synchronize()
        assert np.array_equal(got, host(want, got.dtype)), (kind, k, count, odd, device)
        assert np.array_equal(got_r, host(want_r, np.uint32)), (kind, L, batch, t, device)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_bootstrap_manylut_footprint(kind, odd, device, with_ws):
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    pw = 2 if plan.WORD == 16 else 1
    gad = (wbits(plan) // 4, 4)
    for k, L, batch, t, count in ((1, 3, 3, 2, 3), (2, 2, 3, 4, 9)):
        rng = np.random.default_rng(seed("fp-nml-boot", kind, k, odd))
        lwe, lut = random_words(rng, plan, batch * (L + 1)), random_words(rng, plan, (k + 1) * N)
        kr = key_planes(torch, plan, random_words(rng, plan, L * (k + 1) * gad[1] * (k + 1) * N))
        torch.cuda.synchronize()
        wsb = plan.pbs_workspace_bytes(L, k, gad[1], batch)
        assert wsb % 16 == 0 and wsb > 0
        ar = word_arena(plan, device, 141 + k, odd).take("out", batch * count * (k * N + 1) * pw, written=True, guard=MIN_GUARD_POLYS * N)
        ar.take("lwe_in", lwe).take("lut", lut).build()
        pa = GuardArena(np.uint32, device, 171 + k, odd)
        for i in range(plan.NPRIMES):
            pa.take("bsk%d" % i, host(kr[i], np.uint32))
        if with_ws:
            pa.take("ws", wsb // 4, written=True, guard=MIN_GUARD_POLYS * N, aligned=True)
        pa.build()
        plan.bootstrap_manylut_batch(ar["out"], ar["lwe_in"], ar["lut"], [pa["bsk%d" % i] for i in range(plan.NPRIMES)], L, k, *gad, t, count,
                                     workspace=pa["ws"] if with_ws else None)
        got = ar.check()["out"]
        pa.check()
        want = tml.run_boot(torch, plan, dev(torch, lwe), dev(torch, lut), kr, L, k, gad, t, count, batch)
        assert got.any() and np.array_equal(got, host(want, got.dtype)), (kind, k, L, odd, device, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("kind,odd", CASES, ids=IDS)
def test_circuit_bootstrap_manylut_footprint(kind, odd, with_ws):
    torch = _torch()
    plan = KINDS[kind].try_new(N)
    assert per(plan) == N * (2 if plan.WORD == 16 else 1)
    for k, L, batch, Lc, Lk, t in ((1, 3, 3, 3, 1, 2), (2, 2, 3, 2, 3, 1), (0, 0, 3, 2, 1, 1)):
        gad = (wbits(plan) // 4, 4, min(31, wbits(plan) // Lk), Lk, 5, Lc)
        pb, pl, kb, kl, cb, cl = gad
        rng = np.random.default_rng(seed("fp-nml-cbs", kind, k, odd))
        lwe, bsk_planes, fk = tcb.random_case(torch, plan, rng, L, k, gad, batch)
        torch.cuda.synchronize()
        wsb = plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pl, kl, cl, batch)
        count = batch * tcb.sizes(k, N, kl, cl)[2] * N
        assert wsb % 16 == 0 and wsb > 0
        ar = word_arena(plan, True, 151 + k, odd)
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
        plan.circuit_bootstrap_manylut_batch([pa["out%d" % i] for i in range(plan.NPRIMES)], ar["lwe_in"],
                                             [pa["bsk%d" % i] for i in range(plan.NPRIMES)] if L else None, ar["fpksk"], L, k, pb, pl, kb, kl, cb, cl,
                                             t, workspace=pa["ws"] if with_ws else None)
        ar.check()
        got = pa.check()
        want = tml.run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t)
        assert all(np.array_equal(got["out%d" % i], want[i]) for i in range(plan.NPRIMES)), (kind, k, odd, with_ws)
        assert L == 0 or any(w_.any() for w_ in want), (kind, k)      # (L = 0, k = 0: three bits 0 are three zero selectors)
