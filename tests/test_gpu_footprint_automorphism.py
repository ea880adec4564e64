"""tests/test_gpu_footprint.py continued for include/cntt_prime_automorphism.h: the automorphism in both domains, the Galois keyswitch
and the trace.  Every operand -- the input, the key, the output, the caller's workspace -- is an exact-size slice of ONE guard-band arena
(tests/guard_arena.py) at the word's own alignment (16-byte aligned, and one word past a 16-byte boundary), the workspace exactly
cntt_prime*_..._workspace_bytes long and 16-byte aligned.  Each case asserts the written slice bit-exact against the call on plain
tensors (which tests/test_gpu_prime_automorphism.py pins to the model and the public calls) and check() on the arena: every band word,
and the input and the key, byte for byte what they were.

What is live at these shapes.  One workgroup serves one polynomial with 16-byte loads and stores, so at n = 16 (64-bit words) and
n = 32 (32-bit words) 248 of its 256 threads own no vector and only the loop bound keeps them from storing behind the operand; the last
polynomial of the output ends where the slice ends.  The trace alternates between glwe_out and the LAST bytes of the workspace, so the
same edge sits on the end of the caller's workspace.  Bands: behind every written operand MIN_GUARD_POLYS polynomials (a whole
workgroup's stores at these sizes: 256 threads x 16 bytes is at most 32 polynomials of 128 bytes)."""
import numpy as np
import pytest

import test_gpu_prime_automorphism as tga
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_prime_pbs import dt, host, make_plan, min_n
from test_prime_pbs_model import P30, P62

pytestmark = pytest.mark.gpu

PRIMES = [(P62, "P62"), (P30, "P30")]
CASES = [(p, odd, device) for (p, _) in PRIMES for odd in (False, True) for device in (True,)] + [(P30, True, False), (P62, True, False)]
IDS = ["%s-%s-%s" % ("P62" if p == P62 else "P30", "odd" if o else "aligned", "device" if d else "host") for (p, o, d) in CASES]


def plain(torch, a, device):
    """the operand as the owning tests pass it: a plain device tensor, or the host array itself"""
    return tga.dev(torch, a) if device else a


def sizes_for(p):
    return (min_n(p), 64)


@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_automorphism_footprint(p, odd, device):
    """calls 1 and 2: out written, in read; batch 3 polynomials"""
    torch = tga._torch()
    for n in sizes_for(p):
        plan = make_plan(p, n)
        rng = np.random.default_rng(tga.seed("fp-autom", p, n, odd))
        f = tga.words_with_zeros(rng, p, 3 * n)
        for ntt in (False, True):
            call = plan.automorphism_ntt_batch if ntt else plan.automorphism_batch
            t = 2 * n - 1 if ntt else n // 2 + 1
            ar = GuardArena(dt(p), device, 31 + n, odd).take("out", 3 * n, written=True, guard=MIN_GUARD_POLYS * n).take("in", f).build()
            call(ar["out"], ar["in"], t)
            got = ar.check()["out"]
            ref = plain(torch, tga.poison(p, 3 * n), device)
            call(ref, plain(torch, f, device), t)
            want = host(ref, dt(p)) if device else ref
            assert got.any() and np.array_equal(got, want), (p, n, odd, device, ntt)


def glwe_on_arena(torch, plan, p, device, odd, seed, ct, key, ws_words, run):
    """run(out, in, key, ws) with glwe_out, glwe_in, ak_ntt and (ws_words > 0) the workspace carved from one arena -> the output words"""
    n = plan.ntt_size()
    ar = GuardArena(dt(p), device, seed, odd).take("glwe_out", ct.size, written=True, guard=MIN_GUARD_POLYS * n).take("glwe_in", ct)
    if key is not None:
        ar.take("ak_ntt", key)
    if ws_words:
        ar.take("ws", ws_words, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
    ar.build()
    run(ar["glwe_out"], ar["glwe_in"], ar["ak_ntt"] if key is not None else None, ar["ws"] if ws_words else None)
    return ar.check()["glwe_out"]


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_galois_keyswitch_footprint(p, odd, device, with_ws):
    """call 3 with k = 0 (no key, no workspace), 1 and 2; add_input on the odd dimension"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    for n in sizes_for(p):
        plan = make_plan(p, n)
        for k, beta, ell, batch in ((0, 4, 2, 3), (1, 5, 3, 3), (2, 6, 2, 1)):
            rng = np.random.default_rng(tga.seed("fp-ks", p, n, k, odd))
            kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n)
            torch.cuda.synchronize()
            ct = tga.words_with_zeros(rng, p, batch * (k + 1) * n)
            t, add = n + 1 if k else 3, k == 1
            wsb = plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch)
            assert wsb % isz == 0 and (wsb == 0) == (k == 0)
            got = glwe_on_arena(torch, plan, p, device, odd, 41 + k, ct, host(kt, dt(p)) if k else None, wsb // isz if with_ws else 0,
                                lambda o, i, a, w: plan.glwe_automorphism_keyswitch_batch(o, i, a, t, k, beta, ell, add, workspace=w))
            want = tga.run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, add, batch)
            assert got.any() and np.array_equal(got, want), (p, n, k, odd, device, with_ws)


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_trace_footprint(p, odd, device, with_ws):
    """call 4 with an even and an odd number of steps (the last step lands in glwe_out either way), and no step at all"""
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    plan = make_plan(p, n)
    k, beta, ell, batch = 1, 5, 2, 3
    rng = np.random.default_rng(tga.seed("fp-trace", p, odd))
    kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=3)
    torch.cuda.synchronize()
    ct = tga.words_with_zeros(rng, p, batch * (k + 1) * n)
    wsb = plan.glwe_trace_workspace_bytes(k, ell, batch)
    assert wsb % isz == 0
    per = k * ell * (k + 1) * n
    for steps in (0, 2, 3):
        keys = host(kt, dt(p))[:steps * per] if steps else None
        got = glwe_on_arena(torch, plan, p, device, odd, 51 + steps, ct, keys, wsb // isz if with_ws else 0,
                            lambda o, i, a, w: plan.glwe_trace_batch(o, i, a, steps, k, beta, ell, workspace=w))
        want = tga.steps_of_call_3(torch, plan, p, ct, kt, steps, k, beta, ell, batch)
        assert got.any() and np.array_equal(got, want), (p, steps, odd, device, with_ws)
