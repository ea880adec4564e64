"""tests/test_gpu_footprint_cmux.py continued for include/cntt_prime_cbs.h.  Every operand -- the LWE input, the two keys, the output, the
caller's workspace -- is an exact-size slice of ONE guard-band arena (tests/guard_arena.py) at the word's own alignment (16-byte aligned,
and one word past a 16-byte boundary), the workspace exactly cntt_prime*_circuit_bootstrap_workspace_bytes long and 16-byte aligned.  Each
case asserts the written slice bit-exact against the call on plain tensors (which tests/test_gpu_prime_cbs.py pins to the model and the
public calls) and check() on the arena: every band word, and the input and the keys, byte for byte what they were.

What is live at these shapes.  At n = 16 (64-bit words) and n = 32 (32-bit words) a key row of (k + 1) n words is 16 or 24 vectors of 16
bytes, so 232 of the 256 threads of a product workgroup own no column and only the bound keeps them from reaching behind the key and the
slab sums; 3 * Lc elements are a ragged tile whose absent elements take the digit 0 and store nothing; with Lk = 3 at k = 2 the rows
make two slabs, the last one short, and the slab sums -- the LAST part of the workspace -- end at the end of the caller's buffer."""
import numpy as np
import pytest

import test_gpu_prime_automorphism as tga
import test_gpu_prime_cbs as tcb
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint_automorphism import CASES, IDS
from test_gpu_prime_pbs import dt, host, make_plan, min_n

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("with_ws", [False, True], ids=["null-workspace", "caller-workspace"])
@pytest.mark.parametrize("p,odd,device", CASES, ids=IDS)
def test_circuit_bootstrap_footprint(p, odd, device, with_ws):
    torch = tga._torch()
    isz = np.dtype(dt(p)).itemsize
    n = min_n(p)
    plan = make_plan(p, n)
    for k, L, batch, Lc, Lk in ((1, 3, 3, 2, 1), (2, 2, 3, 1, 3)):
        gad = tcb.gadgets(p, Lk, Lc)
        rng = np.random.default_rng(tga.seed("fp-cbs", p, k, odd))
        lwe, bsk_t, fk_t = tcb.random_case(torch, plan, p, rng, L, k, gad, batch)
        torch.cuda.synchronize()
        wsb = plan.circuit_bootstrap_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch)
        assert wsb % isz == 0 and wsb > 0
        ar = GuardArena(dt(p), device, 111 + k, odd).take("out", batch * tcb.sizes(k, n, Lk, Lc)[2] * n, written=True, guard=MIN_GUARD_POLYS * n)
        ar.take("lwe_in", lwe).take("fpksk_ntt", host(fk_t, dt(p)))
        if L:
            ar.take("bsk_ntt", host(bsk_t, dt(p)))
        if with_ws:
            ar.take("ws", wsb // isz, written=True, guard=MIN_GUARD_POLYS * n, aligned=True)
        ar.build()
        plan.circuit_bootstrap_batch(ar["out"], ar["lwe_in"], ar["bsk_ntt"] if L else None, ar["fpksk_ntt"], L, k, *gad,
                                     workspace=ar["ws"] if with_ws else None)
        got = ar.check()["out"]
        want = tcb.run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
        assert got.any() and np.array_equal(got, want), (p, k, L, odd, device, with_ws)
