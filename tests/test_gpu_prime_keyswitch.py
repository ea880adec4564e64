"""The prime plans' LWE keyswitch and keyswitch + bootstrap (include/cntt_prime_keyswitch.h) on the GPU, bit-exact: the kernel against the
plain-int model of tests/test_prime_keyswitch_abi.py on shapes that cross every edge of its tile and of its chunk rule, on every arithmetic
class of prime, at the accumulator's worst cases, on encrypted messages, and the combined call against the two public calls."""
import os
import random
import subprocess

import numpy as np
import pytest

from concrete_ntt_amd import prime32, prime64
from test_gpu_prime_pbs import P31, PG64, _torch, dev, dt, host, is64, make_plan, min_n, random_words, seed, zeros
from test_prime_keyswitch_abi import chunk_words, model_keyswitch, noiseless_ksk, phase
from test_prime_pbs_model import P30, P32, P50, P62, P63, PM64, edge_words, lift, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# prime_keyswitch.hpp: a workgroup owns 4 * TB batch elements x 64 * TC columns, TB x TC = 8 x 2 for both word types
TILE_B, TILE_C = 32, 128


def words_with_edges(rng, p, count, beta, ell, dtype):
    a = rng.integers(0, p, size=count, dtype=np.uint64).astype(dtype)
    edges = edge_words(p, beta, ell)
    for j, e in enumerate(edges):
        if 3 * j < count:
            a[3 * j] = e
    return a


def run_case(p, beta, ell, lin, lout, batch, pad=0, where="device", lwe=None, ksk=None, tag="", bits=None):
    """bits: the plan's word width (None: 64 for p >= 2^32, else 32)"""
    torch = _torch()
    bits = bits or (64 if is64(p) else 32)
    plan = (prime64 if bits == 64 else prime32).Plan.try_new(16 if bits == 64 else 32, p)
    assert plan is not None, (p, bits)
    dt = lambda _p: np.uint64 if bits == 64 else np.uint32
    random_words = lambda g, q, count: g.integers(0, q, size=count, dtype=np.uint64).astype(dt(q))
    rng = np.random.default_rng(seed("pks", p, beta, ell, lin, lout, batch, pad, tag))
    stride = lout + 1 + pad
    if lwe is None:
        lwe = words_with_edges(rng, p, batch * (lin + 1), beta, ell, dt(p))
    if ksk is None:
        ksk = random_words(rng, p, max(lin * ell * stride - pad, 0))       # the last row ends after its lout + 1 words
    want = np.array(model_keyswitch(lwe.tolist(), ksk.tolist(), p, lin, lout, stride, beta, ell, batch), dtype=dt(p))
    if where == "host":
        out = np.full(batch * (lout + 1), 7, dtype=dt(p))
        plan.keyswitch_batch(out, lwe, ksk if lin else np.zeros(0, dtype=dt(p)), lin, lout, beta, ell, row_stride=stride)
        got = out
    else:
        out = dev(torch, np.full(batch * (lout + 1), 7, dtype=dt(p)))
        plan.keyswitch_batch(out, dev(torch, lwe), dev(torch, ksk), lin, lout, beta, ell, row_stride=stride)
        torch.cuda.synchronize()
        got = host(out, dt(p))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (p, beta, ell, lin, lout, batch, pad, where, bad[:8], got[bad[:4]], want[bad[:4]])


# -- 1. the tile edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P30])
@pytest.mark.parametrize("batch", [TILE_B - 1, TILE_B, TILE_B + 1])
@pytest.mark.parametrize("ncol", [TILE_C - 1, TILE_C, TILE_C + 1])
def test_tile_edges(p, batch, ncol):
    run_case(p, 4, 3, 7, ncol - 1, batch, pad=ncol % 2)


@pytest.mark.parametrize("p,where", [(P62, "device"), (PM64, "host"), (P30, "host"), (P32, "device")])
def test_body_only_output_and_host_path(p, where):
    run_case(p, 5, 2, 9, 0, 5, where=where)
    run_case(p, 5, 2, 9, 3, TILE_B + 2, pad=3, where=where)


# -- 2. the chunk rule ------------------------------------------------------------------------------------------------------------------
def lin_edges(beta, ell):
    c = chunk_words(beta, ell)
    return sorted({0, 1, max(c - 1, 0), c, c + 1, 2 * c + 3})


CHUNKS = [(P62, 3, 5), (P62, 8, 3), (PM64, 1, 64), (PM64, 31, 2), (PM64, 30, 2), (PM64, 16, 4), (P62, 31, 2), (P50, 25, 2), (P50, 26, 1),
          (P32, 8, 4), (P32, 31, 1), (P32, 30, 1), (P32, 16, 2), (P30, 3, 5), (P30, 10, 3)]


@pytest.mark.parametrize("p,beta,ell", CHUNKS)
def test_chunk_edges(p, beta, ell):
    for lin in lin_edges(beta, ell):
        run_case(p, beta, ell, lin, 4, 3, pad=lin % 2)


def test_the_chunk_rule_restated_here_covers_its_cases():
    assert chunk_words(3, 5) == 25 and 128 % 5 and chunk_words(8, 3) == 42 and 128 % 3        # levels that do not divide the chunk rows
    assert chunk_words(31, 2) == 1 and chunk_words(31, 1) == 2 and chunk_words(30, 2) == 2     # one word per chunk; the most frequent folds
    assert chunk_words(1, 64) == 2 and chunk_words(25, 2) == 64 and chunk_words(26, 1) == 64
    assert wbits(PM64) == 16 * 4 and wbits(P62) == 31 * 2 and wbits(P32) == 8 * 4              # base_log * levels = W


# -- 3. every arithmetic class of prime -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, PM64, P50, P63, PG64, 12289, 97, P30, P32, P31])
def test_primes(p):
    W = wbits(p)
    for beta, ell in [(b, l) for b, l in ((1, 1), (2, 3), (8, 3), (23, 1), (31, 2), (16, 4), (min(W, 31), 1)) if b * l <= W]:
        run_case(p, beta, ell, 11, 5, 4, pad=1, bits=32 if p in (P30, P32, P31) else 64)


def test_12289_on_a_32_bit_plan():
    run_case(12289, 3, 4, 11, 5, 4)
    run_case(12289, 14, 1, 11, 5, 4)


# -- 4. the accumulator's worst cases ----------------------------------------------------------------------------------------------------
def extreme_words(p, beta, ell):
    """The pattern `u = B - 1 below the top and u = B at the top` is no canonical word: the top digit +B/2 stands for 2^(W-1), and a lift
    is at most (p - 1) / 2 < 2^(W-1), so it is reached only by rounding up from words whose lower digits are then small.  What can be
    reached: the largest and the smallest lift (top digit at +B/2 resp. -B/2 where the rounding reaches it), and the words whose every
    digit is B/2 - 1 resp. -B/2 (clamped to the lift's range): staged numbers B - 1 resp. 0 on every level."""
    W, B = wbits(p), 1 << beta
    h = (p - 1) // 2
    hi_all = sum((B // 2 - 1) << (W - beta * l) for l in range(1, ell + 1))
    lo_all = -sum((B // 2) << (W - beta * l) for l in range(1, ell + 1))
    return [h, h + 1, min(hi_all, h) % p, max(lo_all, -h) % p]


# (25, 2) and (26, 2): either side of the switch in prime_ks_chunk_rows, where a chunk's 128 resp. 64 rows are exactly what a lazy sum holds
@pytest.mark.parametrize("p,beta,ell,lin", [(PM64, 31, 2, 9), (PM64, 16, 4, 100), (PM64, 1, 64, 7), (P32, 31, 1, 9), (P32, 8, 4, 100),
                                            (PM64, 25, 2, 200), (PM64, 26, 2, 100)])
def test_worst_case_accumulators(p, beta, ell, lin):
    lout, batch = 1, 4
    ksk = np.full(lin * ell * (lout + 1), p - 1, dtype=dt(p))
    ext = extreme_words(p, beta, ell)
    assert lin > 3 * chunk_words(beta, ell)        # several folds
    for shift in (0, 1):                           # the maxima, then the mirrored case first
        lwe = np.array([ext[(b + shift) % 4] for b in range(batch) for _ in range(lin + 1)], dtype=dt(p))
        run_case(p, beta, ell, lin, lout, batch, lwe=lwe, ksk=ksk, tag="worst%d" % shift)


# -- 5. encrypted messages -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,beta,ell", [(PM64, 4, 5), (P62, 3, 6), (P32, 4, 4)])
def test_keyswitch_of_encrypted_messages(p, beta, ell):
    torch = _torch()
    rng = random.Random("pksenc/%d" % p)
    W, B = wbits(p), 1 << beta
    s = W - beta * ell
    lin, lout, batch, noise = 48, 20, 8, 1 << (W - 30)
    s_in, s_out = [rng.randrange(2) for _ in range(lin)], [rng.randrange(2) for _ in range(lout)]
    ksk = noiseless_ksk(rng, p, s_in, s_out, beta, ell, lout + 1, noise=noise)
    delta = p // 16
    msgs = [rng.randrange(16) for _ in range(batch)]
    lwe = []
    for m in msgs:
        mask = [rng.randrange(p) for _ in range(lin)]
        lwe += mask + [(sum(a * k for a, k in zip(mask, s_in)) + m * delta + rng.randint(-noise, noise)) % p]
    plan = make_plan(p, min_n(p))
    out = zeros(torch, p, batch * (lout + 1))
    plan.keyswitch_batch(out, dev(torch, np.array(lwe, dtype=dt(p))), dev(torch, np.array(ksk, dtype=dt(p))), lin, lout, beta, ell)
    torch.cuda.synchronize()
    got = host(out, dt(p)).tolist()
    # |phase_out - phase_in| <= sum_i |s_in[i]| 2^(s-1)  (rounding)  +  sum_{i,l} |d_l| noise  (the key rows' noise), |d_l| <= B/2
    bound = lin * ((1 << s) >> 1) + lin * ell * (B // 2) * noise
    assert bound + noise < delta // 2
    for b, m in enumerate(msgs):
        ph_in = phase(lwe[b * (lin + 1):(b + 1) * (lin + 1)], s_in, p)
        ph_out = phase(got[b * (lout + 1):(b + 1) * (lout + 1)], s_out, p)
        assert abs(lift((ph_out - ph_in) % p, p)) <= bound, (p, b)
        assert round(lift(ph_out, p) / delta) % 16 == m


# -- 6. the combined call ----------------------------------------------------------------------------------------------------------------------
def combined_inputs(torch, p, n, L, k, ks_beta, ks_ell, ell, batch, pad=0):
    rng = np.random.default_rng(seed("pkscomb", p, n))
    big = k * n
    return dict(lwe=dev(torch, random_words(rng, p, batch * (big + 1))), ksk=dev(torch, random_words(rng, p, big * ks_ell * (L + 1 + pad))),
                lut=dev(torch, random_words(rng, p, (k + 1) * n)), bsk=dev(torch, random_words(rng, p, L * (k + 1) * ell * (k + 1) * n)))


@pytest.mark.parametrize("p", [P62, PM64])
@pytest.mark.parametrize("n", [64, 1024])
def test_combined_call_equals_the_two_calls_and_chains(p, n):
    torch = _torch()
    plan = make_plan(p, n)
    L, k, beta, ell, ks_beta, ks_ell, batch, pad = 4, 1, 7, 3, 4, 3, 3, 1
    big, stride = k * n, L + 1 + pad
    a = combined_inputs(torch, p, n, L, k, ks_beta, ks_ell, ell, batch, pad)
    ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=torch.uint8, device="cuda")
    # four separate calls: two rounds of keyswitch, bootstrap
    cur = a["lwe"]
    rounds = []
    for _ in range(2):
        mid, nxt = zeros(torch, p, batch * (L + 1)), zeros(torch, p, batch * (big + 1))
        plan.keyswitch_batch(mid, cur, a["ksk"], big, L, ks_beta, ks_ell, row_stride=stride)
        plan.bootstrap_batch(nxt, mid, a["lut"], a["bsk"], L, k, beta, ell)
        rounds.append(nxt)
        cur = nxt
    for w in (None, ws):                            # NULL workspace and caller workspace: the same words
        one, two = zeros(torch, p, batch * (big + 1)), zeros(torch, p, batch * (big + 1))
        plan.keyswitch_bootstrap_batch(one, a["lwe"], a["ksk"], ks_beta, ks_ell, a["lut"], a["bsk"], L, k, beta, ell, workspace=w, row_stride=stride)
        plan.keyswitch_bootstrap_batch(two, one, a["ksk"], ks_beta, ks_ell, a["lut"], a["bsk"], L, k, beta, ell, workspace=w, row_stride=stride)
        torch.cuda.synchronize()
        assert torch.equal(one, rounds[0]) and torch.equal(two, rounds[1]), (p, n, w is None)
    assert rounds[0].any() and rounds[1].any()
    if n == 64:                                     # the host path, with a host-side workspace (checked, then ignored) and without
        h = {name: host(t, dt(p)).copy() for name, t in a.items()}
        for w in (None, np.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8)):
            one = np.zeros(batch * (big + 1), dtype=dt(p))
            plan.keyswitch_bootstrap_batch(one, h["lwe"], h["ksk"], ks_beta, ks_ell, h["lut"], h["bsk"], L, k, beta, ell, workspace=w, row_stride=stride)
            assert np.array_equal(one, host(rounds[0], dt(p))), (p, n, "host", w is None)


def test_graph_capture_of_the_combined_call_with_a_caller_workspace():
    torch = _torch()
    p, n, L, k, beta, ell, ks_beta, ks_ell, batch = P62, 1024, 6, 1, 8, 3, 4, 3, 5
    plan = make_plan(p, n)
    a = combined_inputs(torch, p, n, L, k, ks_beta, ks_ell, ell, batch)
    ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=torch.uint8, device="cuda")
    eager = zeros(torch, p, batch * (k * n + 1))
    plan.keyswitch_bootstrap_batch(eager, a["lwe"], a["ksk"], ks_beta, ks_ell, a["lut"], a["bsk"], L, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # one stream, a linear chain of kernels: no allocation with a caller workspace at this size
        plan.keyswitch_bootstrap_batch(out, a["lwe"], a["ksk"], ks_beta, ks_ell, a["lut"], a["bsk"], L, k, beta, ell, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(first, eager) and torch.equal(out, eager)


# -- 7. the C example -----------------------------------------------------------------------------------------------------------------------
def test_ks_pbs_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "ks_pbs_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "ks_pbs_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 4 and not any("WRONG" in ln for ln in lines), r.stdout
