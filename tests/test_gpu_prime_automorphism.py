"""The ring automorphism, the Galois keyswitch and the trace of the prime plans (include/cntt_prime_automorphism.h) on the MI355X.
Bit-exact throughout, no tolerance anywhere: calls 1 and 2 against the plain-int model of tests/prime_automorphism_model.py (which
tests/test_prime_automorphism_model.py pins to the CPU oracle's slot order) and against each other through the transforms; call 3
against the sequence of public calls the header states for every prime class (the strict-range primes whose Barrett product wraps
included) and against the big-integer model outside that caveat; call 4 against `steps` calls of 3; both settings of the "autom_lds"
switch; a walk that makes a second, ragged trip; graph capture; encrypted messages through a full trace with noisy keys; the C
example.  The one functional test states its derived noise bound in its docstring."""
import os
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from prime_automorphism_model import LDS_BYTES, autom_gather_np, model_autoks_batch, ntt_permutation, trace_exponents
from test_gpu_prime_pack import first_difference, negacyclic_matrix, tdtype, times_binary
from test_gpu_prime_pbs import ALL, EXACT, _torch, dev, dt, host, is64, key_ntt, make_plan, min_n, random_words, seed
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5A5A5A5A5A5A5A5


def exponents(rng, n, extra=3):
    """the fixed exponents of the issue and a few seeded random odd ones"""
    return sorted({1, 3, 5, n + 1, n // 2 + 1, 2 * n - 1} | {2 * int(rng.integers(0, n)) + 1 for _ in range(extra)})


def poison(p, count):
    return np.full(count, POISON & (2 ** (8 * np.dtype(dt(p)).itemsize) - 1), dtype=dt(p))


def words_with_zeros(rng, p, count):
    w = random_words(rng, p, count)
    w[::7] = 0                                        # zeros stay zero under the sign
    w[1::11] = dt(p)(p - 1)
    return w


# -- 1. calls 1 and 2 against the model ----------------------------------------------------------------------------------------------------
def sizes(p):
    """n = 16 (64-bit words only), 32, 64, 1024; on 64-bit words also 8192 (64 KiB: the largest staged polynomial) and 16384 (past the
    LDS limit: the global gather)"""
    return ([16] if is64(p) else []) + [32, 64, 1024] + ([8192, 16384] if is64(p) else [])


@pytest.mark.parametrize("p", [P62, PM64, P30, P32])
def test_automorphism_matches_model_in_both_domains(p):
    torch = _torch()
    for n in sizes(p):
        assert (n * np.dtype(dt(p)).itemsize > LDS_BYTES) == (n == 16384)
        plan = make_plan(p, n)
        rng = np.random.default_rng(seed("autom", p, n))
        for batch in (1, 3) if n <= 1024 else (2,):
            f = words_with_zeros(rng, p, batch * n)
            ft = dev(torch, f)
            for t in exponents(rng, n, 2 if n > 1024 else 3):
                out, out_ntt = dev(torch, poison(p, batch * n)), dev(torch, poison(p, batch * n))
                plan.automorphism_batch(out, ft, t)
                plan.automorphism_ntt_batch(out_ntt, ft, t)
                torch.cuda.synchronize()
                want = autom_gather_np(f.reshape(batch, n), t, p).reshape(-1)
                assert np.array_equal(host(out, dt(p)), want), (p, n, batch, t, first_difference(host(out, dt(p)), want))
                want = f.reshape(batch, n)[:, ntt_permutation(t, n)].reshape(-1)
                assert np.array_equal(host(out_ntt, dt(p)), want), (p, n, batch, t, "ntt", first_difference(host(out_ntt, dt(p)), want))
            assert np.array_equal(host(ft, dt(p)), f)


@pytest.mark.parametrize("p", [P62, P30])
def test_automorphism_on_the_host_path(p):
    n, batch = 64, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("autom-host", p))
    f = words_with_zeros(rng, p, batch * n)
    for t in (3, n + 1, 2 * n - 1):
        out, out_ntt = poison(p, batch * n), poison(p, batch * n)
        plan.automorphism_batch(out, f, t)
        plan.automorphism_ntt_batch(out_ntt, f, t)
        assert np.array_equal(out, autom_gather_np(f.reshape(batch, n), t, p).reshape(-1)), (p, t)
        assert np.array_equal(out_ntt, f.reshape(batch, n)[:, ntt_permutation(t, n)].reshape(-1)), (p, t)


# -- 2. the two domains agree through the transforms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", [(P62, 16), (PM64, 1024), (P30, 32), (P32, 1024), (P62, 16384)])
def test_ntt_domain_automorphism_is_the_coefficient_one(p, n):
    """inv(automorphism_ntt(fwd f)) n^-1 == automorphism(f) on the device"""
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("domains", p, n))
    batch = 2
    f = random_words(rng, p, batch * n)
    for t in exponents(rng, n, 2):
        fhat = dev(torch, f)
        plan.fwd_batch(fhat)
        g = torch.zeros_like(fhat)
        plan.automorphism_ntt_batch(g, fhat, t)
        plan.inv_batch(g)
        plan.normalize_batch(g)
        direct = torch.zeros_like(fhat)
        plan.automorphism_batch(direct, dev(torch, f), t)
        torch.cuda.synchronize()
        assert direct.any() and torch.equal(g, direct), (p, n, t)


# -- 3. the Galois keyswitch ---------------------------------------------------------------------------------------------------------------
def run_autoks(torch, plan, p, where, ct, kt, t, k, beta, ell, add, batch, with_ws=False):
    """call 3 on word arrays (ciphertexts; the key as the NTT-domain device tensor, or None) -> the output array, poisoned before"""
    out = poison(p, ct.size)
    nws = plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.glwe_automorphism_keyswitch_batch(out, ct, None if kt is None else host(kt, dt(p)).copy(), t, k, beta, ell, add, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.glwe_automorphism_keyswitch_batch(out_t, dev(torch, ct), kt, t, k, beta, ell, add, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def addp(a, b, p):
    s = a.astype(object) + b.astype(object)
    return np.where(s >= p, s - p, s).astype(a.dtype)


def compose(torch, plan, p, ct, kt, t, k, beta, ell, add, batch):
    """The header's sequence of public calls: the prefill (the body permuted by the numpy model), automorphism_batch on the mask
    polynomials, gadget_decompose_batch(plain), the digits negated mod p on the host, external_product_batch(accumulate=True)."""
    n = plan.ntt_size()
    c = ct.reshape(batch, k + 1, n)
    out = np.zeros_like(c)
    out[:, k] = autom_gather_np(c[:, k], t, p)
    if add:
        out = addp(out, c, p)
    out_t = dev(torch, out.reshape(-1))
    if k:
        masks = dev(torch, c[:, :k].reshape(-1))
        rot = torch.zeros_like(masks)
        plan.automorphism_batch(rot, masks, t)
        terms = torch.zeros(batch * k * ell * n, dtype=tdtype(torch, p), device="cuda")
        plan.gadget_decompose_batch(terms, rot, beta, ell, mode="plain")
        torch.cuda.synchronize()
        d = host(terms, dt(p))
        plan.external_product_batch(out_t, dev(torch, np.where(d == 0, d, dt(p)(p) - d)), kt, k * ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def key_for(torch, plan, p, rng, k, ell, n, keys=1):
    """(coefficient-domain key words, the NTT-domain device tensor) of `keys` random keys; (empty, None) when k == 0"""
    kw = random_words(rng, p, keys * k * ell * (k + 1) * n)
    return kw, (key_ntt(torch, plan, kw) if kw.size else None)


def settings_for(p):
    """(k, base_log, levels, batch, add_input, with_ws): k 0 / 1 / 2, levels 1 / 2 / 3, batch 1 / 3, base_log * levels = W where W is the
    word width"""
    W = wbits(p)
    return [(0, 4, 2, 3, False, False), (0, 4, 2, 1, True, True), (1, min(W, 22), 1, 1, False, True), (1, W // 2, 2, 3, True, False),
            (2, 6, 3, 3, False, False), (2, 5, 3, 1, True, True), (1, 1, 3, 3, False, True)]


@pytest.mark.parametrize("p", ALL)
def test_autoks_equals_the_public_calls_for_every_prime_class(p):
    """n = 64; for the primes of EXACT also against the big-integer model, which the strict-range primes whose Barrett product wraps
    (PW63, PW31) need not meet"""
    torch = _torch()
    n = 64
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("autoks", p))
    ts = exponents(rng, n, 2)
    for i, (k, beta, ell, batch, add, with_ws) in enumerate(settings_for(p)):
        kw, kt = key_for(torch, plan, p, rng, k, ell, n)
        ct = words_with_zeros(rng, p, batch * (k + 1) * n)
        for t in (ts[i % len(ts)], ts[(i + 3) % len(ts)]):
            got = run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, add, batch, with_ws)
            want = compose(torch, plan, p, ct, kt, t, k, beta, ell, add, batch)
            assert got.any() and np.array_equal(got, want), (p, k, beta, ell, batch, add, t, "public calls", first_difference(got, want))
        if p in EXACT:
            want = np.array(model_autoks_batch(ct.tolist(), kw.tolist(), p, t, k, n, beta, ell, add, batch), dtype=dt(p))
            assert np.array_equal(got, want), (p, k, beta, ell, batch, add, t, "model", first_difference(got, want))


@pytest.mark.parametrize("p", [PM64, P30])
def test_autoks_at_the_smallest_size_against_the_model(p):
    torch = _torch()
    n = min_n(p)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("autoks-min", p))
    for k, beta, ell, batch, add, with_ws in settings_for(p)[2:5]:
        kw, kt = key_for(torch, plan, p, rng, k, ell, n)
        ct = words_with_zeros(rng, p, batch * (k + 1) * n)
        for t in exponents(rng, n, 1):
            got = run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, add, batch, with_ws)
            want = np.array(model_autoks_batch(ct.tolist(), kw.tolist(), p, t, k, n, beta, ell, add, batch), dtype=dt(p))
            assert np.array_equal(got, want), (p, k, beta, ell, batch, add, t, first_difference(got, want))


@pytest.mark.parametrize("p,n,k,batch", [(P62, 1024, 1, 3), (P30, 1024, 2, 3), (P62, 8192, 1, 2), (P62, 16384, 1, 2), (P30, 8192, 1, 2)])
def test_autoks_at_larger_sizes(p, n, k, batch):
    """n = 1024: the fused chain; 64-bit words at n = 8192 (the largest staged polynomial) and 16384 (the global gather) and 32-bit
    words at 8192: the composed external product, which keeps its own scratch"""
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("autoks-large", p, n))
    beta, ell = 7, 2
    kw, kt = key_for(torch, plan, p, rng, k, ell, n)
    ct = words_with_zeros(rng, p, batch * (k + 1) * n)
    for t, add in ((n // 2 + 1, True), (2 * int(rng.integers(0, n)) + 1, False)):
        got = run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, add, batch, with_ws=add)
        want = compose(torch, plan, p, ct, kt, t, k, beta, ell, add, batch)
        assert got.any() and np.array_equal(got, want), (p, n, t, add, first_difference(got, want))


@pytest.mark.parametrize("p", [P62, P32])
@pytest.mark.parametrize("with_ws", [False, True])
def test_autoks_on_the_host_path(p, with_ws):
    torch = _torch()
    n, beta, ell, batch = 64, 6, 3, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("autoks-host", p))
    for k in (1, 0):   # glwe_dim = 0: no digits, no key, nothing of the workspace
        kw, kt = key_for(torch, plan, p, rng, k, ell, n)
        ct = words_with_zeros(rng, p, batch * (k + 1) * n)
        for t, add in ((n + 1, True), (5, False)):
            got = run_autoks(torch, plan, p, "host", ct, kt, t, k, beta, ell, add, batch, with_ws)
            want = run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, add, batch)
            assert np.array_equal(got, want), (p, k, t, add, first_difference(got, want))
            assert np.array_equal(got, np.array(model_autoks_batch(ct.tolist(), kw.tolist(), p, t, k, n, beta, ell, add, batch), dtype=dt(p)))


# -- 4. the trace --------------------------------------------------------------------------------------------------------------------------
def run_trace(torch, plan, p, where, ct, kt, steps, k, beta, ell, batch, with_ws=False):
    out = poison(p, ct.size)
    nws = plan.glwe_trace_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.glwe_trace_batch(out, ct, None if kt is None else host(kt, dt(p)).copy(), steps, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.glwe_trace_batch(out_t, dev(torch, ct), kt, steps, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def steps_of_call_3(torch, plan, p, ct, kt, steps, k, beta, ell, batch):
    n = plan.ntt_size()
    per = k * ell * (k + 1) * n
    cur = ct
    for r, t in enumerate(trace_exponents(n, steps)):
        cur = run_autoks(torch, plan, p, "device", cur, kt[r * per:(r + 1) * per] if k else None, t, k, beta, ell, True, batch)
    return cur


@pytest.mark.parametrize("p,n,k", [(PM64, 16, 1), (P62, 32, 2), (P30, 32, 1), (P32, 64, 0), (P62, 1024, 1)])
def test_trace_equals_steps_calls_of_the_keyswitch(p, n, k):
    """every steps in [0, log2 n] (n = 1024: 0, 1, 2, 9 and 10), with a caller workspace on the odd ones; the host path once"""
    torch = _torch()
    logn = n.bit_length() - 1
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("trace", p, n))
    beta, ell, batch = 5, 2, 3
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    ct = words_with_zeros(rng, p, batch * (k + 1) * n)
    per = k * ell * (k + 1) * n
    for steps in range(logn + 1) if n <= 64 else (0, 1, 2, logn - 1, logn):
        keys = kt[:steps * per] if k and steps else None
        got = run_trace(torch, plan, p, "device", ct, keys, steps, k, beta, ell, batch, with_ws=steps % 2 == 1)
        want = steps_of_call_3(torch, plan, p, ct, kt, steps, k, beta, ell, batch)
        assert np.array_equal(got, want), (p, n, k, steps, first_difference(got, want))
        if steps == 0:
            assert np.array_equal(got, ct)
        if steps <= 2 and n <= 64:
            # no step (a copy), one step (the digits alone, and with glwe_dim = 0 nothing of the workspace) and two (the second
            # ciphertext too): the other workspace setting on the device, and the host path with and without a workspace
            for where, with_ws in (("device", steps % 2 == 0), ("host", False), ("host", True)):
                again = run_trace(torch, plan, p, where, ct, keys, steps, k, beta, ell, batch, with_ws=with_ws)
                assert np.array_equal(again, want), (p, n, k, steps, where, with_ws, first_difference(again, want))
    if n <= 64:
        assert np.array_equal(run_trace(torch, plan, p, "host", ct, kt, logn, k, beta, ell, batch, with_ws=True), got)


# -- 5. the LDS switch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", [(P62, 32), (P62, 1024), (P62, 8192), (P30, 1024)])
def test_both_settings_of_the_lds_switch_give_identical_words(p, n):
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("lds", p, n))
    k, beta, ell, batch, t = 1, 6, 2, 3, n // 2 + 1
    kw, kt = key_for(torch, plan, p, rng, k, ell, n)
    ct = words_with_zeros(rng, p, batch * (k + 1) * n)
    res = []
    for lds in (1, 0):
        with cntt.debug_switches(autom_lds=lds):
            a, b = dev(torch, poison(p, ct.size)), dev(torch, poison(p, ct.size))
            plan.automorphism_batch(a, dev(torch, ct), t)
            plan.automorphism_ntt_batch(b, dev(torch, ct), t)
            res.append((host(a, dt(p)), host(b, dt(p)), run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, True, batch)))
    for x, y in zip(*res):
        assert x.any() and np.array_equal(x, y), (p, n)
    assert np.array_equal(res[0][0], autom_gather_np(ct.reshape(-1, n), t, p).reshape(-1))


# -- 6. a second, ragged trip of the walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P30])
def test_walk_makes_a_second_trip_with_a_ragged_tail(p):
    """the grid rule caps the workgroups; a batch of cap / (k + 1) + 3 ciphertexts leaves 3 (k + 1) polynomials for a second trip that most
    workgroups do not make"""
    torch = _torch()
    n, k, beta, ell, t = 32, 1, 5, 2, 2 * 32 - 1
    w = np.dtype(dt(p)).itemsize
    cap = cntt.lib().cntt_prime_automorphism_grid(1 << 30, 5, w)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_prime_automorphism_grid(batch * (k + 1), 5, w) == cap < batch * (k + 1) < 2 * cap
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ragged", p))
    kw, kt = key_for(torch, plan, p, rng, k, ell, n)
    ct = words_with_zeros(rng, p, batch * (k + 1) * n)
    got = run_autoks(torch, plan, p, "device", ct, kt, t, k, beta, ell, True, batch)
    want = compose(torch, plan, p, ct, kt, t, k, beta, ell, True, batch)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], ct[tail])
    out = dev(torch, poison(p, ct.size))
    plan.automorphism_ntt_batch(out, dev(torch, ct), t)
    assert np.array_equal(host(out, dt(p)), ct.reshape(-1, n)[:, ntt_permutation(t, n)].reshape(-1))


# -- 7. graph capture ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_trace_with_a_caller_workspace():
    """captured once, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    p, n, k, beta, ell, batch = PM64, 1024, 1, 8, 3, 3
    logn = 10
    plan = make_plan(p, n)
    rng = np.random.default_rng(19)
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    ct = dev(torch, random_words(rng, p, batch * (k + 1) * n))
    ws = torch.zeros(plan.glwe_trace_workspace_bytes(k, ell, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(ct)
    plan.glwe_trace_batch(out, ct, kt, logn, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.glwe_trace_batch(out, ct, kt, logn, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, p, batch * (k + 1) * n))
        eager = torch.zeros_like(out)
        plan.glwe_trace_batch(eager, fresh, kt, logn, k, beta, ell)
        ct.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 8. encrypted messages -----------------------------------------------------------------------------------------------------------------
def test_full_trace_with_noisy_keys_keeps_the_constant_coefficient_only():
    """PM64 (W = 64), n = 256, k = 1, binary key S: a GLWE ciphertext carrying a 3-bit message in EVERY coefficient at steps of
    floor(p / 8), noise below 2^30, is scaled by n^-1 mod p and traced with the log2 n = 8 noisy automorphism keys (|e| < 2^10 per
    coefficient, base_log 8, levels 6).  The constant coefficient decodes to its message, every other coefficient to 0.
    Error bound: the trace is linear in the phase, so coefficient 0 comes out as message + the ciphertext's own noise, exactly; what is
    added is, per step, the rounding of the k = 1 mask polynomial to 48 bits (s = 16), at most k n 2^(s-1) = 2^23 per coefficient, and
    the key noise, k * levels * n digit coefficients of at most 2^7 times 2^10: below 2^28.  Every later step doubles what is there,
    so after 8 steps the sum stays below 2^9 * 2^29 = 2^38 -- far below the floor(p / 16) ~ 2^60 that half a message step allows."""
    torch = _torch()
    p, n, k, beta, ell = PM64, 256, 1, 8, 6
    logn = 8
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("trace-messages"))
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    S_words = S.astype(np.uint64)
    keys = []
    for t in trace_exponents(n, logn):
        rot = autom_gather_np(S_words, t, p).astype(object)
        rot = np.where(rot > p // 2, rot - p, rot)                               # sigma_t(S) with coefficients in {-1, 0, 1}
        A = random_words(rng, p, ell * n).reshape(ell, n)
        body = times_binary(A, NS) + rng.integers(-2 ** 10 + 1, 2 ** 10, size=(ell, n)).astype(object)
        for l in range(1, ell + 1):
            body[l - 1] += rot * (1 << (64 - beta * l))
        keys.append(np.stack([A, (body % p).astype(np.uint64)], axis=1).reshape(-1))     # AK[l][0] = mask, AK[l][1] = body
    kt = key_ntt(torch, plan, np.concatenate(keys))
    msgs = rng.integers(0, 8, size=n)
    a = random_words(rng, p, n)
    body = times_binary(a[None, :], NS)[0] + msgs.astype(object) * (p // 8) + rng.integers(-2 ** 30 + 1, 2 ** 30, size=n).astype(object)
    ct = np.concatenate([a.astype(object), body % p])
    n_inv = pow(n, -1, p)
    scaled = ((ct * n_inv) % p).astype(np.uint64)
    got = run_trace(torch, plan, p, "device", scaled, kt, logn, k, beta, ell, 1, with_ws=True)
    phase = (got[n:].astype(object) - times_binary(got[None, :n], NS)[0]) % p
    dec = [int((8 * int(x) + p // 2) // p) % 8 for x in phase]
    assert dec[0] == int(msgs[0]) and msgs[1:].any(), (dec[0], int(msgs[0]))
    assert not any(dec[1:]), dec
    centred = [min(int(x), p - int(x)) for x in phase[1:]]
    assert max(centred) < 1 << 38, max(centred).bit_length()


# -- 9. the C example ----------------------------------------------------------------------------------------------------------------------
def test_trace_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "trace_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "trace_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "only the constant coefficient survived" in r.stdout, r.stdout
