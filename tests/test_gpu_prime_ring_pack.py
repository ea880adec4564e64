"""Ring packing of LWE ciphertexts through automorphisms on the prime plans (include/cntt_prime_ring_pack.h) on the MI355X.  Bit-exact
throughout, no tolerance anywhere: the embedding against the model of tests/prime_ring_pack_model.py and against sample extraction; one
tree node against the big-integer model on the exact primes and against the sequence of public calls the header states on every prime
class, over rotations that hit unaligned reads and sign wraps; the size classes of the staging; both settings of the "autom_lds" switch;
a walk that makes a second, ragged trip; the whole packing against embed -> per-stage merges -> trace; graph capture; encrypted messages
through noisy keys; the C example.  The one functional test states its derived noise bound in its docstring."""
import os
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_prime_automorphism as tga
from prime_automorphism_model import autom_gather_np, trace_exponents
from prime_ring_pack_model import LDS_BYTES, embed_np, merge_parts_np, model_merge, stage_params
from test_gpu_prime_pack import first_difference, negacyclic_matrix, tdtype, times_binary
from test_gpu_prime_pbs import ALL, EXACT, _torch, dev, dt, host, is64, key_ntt, make_plan, min_n, random_words, seed
from test_prime_pbs_model import P30, P32, P62, PM64, model_extract, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
poison, words_with_zeros, key_for = tga.poison, tga.words_with_zeros, tga.key_for


def shifts(n):
    """aligned and unaligned rotated reads, the sign wrap at n and the last exponent"""
    return [0, 1, n // 2, n - 1, n, 2 * n - 1]


# -- 1. the embedding ------------------------------------------------------------------------------------------------------------------------
def run_embed(torch, plan, p, where, lwe, k):
    n = plan.ntt_size()
    batch = lwe.size // (k * n + 1)
    out = poison(p, batch * (k + 1) * n)
    if where == "host":
        plan.glwe_embed_batch(out, lwe, k)
        return out
    out_t = dev(torch, out)
    plan.glwe_embed_batch(out_t, dev(torch, lwe), k)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", [P62, PM64, P30, P32])
def test_embed_matches_model_and_inverts_sample_extraction(p, where):
    torch = _torch()
    for n in (min_n(p), 1024):
        plan = make_plan(p, n)
        rng = np.random.default_rng(seed("embed", p, n))
        for k in (0, 1, 2):
            batch = 3
            lwe = words_with_zeros(rng, p, batch * (k * n + 1))
            got = run_embed(torch, plan, p, where, lwe, k)
            want = embed_np(lwe.reshape(batch, k * n + 1), p, k, n).reshape(-1)
            assert got.any() and np.array_equal(got, want), (p, n, k, where, first_difference(got, want))
            if n == min_n(p):                                         # the numpy form is the plain-int model's
                g = got[:(k + 1) * n].tolist()
                assert model_extract([g[q * n:(q + 1) * n] for q in range(k + 1)], 0, p) == lwe[:k * n + 1].tolist()
            back = poison(p, lwe.size)
            if where == "host":
                plan.sample_extract_batch(back, got, k, 0)
            else:
                back_t = dev(torch, back)
                plan.sample_extract_batch(back_t, dev(torch, got), k, 0)
                back = host(back_t, dt(p))
            assert np.array_equal(back, lwe), (p, n, k, where)


# -- 2. one tree node ----------------------------------------------------------------------------------------------------------------------
def run_merge(torch, plan, p, where, E, O, kt, shift, t, k, beta, ell, with_ws=False):
    """call 2 on word arrays (the key as the NTT-domain device tensor, or None) -> the output array, poisoned before"""
    n = plan.ntt_size()
    batch = E.size // ((k + 1) * n)
    out = poison(p, E.size)
    nws = plan.glwe_merge_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.glwe_merge_batch(out, E, O, None if kt is None else host(kt, dt(p)).copy(), shift, t, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.glwe_merge_batch(out_t, dev(torch, E), dev(torch, O), kt, shift, t, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def compose_merge(torch, plan, p, E, O, kt, shift, t, k, beta, ell):
    """The header's sequence of public calls: a and d built on the host, automorphism_batch on d, the prefill (a, the body plus the
    permuted body of d), gadget_decompose_batch(plain) on the permuted mask polynomials, the digits negated mod p on the host,
    external_product_batch(accumulate=True)."""
    n = plan.ntt_size()
    batch = E.size // ((k + 1) * n)
    a, d = merge_parts_np(E.reshape(batch, k + 1, n), O.reshape(batch, k + 1, n), shift, p)
    rot_t = dev(torch, poison(p, d.size))
    plan.automorphism_batch(rot_t, dev(torch, d.reshape(-1)), t)
    torch.cuda.synchronize()
    rot = host(rot_t, dt(p)).reshape(batch, k + 1, n)
    out = a.copy()
    out[:, k] = tga.addp(a[:, k], rot[:, k], p)
    out_t = dev(torch, out.reshape(-1))
    if k:
        terms = torch.zeros(batch * k * ell * n, dtype=tdtype(torch, p), device="cuda")
        plan.gadget_decompose_batch(terms, dev(torch, rot[:, :k].reshape(-1)), beta, ell, mode="plain")
        torch.cuda.synchronize()
        g = host(terms, dt(p))
        plan.external_product_batch(out_t, dev(torch, np.where(g == 0, g, dt(p)(p) - g)), kt, k * ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def merge_settings(p):
    """(k, base_log, levels, batch, with_ws): k 0 / 1 / 2, levels 1 / 2 / 3, base_log * levels = W once"""
    W = wbits(p)
    return [(0, 4, 2, 3, False), (1, min(W, 22), 1, 1, True), (1, W // 2, 2, 3, False), (2, 6, 3, 2, True)]


@pytest.mark.parametrize("p", ALL)
def test_merge_equals_the_public_calls_for_every_prime_class(p):
    """n = 64, every shift of shifts(), several t; for the primes of EXACT also against the big-integer model"""
    torch = _torch()
    n = 64
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("merge", p))
    ts = tga.exponents(rng, n, 2)
    for i, (k, beta, ell, batch, with_ws) in enumerate(merge_settings(p)):
        kw, kt = key_for(torch, plan, p, rng, k, ell, n)
        E, O = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
        for j, shift in enumerate(shifts(n)):
            t = ts[(i + 2 * j) % len(ts)]
            got = run_merge(torch, plan, p, "device", E, O, kt, shift, t, k, beta, ell, with_ws)
            want = compose_merge(torch, plan, p, E, O, kt, shift, t, k, beta, ell)
            assert got.any() and np.array_equal(got, want), (p, k, beta, ell, shift, t, "public calls", first_difference(got, want))
            if p in EXACT and j % 3 == i % 3:
                per = (k + 1) * n
                want = [w for b in range(batch) for w in model_merge(E[b * per:(b + 1) * per].tolist(), O[b * per:(b + 1) * per].tolist(),
                                                                     kw.tolist(), p, shift, t, k, n, beta, ell)]
                assert np.array_equal(got, np.array(want, dtype=dt(p))), (p, k, shift, t, "model")


@pytest.mark.parametrize("p,n,k", [(P62, 1024, 1), (P30, 1024, 2), (P62, 4096, 1), (P62, 8192, 1), (P30, 16384, 1)])
def test_merge_size_classes(p, n, k):
    """n = 1024: the fused chain; 64-bit words at n = 4096, the largest size at which both sources are staged, and at 8192, the global
    gather; 32-bit words at 16384, the global gather"""
    torch = _torch()
    staged = 2 * n * np.dtype(dt(p)).itemsize <= LDS_BYTES
    assert staged == (n <= 4096)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("merge-large", p, n))
    beta, ell, batch = 7, 2, 2
    kw, kt = key_for(torch, plan, p, rng, k, ell, n)
    E, O = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
    for shift, t in ((n // 2 + 1, n // 2 + 1), (2 * n - 1, 2 * int(rng.integers(0, n)) + 1)):
        got = run_merge(torch, plan, p, "device", E, O, kt, shift, t, k, beta, ell, with_ws=shift > n)
        want = compose_merge(torch, plan, p, E, O, kt, shift, t, k, beta, ell)
        assert got.any() and np.array_equal(got, want), (p, n, shift, t, first_difference(got, want))


@pytest.mark.parametrize("p", [P62, P32])
def test_merge_on_the_host_path(p):
    torch = _torch()
    n, beta, ell, batch = 64, 6, 3, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("merge-host", p))
    for k in (1, 0):   # glwe_dim = 0: no digits, no key, nothing of the workspace -- there the device path with one as well
        kw, kt = key_for(torch, plan, p, rng, k, ell, n)
        E, O = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
        for shift, t, with_ws in ((n + 3, n + 1, True), (5, 5, False)):
            got = run_merge(torch, plan, p, "host", E, O, kt, shift, t, k, beta, ell, with_ws)
            assert np.array_equal(got, run_merge(torch, plan, p, "device", E, O, kt, shift, t, k, beta, ell)), (p, k, shift, t)
            if k == 0:
                assert np.array_equal(got, compose_merge(torch, plan, p, E, O, kt, shift, t, k, beta, ell)), (p, shift, t)
                assert np.array_equal(got, run_merge(torch, plan, p, "device", E, O, kt, shift, t, k, beta, ell, with_ws=True)), (p, shift, t)


# -- 3. the whole packing ------------------------------------------------------------------------------------------------------------------
def run_pack(torch, plan, p, where, lwe, kt, m, k, beta, ell, batch, with_ws=False):
    n = plan.ntt_size()
    out = poison(p, batch * (k + 1) * n)
    nws = plan.ring_pack_workspace_bytes(m, k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.ring_pack_batch(out, lwe, None if kt is None else host(kt, dt(p)).copy(), m, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.ring_pack_batch(out_t, dev(torch, lwe), kt, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def compose_pack(torch, plan, p, lwe, kt, m, k, beta, ell, batch):
    """the header's sequence: glwe_embed_batch on all M ciphertexts, one glwe_merge_batch per stage on the batch * h pairs of that stage,
    glwe_trace_batch"""
    n = plan.ntt_size()
    logn = n.bit_length() - 1
    per = k * ell * (k + 1) * n
    cur = run_embed(torch, plan, p, "device", lwe, k).reshape(batch, m, (k + 1) * n)
    for h, shift, t, r in stage_params(n, m):
        E, O = np.ascontiguousarray(cur[:, :h]).reshape(-1), np.ascontiguousarray(cur[:, h:]).reshape(-1)
        cur = run_merge(torch, plan, p, "device", E, O, kt[r * per:(r + 1) * per] if k else None, shift, t, k, beta, ell).reshape(batch, h, (k + 1) * n)
    steps = logn - (m.bit_length() - 1)
    return tga.run_trace(torch, plan, p, "device", cur.reshape(-1), kt[:steps * per] if k and steps else None, steps, k, beta, ell, batch)


@pytest.mark.parametrize("p,n,k,batch", [(P62, 32, 1, 1), (P30, 32, 2, 3), (PM64, 32, 0, 3), (P32, 32, 1, 3), (P62, 1024, 1, 1), (P30, 1024, 1, 1)])
def test_ring_pack_equals_embed_merges_and_trace(p, n, k, batch):
    """n = 32 with M in {1, 2, 8, 32}, n = 1024 with M in {1, 4, 1024}; with a caller workspace on every second M; the host path once"""
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("pack", p, n, k))
    beta, ell = 5, 2
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=n.bit_length() - 1)
    for i, m in enumerate((1, 2, 8, 32) if n == 32 else (1, 4, 1024)):
        lwe = words_with_zeros(rng, p, batch * m * (k * n + 1))
        want = compose_pack(torch, plan, p, lwe, kt, m, k, beta, ell, batch)
        for with_ws in (False, True):
            got = run_pack(torch, plan, p, "device", lwe, kt, m, k, beta, ell, batch, with_ws)
            assert got.any() and np.array_equal(got, want), (p, n, k, m, with_ws, first_difference(got, want))
        if n == 32 and m == 8:
            assert np.array_equal(run_pack(torch, plan, p, "host", lwe, kt, m, k, beta, ell, batch, with_ws=True), want), (p, k, "host")
            assert np.array_equal(run_pack(torch, plan, p, "host", lwe, kt, m, k, beta, ell, batch, with_ws=False), want), (p, k, "host, no workspace")


@pytest.mark.parametrize("p,k", [(P62, 1), (P30, 2), (PM64, 0)])
def test_lwe_leaf_stage_equals_embedding_then_merging(p, k):
    """M = 2: the packing is stage 1 -- which reads the LWE rows as leaves and never writes their embeddings -- and the trace; the same
    words as glwe_embed_batch, glwe_merge_batch(shift = n / 2, t = 3) and glwe_trace_batch(steps = log2 n - 1).  At M = n (no trace at
    all: the last stage writes glwe_out) the leaves feed log2 n stages."""
    torch = _torch()
    n = min_n(p)
    logn = n.bit_length() - 1
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("leaf", p, k))
    beta, ell, batch = 6, 2, 3
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    per = k * ell * (k + 1) * n
    lwe = words_with_zeros(rng, p, batch * 2 * (k * n + 1))
    emb = run_embed(torch, plan, p, "device", lwe, k).reshape(batch, 2, (k + 1) * n)
    node = run_merge(torch, plan, p, "device", np.ascontiguousarray(emb[:, 0]).reshape(-1), np.ascontiguousarray(emb[:, 1]).reshape(-1),
                     kt[(logn - 1) * per:] if k else None, n // 2, 3, k, beta, ell)
    want = tga.run_trace(torch, plan, p, "device", node, kt[:(logn - 1) * per] if k else None, logn - 1, k, beta, ell, batch)
    got = run_pack(torch, plan, p, "device", lwe, kt, 2, k, beta, ell, batch, with_ws=True)
    assert got.any() and np.array_equal(got, want), (p, k, first_difference(got, want))
    lwe = words_with_zeros(rng, p, batch * n * (k * n + 1))
    got = run_pack(torch, plan, p, "device", lwe, kt, n, k, beta, ell, batch)
    assert np.array_equal(got, compose_pack(torch, plan, p, lwe, kt, n, k, beta, ell, batch)), (p, k, "M = n")


# -- 4. the LDS switch ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", [(P62, 64), (P62, 1024), (P30, 64), (P30, 1024)])
def test_both_settings_of_the_lds_switch_give_identical_words(p, n):
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ring-lds", p, n))
    k, beta, ell, batch, m = 1, 6, 2, 3, 4
    logn = n.bit_length() - 1
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    E, O = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
    lwe = words_with_zeros(rng, p, batch * m * (k * n + 1))
    res = []
    for lds in (1, 0):
        with cntt.debug_switches(autom_lds=lds):
            res.append((run_merge(torch, plan, p, "device", E, O, kt[:k * ell * (k + 1) * n], n - 1, n // 2 + 1, k, beta, ell),
                        run_pack(torch, plan, p, "device", lwe, kt, m, k, beta, ell, batch)))
    for x, y in zip(*res):
        assert x.any() and np.array_equal(x, y), (p, n)
    assert np.array_equal(res[0][0], compose_merge(torch, plan, p, E, O, kt[:k * ell * (k + 1) * n], n - 1, n // 2 + 1, k, beta, ell))


# -- 5. a second, ragged trip of the walk ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P30])
def test_walk_makes_a_second_trip_with_a_ragged_tail(p):
    """the grid rule caps the workgroups; cap / (k + 1) + 3 output ciphertexts leave 3 (k + 1) polynomials for a second trip that most
    workgroups do not make -- in the merge, in the embedding, and in stage 1 of a packing with M = 2"""
    torch = _torch()
    n, k, beta, ell = min_n(p), 1, 5, 2
    logn = n.bit_length() - 1
    w = np.dtype(dt(p)).itemsize
    cap = cntt.lib().cntt_prime_ring_pack_grid(1 << 30, logn, w)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_prime_ring_pack_grid(batch * (k + 1), logn, w) == cap < batch * (k + 1) < 2 * cap
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ring-ragged", p))
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=logn)
    one = kt[(logn - 1) * k * ell * (k + 1) * n:]
    lwe = words_with_zeros(rng, p, batch * 2 * (k * n + 1))
    emb = run_embed(torch, plan, p, "device", lwe, k)
    assert np.array_equal(emb, embed_np(lwe.reshape(-1, k * n + 1), p, k, n).reshape(-1))
    pairs = emb.reshape(batch, 2, (k + 1) * n)
    E, O = np.ascontiguousarray(pairs[:, 0]).reshape(-1), np.ascontiguousarray(pairs[:, 1]).reshape(-1)
    got = run_merge(torch, plan, p, "device", E, O, one, n // 2, 3, k, beta, ell)
    want = compose_merge(torch, plan, p, E, O, one, n // 2, 3, k, beta, ell)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], E[tail])
    packed = run_pack(torch, plan, p, "device", lwe, kt, 2, k, beta, ell, batch)
    assert np.array_equal(packed, tga.run_trace(torch, plan, p, "device", got, kt[:(logn - 1) * k * ell * (k + 1) * n], logn - 1, k, beta, ell, batch))


# -- 6. graph capture ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_ring_pack_with_a_caller_workspace():
    """captured once, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    p, n, k, beta, ell, batch, m = PM64, 1024, 1, 8, 3, 2, 16
    plan = make_plan(p, n)
    rng = np.random.default_rng(20)
    kw, kt = key_for(torch, plan, p, rng, k, ell, n, keys=10)
    lwe = dev(torch, random_words(rng, p, batch * m * (k * n + 1)))
    ws = torch.zeros(plan.ring_pack_workspace_bytes(m, k, ell, batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(p, batch * (k + 1) * n))
    plan.ring_pack_batch(out, lwe, kt, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.ring_pack_batch(out, lwe, kt, m, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, p, batch * m * (k * n + 1)))
        eager = torch.zeros_like(out)
        plan.ring_pack_batch(eager, fresh, kt, m, k, beta, ell)
        lwe.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 7. encrypted messages -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [16, 256])
def test_packed_messages_decode_at_their_strided_coefficients(m):
    """PM64 (W = 64), n = 256, k = 1, binary key S: M LWE ciphertexts under the flattened key, each a 3-bit message at steps of
    floor(p / 8) with noise below 2^30, scaled by n^-1 mod p, are packed with the log2 n = 8 noisy trace keys (|e| < 2^10 per coefficient,
    base_log 16, levels 4: base_log * levels = 64, no rounding).  Message j decodes at coefficient j n / M and every other coefficient
    decodes to 0; no case is left out.
    Error bound: the packing is linear in the phase, so message j comes out with its own LWE noise, below 2^30.  Each of the log2 n = 8
    keyswitches adds the key noise, k n levels digit coefficients of at most B / 2 = 2^15 times 2^10, below 2^35 per coefficient, and every
    later step at most doubles what is there; the issue's worst case n log2 n k n levels (B / 2) 2^10 = 2^8 * 2^3 * 2^35 = 2^46 bounds
    the sum -- far below the floor(p / 16) ~ 2^60 that half a message step allows."""
    torch = _torch()
    p, n, k, beta, ell = PM64, 256, 1, 16, 4
    logn = 8
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ring-messages", m))
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
    msgs = rng.integers(0, 8, size=m)
    mask = random_words(rng, p, m * n).reshape(m, n)
    dot = (mask.astype(object) * S.astype(object)).sum(axis=1)                   # <mask, s> under the flattened key s = S
    body = dot + msgs.astype(object) * (p // 8) + rng.integers(-2 ** 30 + 1, 2 ** 30, size=m).astype(object)
    lwe = np.concatenate([mask.astype(object), (body % p)[:, None]], axis=1)
    scaled = ((lwe * pow(n, -1, p)) % p).astype(np.uint64).reshape(-1)
    got = run_pack(torch, plan, p, "device", scaled, kt, m, k, beta, ell, 1, with_ws=True)
    phase = (got[n:].astype(object) - times_binary(got[None, :n], NS)[0]) % p
    dec = [int((8 * int(x) + p // 2) // p) % 8 for x in phase]
    want = [0] * n
    for j in range(m):
        want[j * (n // m)] = int(msgs[j])
    assert msgs.any() and dec == want, (m, dec, want)
    err = [(int(x) - w * (p // 8)) % p for x, w in zip(phase, want)]
    assert max(min(e, p - e) for e in err) < 1 << 46


# -- 8. the C example ----------------------------------------------------------------------------------------------------------------------
def test_ring_pack_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "ring_pack_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "ring_pack_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "every message decoded at its strided coefficient" in r.stdout, r.stdout
