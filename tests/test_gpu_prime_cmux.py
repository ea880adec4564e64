"""The CMux and the CMux tree against GGSW selectors on the prime plans (include/cntt_prime_cmux.h) on the MI355X.  Bit-exact throughout,
no tolerance anywhere: call 1 against the sequence of public calls the header states on every prime class and against the big-integer
model on the exact primes; the size classes of the external product; the host path; the tree against the leaf stage from public calls
and one glwe_cmux_batch per stage; the leaf stage against call 1 on trivial ciphertexts; a walk that makes a second, ragged trip; graph
capture; the STREAM form at its first shape; a whole encrypted table lookup through noisy selectors; the C example.  The one functional
test states its derived noise bound in its docstring."""
import gc
import os
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_prime_automorphism as tga
from prime_cmux_model import model_cmux, stage_params
from test_gpu_prime_pack import first_difference, negacyclic_matrix, tdtype, times_binary
from test_gpu_prime_pbs import ALL, EXACT, STREAM_BYTES, _torch, dev, device_words, dt, host, key_ntt, make_plan, min_n, random_words, seed
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
poison, words_with_zeros = tga.poison, tga.words_with_zeros


def sel_polys(k, ell):
    return (k + 1) * ell * (k + 1)


def selectors(torch, plan, p, rng, k, ell, n, count=1):
    """(coefficient-domain words, the NTT-domain device tensor) of `count` random selectors: the statements are about the words"""
    kw = random_words(rng, p, count * sel_polys(k, ell) * n)
    return kw, key_ntt(torch, plan, kw)


def subp(a, b, p):
    """a - b mod p on canonical words"""
    d = a.astype(object) - b.astype(object)
    return np.where(d < 0, d + p, d).astype(a.dtype)


# -- 1. one node -----------------------------------------------------------------------------------------------------------------------------
def run_cmux(torch, plan, p, where, c0, c1, kt, k, beta, ell, with_ws=False):
    """call 1 on word arrays (the selector as the NTT-domain device tensor) -> the output array, poisoned before"""
    n = plan.ntt_size()
    batch = c0.size // ((k + 1) * n)
    out = poison(p, c0.size)
    nws = plan.glwe_cmux_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.glwe_cmux_batch(out, c0, c1, host(kt, dt(p)).copy(), k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.glwe_cmux_batch(out_t, dev(torch, c0), dev(torch, c1), kt, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def compose_cmux(torch, plan, p, c0, c1, kt, k, beta, ell):
    """The header's sequence of public calls: the copy of c0, the difference on the host, gadget_decompose_batch(plain) -- the digits as
    they come -- and external_product_batch(accumulate=True)."""
    n = plan.ntt_size()
    batch = c0.size // ((k + 1) * n)
    out_t = dev(torch, c0.copy())
    terms = torch.zeros(batch * (k + 1) * ell * n, dtype=tdtype(torch, p), device="cuda")
    plan.gadget_decompose_batch(terms, dev(torch, subp(c1, c0, p)), beta, ell, mode="plain")
    plan.external_product_batch(out_t, terms, kt, (k + 1) * ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def cmux_settings(p):
    """(k, base_log, levels, batch): k 0 / 1 / 2, levels 1 / 2 / 3, base_log * levels = W once"""
    W = wbits(p)
    return [(0, 4, 2, 3), (1, min(W, 22), 1, 1), (1, W // 2, 2, 3), (2, 6, 3, 2)]


@pytest.mark.parametrize("p", ALL)
def test_cmux_equals_the_public_calls_for_every_prime_class(p):
    """n = 64, with and without a caller workspace; for the primes of EXACT a third of the cases also against the big-integer model"""
    torch = _torch()
    n = 64
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux", p))
    case = 0
    for k, beta, ell, batch in cmux_settings(p):
        kw, kt = selectors(torch, plan, p, rng, k, ell, n)
        c0, c1 = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
        c1[:n // 2] = c0[:n // 2]                                    # equal words: a zero difference, all digits zero
        want = compose_cmux(torch, plan, p, c0, c1, kt, k, beta, ell)
        for with_ws in (False, True):
            got = run_cmux(torch, plan, p, "device", c0, c1, kt, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, want), (p, k, beta, ell, with_ws, "public calls", first_difference(got, want))
            if p in EXACT and case % 3 == 0:
                per = (k + 1) * n
                model = [w for b in range(batch) for w in model_cmux(c0[b * per:(b + 1) * per].tolist(), c1[b * per:(b + 1) * per].tolist(),
                                                                     kw.tolist(), p, k, n, beta, ell)]
                assert np.array_equal(got, np.array(model, dtype=dt(p))), (p, k, beta, ell, "model")
            case += 1


@pytest.mark.parametrize("p,n,k", [(P62, 1024, 1), (P30, 1024, 2), (P62, 4096, 1), (P30, 16384, 1)])
def test_cmux_size_classes(p, n, k):
    """n = 1024: the fused chain; 64-bit words at n = 4096 and 32-bit words at 16384: the composed product"""
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux-large", p, n))
    beta, ell, batch = 7, 2, 2
    kw, kt = selectors(torch, plan, p, rng, k, ell, n)
    c0, c1 = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
    want = compose_cmux(torch, plan, p, c0, c1, kt, k, beta, ell)
    for with_ws in (False, True):
        got = run_cmux(torch, plan, p, "device", c0, c1, kt, k, beta, ell, with_ws)
        assert got.any() and np.array_equal(got, want), (p, n, with_ws, first_difference(got, want))


@pytest.mark.parametrize("p", [P62, P32])
def test_cmux_on_the_host_path(p):
    torch = _torch()
    n, beta, ell, batch = 64, 6, 3, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux-host", p))
    for k in (1, 0):
        kw, kt = selectors(torch, plan, p, rng, k, ell, n)
        c0, c1 = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
        want = run_cmux(torch, plan, p, "device", c0, c1, kt, k, beta, ell)
        for with_ws in (True, False):
            got = run_cmux(torch, plan, p, "host", c0, c1, kt, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, want), (p, k, with_ws, first_difference(got, want))


# -- 2. the tree -----------------------------------------------------------------------------------------------------------------------------
def run_tree(torch, plan, p, where, lut, kt, m, k, beta, ell, batch, with_ws=False):
    n = plan.ntt_size()
    out = poison(p, batch * (k + 1) * n)
    nws = plan.cmux_tree_workspace_bytes(m, k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws and nws else None   # one entry needs none
        plan.cmux_tree_batch(out, lut, None if kt is None else host(kt, dt(p)).copy(), m, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.cmux_tree_batch(out_t, dev(torch, lut), kt, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def compose_leaf(torch, plan, p, f0, f1, sel, k, beta, ell):
    """stage 1 as the header defines it, from public calls: zero masks, the body f0, the `levels` digit polynomials of f1 - f0, and
    external_product_batch(nterms = levels, accumulate=True) against the selector's body rows.  f0, f1: (count, n) word arrays."""
    n = plan.ntt_size()
    count = f0.shape[0]
    out = np.zeros((count, k + 1, n), dtype=dt(p))
    out[:, k] = f0
    out_t = dev(torch, out.reshape(-1))
    terms = torch.zeros(count * ell * n, dtype=tdtype(torch, p), device="cuda")
    plan.gadget_decompose_batch(terms, dev(torch, subp(f1, f0, p).reshape(-1)), beta, ell, mode="plain")
    plan.external_product_batch(out_t, terms, sel[k * ell * (k + 1) * n:], ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def compose_tree(torch, plan, p, lut, kt, m, k, beta, ell, batch):
    """the header's sequence: the leaf stage from public calls, then one glwe_cmux_batch per stage on the batch * h pairs of that stage"""
    n = plan.ntt_size()
    per = sel_polys(k, ell) * n
    if m == 1:
        out = np.zeros((batch, k + 1, n), dtype=dt(p))
        out[:, k] = lut.reshape(batch, n)
        return out.reshape(-1)
    cur = lut.reshape(batch, m, n)
    for s, (h, i) in enumerate(stage_params(m), 1):
        sel = kt[i * per:(i + 1) * per]
        lo, hi = np.ascontiguousarray(cur[:, :h]), np.ascontiguousarray(cur[:, h:])
        if s == 1:
            cur = compose_leaf(torch, plan, p, lo.reshape(batch * h, n), hi.reshape(batch * h, n), sel, k, beta, ell)
        else:
            cur = run_cmux(torch, plan, p, "device", lo.reshape(-1), hi.reshape(-1), sel, k, beta, ell)
        cur = cur.reshape(batch, h, (k + 1) * n)
    return cur.reshape(-1)


@pytest.mark.parametrize("p,n,k,batch", [(P62, 32, 1, 1), (P30, 32, 2, 3), (PM64, 32, 0, 3), (P32, 32, 1, 3), (P62, 1024, 1, 3), (P30, 1024, 2, 1),
                                         (PM64, 1024, 0, 1)])
def test_tree_equals_the_leaf_stage_and_one_cmux_per_stage(p, n, k, batch):
    """n = 32 with M in {1, 2, 4, 16}, n = 1024 with M in {1, 8}; both workspace modes; the host path once"""
    torch = _torch()
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("tree", p, n, k))
    beta, ell = 5, 2
    for m in (1, 2, 4, 16) if n == 32 else (1, 8):
        depth = m.bit_length() - 1
        kt = selectors(torch, plan, p, rng, k, ell, n, depth)[1] if depth else None
        lut = words_with_zeros(rng, p, batch * m * n)
        want = compose_tree(torch, plan, p, lut, kt, m, k, beta, ell, batch)
        for with_ws in (False, True):
            got = run_tree(torch, plan, p, "device", lut, kt, m, k, beta, ell, batch, with_ws)
            assert got.any() and np.array_equal(got, want), (p, n, k, m, with_ws, first_difference(got, want))
        if n == 32 and m in (1, 4):
            assert np.array_equal(run_tree(torch, plan, p, "host", lut, kt, m, k, beta, ell, batch, with_ws=True), want), (p, k, m, "host")
            assert np.array_equal(run_tree(torch, plan, p, "host", lut, kt, m, k, beta, ell, batch, with_ws=False), want), (p, k, m, "host, no workspace")


@pytest.mark.parametrize("p,k", [(P62, 1), (P30, 2), (PM64, 0), (P32, 1)])
def test_leaf_stage_equals_cmux_on_trivial_ciphertexts(p, k):
    """M = 2 is the leaf stage alone.  On the exact primes it has the words of glwe_cmux_batch on host-built trivial ciphertexts, whose
    zero masks call 1 does decompose."""
    assert p in EXACT
    torch = _torch()
    for n in (min_n(p), 1024):
        plan = make_plan(p, n)
        rng = np.random.default_rng(seed("leaf", p, k, n))
        beta, ell, batch = 6, 2, 3
        kw, kt = selectors(torch, plan, p, rng, k, ell, n)
        lut = words_with_zeros(rng, p, batch * 2 * n)
        triv = np.zeros((batch, 2, k + 1, n), dtype=dt(p))
        triv[:, :, k] = lut.reshape(batch, 2, n)
        want = run_cmux(torch, plan, p, "device", np.ascontiguousarray(triv[:, 0]).reshape(-1), np.ascontiguousarray(triv[:, 1]).reshape(-1), kt, k, beta, ell)
        got = run_tree(torch, plan, p, "device", lut, kt, 2, k, beta, ell, batch, with_ws=True)
        assert got.any() and np.array_equal(got, want), (p, k, n, first_difference(got, want))


# -- 3. a second, ragged trip of the walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P30])
def test_walk_makes_a_second_trip_with_a_ragged_tail(p):
    """the grid rule caps the workgroups; cap / (k + 1) + 3 output ciphertexts leave 3 (k + 1) polynomials for a second trip that most
    workgroups do not make -- in call 1 and in the leaf stage of a tree with M = 2"""
    torch = _torch()
    n, k, beta, ell = min_n(p), 1, 5, 2
    logn = n.bit_length() - 1
    w = np.dtype(dt(p)).itemsize
    cap = cntt.lib().cntt_prime_cmux_grid(1 << 30, logn, w)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_prime_cmux_grid(batch * (k + 1), logn, w) == cap < batch * (k + 1) < 2 * cap
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux-ragged", p))
    kw, kt = selectors(torch, plan, p, rng, k, ell, n)
    c0, c1 = (words_with_zeros(rng, p, batch * (k + 1) * n) for _ in range(2))
    got = run_cmux(torch, plan, p, "device", c0, c1, kt, k, beta, ell)
    want = compose_cmux(torch, plan, p, c0, c1, kt, k, beta, ell)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], c0[tail]) and not np.array_equal(got[tail], poison(p, got[tail].size))
    lut = words_with_zeros(rng, p, batch * 2 * n)
    got = run_tree(torch, plan, p, "device", lut, kt, 2, k, beta, ell, batch)
    want = compose_tree(torch, plan, p, lut, kt, 2, k, beta, ell, batch)
    assert np.array_equal(got, want), first_difference(got, want)
    assert got[tail].any() and not np.array_equal(got[tail], poison(p, got[tail].size))


# -- 4. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_tree_with_a_caller_workspace():
    """captured once, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    p, n, k, beta, ell, batch, m = PM64, 1024, 1, 8, 3, 2, 16
    plan = make_plan(p, n)
    rng = np.random.default_rng(23)
    kt = selectors(torch, plan, p, rng, k, ell, n, 4)[1]
    lut = dev(torch, random_words(rng, p, batch * m * n))
    ws = torch.zeros(plan.cmux_tree_workspace_bytes(m, k, ell, batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(p, batch * (k + 1) * n))
    plan.cmux_tree_batch(out, lut, kt, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.cmux_tree_batch(out, lut, kt, m, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, p, batch * m * n))
        eager = torch.zeros_like(out)
        plan.cmux_tree_batch(eager, fresh, kt, m, k, beta, ell)
        lut.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 5. the STREAM form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,beta", [(P62, 4), (P30, 2)])
def test_cmux_and_leaf_stage_of_a_streaming_batch(p, beta):
    """prime_cmux_diff_kernel<T, true, LEAF>: the first batch whose digits pass STREAM_BYTES (host_prime_cmux.inc compares
    nct * (k + 1) * levels * n * word for ciphertext sources and nct * levels * n * word for table leaves), at n = 1024, k = 1 and 15
    levels, with a caller workspace of exactly the workspace formula.  Every word against the call over two halves of the batch, which
    do not stream; the first and the last element against the public calls."""
    torch = _torch()
    n, k, ell = 1024, 1, 15
    w = np.dtype(dt(p)).itemsize
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux-stream", p))
    kw, kt = selectors(torch, plan, p, rng, k, ell, n)
    del kw
    gen = torch.Generator(device="cuda").manual_seed(seed("cmux-stream", p))
    for leaf in (False, True):
        unit = (1 if leaf else k + 1) * ell * n * w
        batch = STREAM_BYTES // unit + 1
        assert batch * unit > STREAM_BYTES >= (batch - 1) * unit and (batch - batch // 2) * unit <= STREAM_BYTES
        per_in, per_out = (2 * n if leaf else (k + 1) * n), (k + 1) * n
        a = device_words(torch, p, batch * per_in, gen)
        b = None if leaf else device_words(torch, p, batch * per_in, gen)
        out = torch.full((batch * per_out,), 0x5A5A5A5A, dtype=a.dtype, device="cuda")
        nws = plan.cmux_tree_workspace_bytes(2, k, ell, batch) if leaf else plan.glwe_cmux_workspace_bytes(k, ell, batch)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

        def call(dst, lo, hi, workspace=None):
            if leaf:
                plan.cmux_tree_batch(dst, a[lo * per_in:hi * per_in], kt, 2, k, beta, ell, workspace=workspace)
            else:
                plan.glwe_cmux_batch(dst, a[lo * per_in:hi * per_in], b[lo * per_in:hi * per_in], kt, k, beta, ell, workspace=workspace)

        call(out, 0, batch, ws)
        half = batch // 2
        small = torch.empty((batch - half) * per_out, dtype=a.dtype, device="cuda")
        for lo, hi in ((0, half), (half, batch)):
            part = small[:(hi - lo) * per_out]
            part.fill_(0x5A5A5A5A)
            call(part, lo, hi)
            assert torch.equal(part, out[lo * per_out:hi * per_out]), (p, leaf, lo, hi)
        for e in (0, batch - 1):
            got = host(out[e * per_out:(e + 1) * per_out], dt(p))
            src = host(a[e * per_in:(e + 1) * per_in], dt(p))
            if leaf:
                want = compose_leaf(torch, plan, p, src[None, :n], src[None, n:], kt, k, beta, ell)
            else:
                want = compose_cmux(torch, plan, p, src, host(b[e * per_in:(e + 1) * per_in], dt(p)), kt, k, beta, ell)
            assert got.any() and np.array_equal(got, want), (p, leaf, e, first_difference(got, want))
        del a, b, out, ws, small
        gc.collect()
        torch.cuda.empty_cache()


# -- 6. an encrypted table lookup ------------------------------------------------------------------------------------------------------------
def noisy_ggsw(rng, p, S, NS, bit, n, beta, ell):
    """GGSW(bit) under the binary key S (k = 1), coefficient domain: row (q, l) = (A, A (*) S + e) with |e| < 2^10 and
    bit * 2^(64 - beta l) added to polynomial q"""
    rows = 2 * ell
    A = random_words(rng, p, rows * n).reshape(rows, n).astype(object)
    body = times_binary(A, NS) + rng.integers(-2 ** 10 + 1, 2 ** 10, size=(rows, n)).astype(object)
    for q in range(2):
        for l in range(1, ell + 1):
            (A if q == 0 else body)[q * ell + l - 1, 0] += bit << (64 - beta * l)
    return np.stack([(A % p).astype(np.uint64), (body % p).astype(np.uint64)], axis=1).reshape(-1)


@pytest.mark.parametrize("m", [4, 16])
def test_every_address_of_an_encrypted_lookup_decodes(m):
    """PM64 (W = 64), n = 256, k = 1, binary key, base_log 16, levels 4 (base_log * levels = 64: no rounding): a random table of M * 256
    3-bit entries at steps of floor(p / 8), log2 M + 8 address bits as noisy GGSWs (|e| < 2^10).  cmux_tree_batch over the top log2 M
    bits, blind_rotate_batch with rot_t[i] = 2n - 2^i over the low 8, sample_extract_batch(index 0): EVERY address decodes to its entry.
    Error bound: the table is noise-free.  Each CMux adds at most (k + 1) n levels (B / 2) 2^10 = 2 * 2^8 * 2^2 * 2^15 * 2^10 = 2^36 and
    passes on at most the larger of its inputs' noise; the log2 M tree stages and the log2 n = 8 rotations are each one CMux.  So the
    error is below (log2 M + log2 n) * 2^36 < 2^40, asserted; half a message step is about 2^60."""
    torch = _torch()
    p, n, k, beta, ell = PM64, 256, 1, 16, 4
    logn, depth = 8, m.bit_length() - 1
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cmux-lookup", m))
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    # GGSW(0) and GGSW(1) of every address bit, in the NTT domain: bit i of the address uses G[i][its value]
    G = [[key_ntt(torch, plan, noisy_ggsw(rng, p, S, NS, bit, n, beta, ell)) for bit in (0, 1)] for _ in range(logn + depth)]
    entries = rng.integers(0, 8, size=(m, n))
    table = dev(torch, (entries.astype(object) * (p // 8)).astype(np.uint64).reshape(-1))
    rot_t = dev(torch, np.array([2 * n - (1 << i) for i in range(logn)] + [0], dtype=np.uint32))
    accs = torch.zeros(m * n * (k + 1) * n, dtype=torch.int64, device="cuda")
    ws_tree = torch.zeros(max(plan.cmux_tree_workspace_bytes(m, k, ell, 1), 16), dtype=torch.uint8, device="cuda")
    ws_rot = torch.zeros(plan.pbs_workspace_bytes(logn, k, ell, 1), dtype=torch.uint8, device="cuda")
    glwe = torch.zeros((k + 1) * n, dtype=torch.int64, device="cuda")
    low = [torch.cat([G[i][(a >> i) & 1] for i in range(logn)]) for a in range(n)]
    for hi in range(m):
        plan.cmux_tree_batch(glwe, table, torch.cat([G[logn + i][(hi >> i) & 1] for i in range(depth)]), m, k, beta, ell, workspace=ws_tree)
        for lo in range(n):
            a = hi * n + lo
            plan.blind_rotate_batch(accs[a * (k + 1) * n:(a + 1) * (k + 1) * n], glwe, rot_t, low[lo], logn, k, beta, ell, workspace=ws_rot,
                                    lut_per_element=True)
    lwe = torch.zeros(m * n * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.sample_extract_batch(lwe, accs, k, 0)
    torch.cuda.synchronize()
    rows = host(lwe, np.uint64).reshape(m * n, n + 1)
    lo32, hi32 = (rows[:, :n] & np.uint64(0xFFFFFFFF)).astype(np.int64), (rows[:, :n] >> np.uint64(32)).astype(np.int64)
    dot = lo32.dot(S).astype(object) + hi32.dot(S).astype(object) * (1 << 32)
    phase = (rows[:, n].astype(object) - dot) % p
    dec = [int((8 * int(x) + p // 2) // p) % 8 for x in phase]
    want = entries.reshape(-1).tolist()
    assert len(set(want)) == 8 and dec == want, (m, [i for i, (x, y) in enumerate(zip(dec, want)) if x != y][:8])
    err = [(int(x) - y * (p // 8)) % p for x, y in zip(phase, want)]
    worst = max(min(e, p - e) for e in err)
    print("lookup M = %d: worst error 2^%.2f over %d addresses" % (m, np.log2(max(worst, 1)), m * n))
    assert worst < 1 << 40


# -- 7. the C example ------------------------------------------------------------------------------------------------------------------------
def test_lookup_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "lookup_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "lookup_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "every looked-up entry decoded" in r.stdout, r.stdout
