"""The multi-bit blind rotation and bootstrap of the prime plans (include/cntt_prime_multibit.h) on the MI355X.  Bit-exact:
cntt_prime*_multibit_accumulate_batch against the big-integer model of tests/prime_multibit_model.py for every arithmetic class -- the
strict-range primes whose Barrett products wrap included, since the kernel's products are exact; the blind rotation against the
composition of public calls and against the ring model; the bootstrap against its three steps; workspace, graph capture, host path,
refusals.  The 32-bit plans start at n = 32, so the smallest size is n = 16 on 64-bit words and n = 32 on 32-bit words (four and eight
16-byte vectors per polynomial)."""
import ctypes

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd._lib import EINVAL
from prime_multibit_model import model_accumulate, model_multibit_rotate, subset_exponents, monomial_ntt
from test_gpu_prime_pbs import ALL, PW31, PW63, _torch, dev, dt, host, is64, key_ntt, make_plan, random_words, seed, zeros
from test_prime_pbs_model import P30, P32, P62, PM64, wbits

pytestmark = pytest.mark.gpu


def psi_of(plan):
    return int(plan.info().root)


def special_words(rng, p, count):
    a = random_words(rng, p, count)
    a[:3] = [0, 1, p - 1]
    a[-3:] = [p - 1, 0, 1]
    return a


def group_rows(rng, n, g, batch):
    """g x batch exponents: 0, n and 2n - 1 appear, and in element 0 every row is 2n - 1, so every subset sum of two or more wraps 2n"""
    rows = rng.integers(0, 2 * n, size=(g, batch), dtype=np.uint32)
    rows[:, 0] = 2 * n - 1
    if batch > 1:
        rows[:, 1] = [(0, n, 2 * n - 1, 1)[i] for i in range(g)]
    return rows.reshape(-1)


def run_accumulate(torch, plan, p, n, nterms, nout, g, batch, rng):
    terms = special_words(rng, p, batch * nterms * n)
    key = special_words(rng, p, (nterms * nout << g) * n)
    rows = group_rows(rng, n, g, batch)
    out = zeros(torch, p, batch * nout * n)
    plan.multibit_accumulate_batch(out, dev(torch, terms), dev(torch, rows), dev(torch, key), nterms, nout, g)
    torch.cuda.synchronize()
    return terms, key, rows, host(out, dt(p))


# -- 1. the kernel alone against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("p,n", [(P62, 16), (P62, 64), (P30, 32), (P30, 64)])
def test_accumulate_matches_model(p, n, g):
    torch = _torch()
    plan = make_plan(p, n)
    psi = psi_of(plan)
    for nterms, nout in [(j, o) for j in (1, 3, 8) for o in (1, 2, 5)]:
        for batch in (1, 3):
            rng = np.random.default_rng(seed("mbacc", p, n, g, nterms, nout, batch))
            terms, key, rows, got = run_accumulate(torch, plan, p, n, nterms, nout, g, batch, rng)
            want = model_accumulate(terms.tolist(), key.tolist(), rows.tolist(), psi, n, p, nterms, nout, g, batch)
            assert [int(x) for x in got] == want, (p, n, g, nterms, nout, batch)


@pytest.mark.parametrize("p,n", [(P62, 16), (P30, 32)])
def test_accumulate_over_a_second_trip_of_the_grid(p, n):
    """a batch one element and a ragged tail past what the launcher's largest grid covers in one trip (cntt_prime_multibit_grid), so
    the grid-stride loop runs again; the model replays the first elements, those on both sides of the trip boundary and the last"""
    torch = _torch()
    plan = make_plan(p, n)
    grid = cntt.lib().cntt_prime_multibit_grid
    cap = grid(1 << 40)
    assert grid(cap * 256) == cap and grid(cap * 256 - 256) == cap - 1
    vpp = n * (8 if is64(p) else 4) // 16
    g, nterms, nout = 2, 2, 1
    edge = cap * 256 // (vpp * nout)
    batch = edge + 3
    rng = np.random.default_rng(seed("mbtrip", p))
    terms, key, rows, got = run_accumulate(torch, plan, p, n, nterms, nout, g, batch, rng)
    psi = psi_of(plan)
    T, R, O = terms.reshape(batch, nterms * n), rows.reshape(g, batch), got.reshape(batch, nout * n)
    for b in (0, 1, edge - 1, edge, edge + 1, batch - 1):
        want = model_accumulate(T[b].tolist(), key.tolist(), R[:, b].tolist(), psi, n, p, nterms, nout, g, 1)
        assert [int(x) for x in O[b]] == want, (p, b)
    # every element against a vectorised replay of the same formula where the products fit 64 bits
    if not is64(p):
        K = key.reshape(1 << g, nterms, n).astype(np.uint64)
        Tn = terms.reshape(batch, nterms, n).astype(np.uint64)
        mono = np.array([monomial_ntt(e, psi, n, p) for e in range(2 * n)], dtype=np.uint64)
        acc = np.zeros((batch, n), dtype=np.uint64)
        for t in range(1 << g):
            e = np.zeros(batch, dtype=np.int64)
            for i in range(g):
                if (t >> i) & 1:
                    e += R[i].astype(np.int64)
            s = np.zeros((batch, n), dtype=np.uint64)
            for j in range(nterms):
                s = (s + Tn[:, j] * K[t, j] % p) % p
            acc = (acc + s * mono[e % (2 * n)] % p) % p
        assert np.array_equal(acc.astype(np.uint32), O)


# -- 2. every arithmetic class, the primes whose Barrett products wrap included ----------------------------------------------------------
@pytest.mark.parametrize("p", ALL)
def test_accumulate_is_exact_in_every_arithmetic_class(p):
    assert PW63 in ALL and PW31 in ALL
    torch = _torch()
    n, g, nterms, nout, batch = 64, 2, 4, 2, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("mbclass", p))
    terms, key, rows, got = run_accumulate(torch, plan, p, n, nterms, nout, g, batch, rng)
    want = model_accumulate(terms.tolist(), key.tolist(), rows.tolist(), psi_of(plan), n, p, nterms, nout, g, batch)
    assert [int(x) for x in got] == want, p


# -- 3. the blind rotation ----------------------------------------------------------------------------------------------------------------
def rot_table(rng, n, L, batch):
    rot = rng.integers(0, 2 * n, size=(L + 1, batch), dtype=np.uint32)
    rot[:, 0] = 2 * n - 1
    return rot.reshape(-1)


def composition(torch, plan, p, n, lut_t, rot_t, bsk, L, k, beta, ell, g, batch):
    """the public calls the header names, group by group"""
    J = (k + 1) * ell
    acc = zeros(torch, p, batch * (k + 1) * n)
    plan.blind_rotate_batch(acc, lut_t, rot_t[L * batch:], bsk[:0], 0, k, beta, ell)          # the set-up: X^(body) lut
    terms, nxt = zeros(torch, p, batch * J * n), zeros(torch, p, batch * (k + 1) * n)
    size = (J * (k + 1) << g) * n
    for r in range(L // g):
        plan.gadget_decompose_batch(terms, acc, beta, ell)
        plan.fwd_batch(terms)
        plan.multibit_accumulate_batch(nxt, terms, rot_t[r * g * batch:(r + 1) * g * batch], bsk[r * size:(r + 1) * size], J, k + 1, g)
        plan.inv_batch(nxt)
        acc, nxt = nxt, acc
    return acc


def settings_of(p):
    W = wbits(p)
    return [(4, 3), (W, 1)] + ([(16, 4)] if W == 64 else [])


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("p,n", [(PM64, 16), (PW63, 64), (P30, 32)])
def test_blind_rotate_equals_the_public_calls_and_the_model(p, n, g, k):
    torch = _torch()
    plan = make_plan(p, n)
    G, batch = 2, 2
    L = G * g
    for si, (beta, ell) in enumerate(settings_of(p)):
        per_element = (si + g + k) % 2 == 1
        rng = np.random.default_rng(seed("mbrot", p, n, g, k, beta, ell))
        lut = random_words(rng, p, (batch if per_element else 1) * (k + 1) * n)
        rot = rot_table(rng, n, L, batch)
        key = random_words(rng, p, (G * (k + 1) * ell * (k + 1) << g) * n)
        lut_t, rot_t, bsk = dev(torch, lut), dev(torch, rot), key_ntt(torch, plan, key)
        acc = zeros(torch, p, batch * (k + 1) * n)
        plan.multibit_blind_rotate_batch(acc, lut_t, rot_t, bsk, L, k, beta, ell, g, lut_per_element=per_element)
        ref = composition(torch, plan, p, n, lut_t, rot_t, bsk, L, k, beta, ell, g, batch)
        torch.cuda.synchronize()
        got = host(acc, dt(p))
        assert got.any() and np.array_equal(got, host(ref, dt(p))), (p, n, g, k, beta, ell)
        if n <= 32 or (g <= 2 and k == 1):
            want = model_multibit_rotate(lut.tolist(), rot.tolist(), key.tolist(), p, n, L, k, beta, ell, g, batch, per_element)
            assert [int(x) for x in got] == want, (p, n, g, k, beta, ell)
        if si == 0 and (g, k) == (2, 1):
            # the same words with a caller workspace on the device and through the host path with and without one; then no group at
            # all (lwe_dim = 0: the set-up alone, a workspace the call does not touch) on the same three paths and without one
            for Lf, want_t in ((L, acc), (0, composition(torch, plan, p, n, lut_t, rot_t[L * batch:], bsk, 0, k, beta, ell, g, batch))):
                rot_f, nws = rot_t[(L - Lf) * batch:], plan.multibit_pbs_workspace_bytes(Lf, k, ell, g, batch)
                key_f = bsk if Lf else bsk[:0]
                for where, with_ws in (("device", False), ("device", True), ("host", False), ("host", True)):
                    if where == "host":
                        out = np.zeros(batch * (k + 1) * n, dtype=dt(p))
                        plan.multibit_blind_rotate_batch(out, lut, host(rot_f, np.uint32).copy(), host(key_f, dt(p)).copy(), Lf, k, beta, ell, g,
                                                         workspace=np.zeros(nws, dtype=np.uint8) if with_ws else None, lut_per_element=per_element)
                    else:
                        out_t = zeros(torch, p, batch * (k + 1) * n)
                        ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
                        plan.multibit_blind_rotate_batch(out_t, lut_t, rot_f, key_f, Lf, k, beta, ell, g, workspace=ws, lut_per_element=per_element)
                        torch.cuda.synchronize()
                        out = host(out_t, dt(p))
                    assert np.array_equal(out, host(want_t, dt(p))), (p, n, Lf, where, with_ws)


def test_blind_rotate_past_a_wavefront_resident_transform():
    """n = 4096 on 64-bit words, batch 2, L = 4, g = 2: the whole call against one group through the call followed by the model's
    pointwise step on the last group (the digits and the transforms around it are the public calls)"""
    torch = _torch()
    p, n, k, beta, ell, g, L, batch = P62, 4096, 1, 31, 2, 2, 4, 2
    J = (k + 1) * ell
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("mb4096"))
    lut = dev(torch, random_words(rng, p, (k + 1) * n))
    rot = rot_table(rng, n, L, batch)
    rot_t = dev(torch, rot)
    bsk = key_ntt(torch, plan, random_words(rng, p, (2 * J * (k + 1) << g) * n))
    whole, first = zeros(torch, p, batch * (k + 1) * n), zeros(torch, p, batch * (k + 1) * n)
    plan.multibit_blind_rotate_batch(whole, lut, rot_t, bsk, L, k, beta, ell, g)
    head = dev(torch, np.concatenate([rot[:g * batch], rot[L * batch:]]))
    size = (J * (k + 1) << g) * n
    plan.multibit_blind_rotate_batch(first, lut, head, bsk[:size], g, k, beta, ell, g)
    terms = zeros(torch, p, batch * J * n)
    plan.gadget_decompose_batch(terms, first, beta, ell)
    plan.fwd_batch(terms)
    torch.cuda.synchronize()
    last = model_accumulate(host(terms, np.uint64).tolist(), host(bsk[size:], np.uint64).tolist(), rot[g * batch:2 * g * batch].tolist(),
                            psi_of(plan), n, p, J, k + 1, g, batch)
    nxt = dev(torch, np.array(last, dtype=np.uint64))
    plan.inv_batch(nxt)
    torch.cuda.synchronize()
    assert whole.any() and torch.equal(whole, nxt)


# -- 4. bootstrap == its three steps; workspace and NULL; host path ---------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,where,with_ws", [(P62, 1024, "device", True), (P62, 1024, "device", False), (PM64, 64, "host", True),
                                               (P30, 64, "host", False), (P32, 2048, "device", True)])
def test_bootstrap_equals_its_three_steps(p, n, where, with_ws):
    check_bootstrap_steps(p, n, where, with_ws, L=6, batch=5)


@pytest.mark.parametrize("p,where,with_ws", [(P62, "device", True), (P62, "device", False), (P30, "host", True)])
def test_bootstrap_without_mask_words_equals_its_three_steps(p, where, with_ws):
    """lwe_dim = 0: no group, no key, and of the workspace only rot_t and the accumulator"""
    check_bootstrap_steps(p, 64, where, with_ws, L=0, batch=2)


def check_bootstrap_steps(p, n, where, with_ws, L, batch):
    torch = _torch()
    plan = make_plan(p, n)
    k, beta, ell, g = 1, 7, 3, 3 if n == 64 else 2
    rng = np.random.default_rng(seed("mbboot", p, n, where))
    lwe_a = random_words(rng, p, batch * (L + 1))
    lut_a = random_words(rng, p, (k + 1) * n)
    key_a = random_words(rng, p, ((L // g) * (k + 1) * ell * (k + 1) << g) * n)
    nbytes = plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch)
    assert nbytes == plan.pbs_workspace_bytes(L, k, ell, batch)
    if where == "host":
        to, fro = (lambda a: a.copy()), (lambda a, d: a)
        ws = np.zeros(nbytes, dtype=np.uint8) if with_ws else None
    else:
        to, fro = (lambda a: dev(torch, a)), host
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if with_ws else None      # exactly the figure, not a byte more
    lwe_t, lut_t, bsk = to(lwe_a), to(lut_a), to(key_a)
    one = to(np.zeros(batch * (k * n + 1), dtype=dt(p)))
    plan.multibit_bootstrap_batch(one, lwe_t, lut_t, bsk, L, k, beta, ell, g, workspace=ws)
    rot_t = to(np.zeros((L + 1) * batch, dtype=np.uint32))
    acc = to(np.zeros(batch * (k + 1) * n, dtype=dt(p)))
    steps = to(np.zeros(batch * (k * n + 1), dtype=dt(p)))
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    plan.multibit_blind_rotate_batch(acc, lut_t, rot_t, bsk, L, k, beta, ell, g, workspace=ws)
    plan.sample_extract_batch(steps, acc, k, 0)
    if where == "device":
        torch.cuda.synchronize()
    assert np.array_equal(fro(one, dt(p)), fro(steps, dt(p))), (p, n, where, with_ws)
    assert fro(one, dt(p)).any()


# -- 5. graph capture at a size the classic call cannot capture ----------------------------------------------------------------------------
def test_graph_capture_at_n_4096_with_a_caller_workspace():
    torch = _torch()
    p, n, L, k, beta, ell, g, batch = P62, 4096, 4, 1, 8, 3, 2, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(17)
    lwe = dev(torch, random_words(rng, p, batch * (L + 1)))
    lut = dev(torch, random_words(rng, p, (k + 1) * n))
    bsk = dev(torch, random_words(rng, p, ((L // g) * (k + 1) * ell * (k + 1) << g) * n))
    ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch), dtype=torch.uint8, device="cuda")
    eager = zeros(torch, p, batch * (k * n + 1))
    plan.multibit_bootstrap_batch(eager, lwe, lut, bsk, L, k, beta, ell, g, workspace=ws)     # also builds the plan's tables
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # a linear chain of kernels: no allocation and no copy with a caller workspace
        plan.multibit_bootstrap_batch(out, lwe, lut, bsk, L, k, beta, ell, g, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(first, eager) and torch.equal(out, eager)


# -- 6. the bootstrap bootstraps ------------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


@pytest.mark.parametrize("g", [2, 3])
def test_bootstrap_evaluates_the_table_on_encrypted_messages(g):
    """p = 2^64 - 2^32 + 1, n = 1024, k = 1, L = 12, base_log 8, levels 4; binary keys.  Key (r, t), row (q, l): a GLWE encryption of
    zero (uniform mask, body = mask * S + e, |e| < 2^10 from this test's generator) plus [t == the group's secret pattern] times
    2^(W - base_log l) on coefficient 0 of polynomial q.  Four messages under one padding bit, enc(m) = round(m p / 8), the table
    X^(-n/8) v0 with boxes of n / 4 coefficients, input noise below 2^20.

    Why the decoding must succeed.  Box selection as in the classic test: the exponent sum errs by at most (L + 1) / 2 + 2 < 128.  The
    phase error of one group step: the gadget rounding, at most (1 + k n) 2^(s-1) with s = 64 - 32; and the key noise, every one of
    the 2^g J rows contributing a digit polynomial (|d| <= 2^7) times a noise polynomial (< 2^10): below 2^g J n 2^17.  Over
    G = L / g steps: G ((1 + n) 2^31 + 2^g 8 n 2^17) < 6 (2^41 + 2^33) < 2^44, far below the decoding margin p / 16 > 2^59."""
    torch = _torch()
    p, n, k, beta, ell, L, reps = PM64, 1024, 1, 8, 4, 12, 2
    W, G, J = 64, L // g, (k + 1) * ell
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("mbfunctional", g))
    s = [int(x) for x in rng.integers(0, 2, size=L)]
    S = rng.integers(0, 2, size=k * n).astype(np.uint64)
    shape = (G, 1 << g, J, k + 1, n)
    key = np.zeros(shape, dtype=np.uint64)
    key[..., :k, :] = random_words(rng, p, G * (J << g) * k * n).reshape(G, 1 << g, J, k, n)
    S_ntt = dev(torch, np.ascontiguousarray(np.broadcast_to(S.reshape(1, 1, 1, k, n), (G, 1 << g, J, k, n))).reshape(-1))
    plan.fwd_batch(S_ntt)
    prod = dev(torch, np.ascontiguousarray(key[..., :k, :]).reshape(-1))
    plan.mul_ntt_batch(prod, S_ntt)
    torch.cuda.synchronize()
    body = host(prod, np.uint64).reshape(G, 1 << g, J, k, n).astype(object).sum(axis=3)
    body = (body + rng.integers(-2 ** 10 + 1, 2 ** 10, size=body.shape).astype(object)) % p
    for r in range(G):
        pattern = sum(s[r * g + i] << i for i in range(g))
        for q in range(k + 1):
            for l in range(1, ell + 1):
                j = q * ell + l - 1
                if q == k:
                    body[r, pattern, j, 0] = (body[r, pattern, j, 0] + pow(2, W - beta * l, p)) % p
                else:
                    key[r, pattern, j, q, 0] = (int(key[r, pattern, j, q, 0]) + pow(2, W - beta * l, p)) % p
    key[..., k, :] = body.astype(np.uint64)
    bsk = key_ntt(torch, plan, key.reshape(-1))

    def enc(m):
        return (2 * m * p + 8) // 16          # round(m p / 8)

    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = enc(pbs_f((t % n) // (n // 4)))
        lut[k * n + j] = v if t < n else (-v) % p
    msgs = [m for _ in range(reps) for m in range(4)]
    batch = len(msgs)
    a = random_words(rng, p, batch * L).reshape(batch, L)
    noise = [int(x) for x in rng.integers(-2 ** 20 + 1, 2 ** 20, size=batch)]
    lwe_in = np.zeros((batch, L + 1), dtype=np.uint64)
    lwe_in[:, :L] = a
    for b in range(batch):
        lwe_in[b, L] = (sum(int(a[b, i]) * s[i] for i in range(L)) + enc(msgs[b]) + noise[b]) % p
    lwe_out = zeros(torch, p, batch * (k * n + 1))
    plan.multibit_bootstrap_batch(lwe_out, dev(torch, lwe_in.reshape(-1)), dev(torch, lut), bsk, L, k, beta, ell, g)
    torch.cuda.synchronize()
    ct = host(lwe_out, np.uint64).reshape(batch, k * n + 1)
    Si = [int(x) for x in S]
    worst = 0
    for b in range(batch):
        phase = (int(ct[b, k * n]) - sum(int(x) * y for x, y in zip(ct[b, :k * n], Si))) % p
        err = (phase - enc(pbs_f(msgs[b]))) % p
        worst = max(worst, min(err, p - err))
        assert ((16 * phase + p) // (2 * p)) % 8 == pbs_f(msgs[b]), (g, b, msgs[b], phase)
    print("g = %d: largest |phase error| = 2^%.1f" % (g, np.log2(max(worst, 1))))
    assert worst < 1 << 44, worst


# -- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def ptr(a):
    return None if a is None else ctypes.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


@pytest.mark.parametrize("bits,p", [(64, P62), (32, P30)])
def test_every_refusal_leaves_the_outputs_untouched(bits, p):
    """host buffers: every case is refused by the argument checks that precede any device call"""
    n, L, k, beta, ell, g, batch = 64, 4, 1, 4, 3, 2, 2
    plan = make_plan(p, n)
    W, d = wbits(p), dt(p)
    J = (k + 1) * ell
    POISON = 7
    big = np.full(1 << 16, POISON, dtype=d)
    acc, lwe_out = big[:batch * (k + 1) * n], big[4096:4096 + batch * (k * n + 1)]
    out_ntt = big[8192:8192 + batch * (k + 1) * n]
    lut = np.zeros((k + 1) * n, dtype=d)
    rot = np.zeros((L + 1) * batch, dtype=np.uint32)
    lwe_in = np.zeros(batch * (L + 1), dtype=d)
    key = np.zeros(((L // g) * J * (k + 1) << g) * n, dtype=d)
    terms = np.zeros(batch * J * n, dtype=d)
    nbytes = plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch)
    ws = np.zeros(nbytes + 32, dtype=np.uint8)
    off = (-ws.ctypes.data) % 16
    good, odd = ws[off:off + nbytes], ws[off + 4:off + 4 + nbytes]
    lib = cntt.lib()
    rot_fn = getattr(lib, "cntt_prime%d_multibit_blind_rotate_batch" % bits)
    boot_fn = getattr(lib, "cntt_prime%d_multibit_bootstrap_batch" % bits)
    acc_fn = getattr(lib, "cntt_prime%d_multibit_accumulate_batch" % bits)

    def rotate(plan_=plan._h, acc_=acc, lut_=lut, rot_=rot, key_=key, L_=L, beta_=beta, ell_=ell, g_=g, ws_=None, wsb=None):
        return rot_fn(plan_, ptr(acc_), ptr(lut_), 0, ptr(rot_), ptr(key_), L_, k, beta_, ell_, g_, batch, ptr(ws_),
                      (0 if ws_ is None else ws_.nbytes) if wsb is None else wsb, 0, None)

    def boot(out_=lwe_out, in_=lwe_in, lut_=lut, key_=key, L_=L, beta_=beta, ell_=ell, g_=g, ws_=None, wsb=None):
        return boot_fn(plan._h, ptr(out_), ptr(in_), ptr(lut_), 0, ptr(key_), L_, k, beta_, ell_, g_, batch, ptr(ws_),
                       (0 if ws_ is None else ws_.nbytes) if wsb is None else wsb, 0, None)

    def accumulate(out_=out_ntt, terms_=terms, rot_=rot[:g * batch], key_=key[:(J * (k + 1) << g) * n], g_=g):
        return acc_fn(plan._h, ptr(out_), ptr(terms_), ptr(rot_), ptr(key_), J, k + 1, g_, batch, 0, None)

    bad_rot = rot.copy()
    bad_rot[3] = 2 * n
    cases = [
        (lambda: rotate(plan_=None), "plan"), (lambda: rotate(beta_=0), "base_log is 0"), (lambda: rotate(ell_=0), "levels is 0"),
        (lambda: rotate(beta_=W, ell_=2), "exceeds the bit length"), (lambda: rotate(g_=0), "grouping"), (lambda: rotate(g_=5), "grouping"),
        (lambda: rotate(L_=5), "multiple of grouping"), (lambda: rotate(acc_=None), "acc"), (lambda: rotate(lut_=None), "lut"),
        (lambda: rotate(rot_=None), "rot_t"), (lambda: rotate(key_=None), "bsk_mb"),
        (lambda: rotate(lut_=big[8:8 + lut.size]), "acc overlaps lut"), (lambda: rotate(key_=big[8:8 + key.size]), "acc overlaps bsk_mb"),
        (lambda: rotate(rot_=big.view(np.uint32)[8:8 + rot.size]), "acc overlaps rot_t"),
        (lambda: rotate(ws_=big.view(np.uint8)[:nbytes]), "overlaps"), (lambda: rotate(ws_=odd), "aligned"),
        (lambda: rotate(ws_=good, wsb=batch * J * n * d().itemsize - 1), "workspace_bytes"), (lambda: rotate(rot_=bad_rot), "rot_t[3]"),
        (lambda: boot(beta_=0), "base_log is 0"), (lambda: boot(g_=7), "grouping"), (lambda: boot(L_=3), "multiple of grouping"),
        (lambda: boot(out_=None), "lwe_out"), (lambda: boot(in_=None), "lwe_in"), (lambda: boot(lut_=None), "lut"),
        (lambda: boot(key_=None), "bsk_mb"), (lambda: boot(in_=big[4096 + 8:4096 + 8 + lwe_in.size]), "lwe_out overlaps lwe_in"),
        (lambda: boot(ws_=odd), "aligned"), (lambda: boot(ws_=good, wsb=nbytes - 1), "workspace_bytes"),
        (lambda: accumulate(g_=0), "grouping"), (lambda: accumulate(g_=5), "grouping"), (lambda: accumulate(out_=None), "out_ntt"),
        (lambda: accumulate(terms_=None), "terms_ntt"), (lambda: accumulate(rot_=None), "rot_rows"),
        (lambda: accumulate(key_=None), "key_group"), (lambda: accumulate(terms_=big[8192 + 8:8192 + 8 + terms.size]), "out_ntt overlaps terms_ntt"),
        (lambda: accumulate(rot_=bad_rot[:g * batch]), "rot_rows[3]"),
    ]
    for i, (call, word) in enumerate(cases):
        assert call() == EINVAL, (i, word)
        assert word in lib.cntt_last_error().decode(), (i, word, lib.cntt_last_error().decode())
        assert (big == POISON).all(), (i, word)
    # batch == 0 does nothing; lwe_dim == 0 writes the rotated table only and needs no key
    assert rot_fn(plan._h, None, None, 0, None, None, L, k, beta, ell, g, 0, None, 0, 0, None) == 0
    table = np.arange((k + 1) * n, dtype=d)
    plan.multibit_blind_rotate_batch(acc, table, np.zeros(batch, dtype=np.uint32), key[:0], 0, k, beta, ell, g)
    assert np.array_equal(acc, np.tile(table, batch))


# -- 8. the C example -----------------------------------------------------------------------------------------------------------------------
def test_pbs_multibit_prime_example_builds_and_runs():
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["make", "-s", "-C", os.path.join(root, "examples"), "pbs_multibit_prime"], check=True)
    r = subprocess.run([os.path.join(root, "examples", "pbs_multibit_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 4 and not any("WRONG" in ln for ln in lines), r.stdout
