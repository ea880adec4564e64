"""The LWE-to-GLWE packing keyswitch of the prime plans (include/cntt_prime_pack.h) on the MI355X.  Bit-exact throughout, no tolerance
anywhere: the call against the plain-int model of tests/prime_pack_model.py (which tests/test_prime_pack_abi.py checks against the
header's formula and its phase identity) on shapes that cross every tile and chunk edge and on deterministic worst cases; against the
sequence of public calls the header states, for every prime class (the strict-range primes whose Barrett product wraps included);
against the direct route through cntt_prime*_keyswitch_batch; on encrypted messages and on the outputs of a bootstrap; graph capture;
with and without a caller workspace; the C example."""
import os
import subprocess

import numpy as np
import pytest

from prime_pack_model import C, TI, TT, model_pack_batch
from test_gpu_prime_pbs import ALL, EXACT, _torch, dev, dt, host, is64, key_ntt, make_plan, random_words, seed
from test_prime_pbs_model import P30, P32, P62, PM64, signed_digits, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5A5A5A5A5A5A5A5


def tdtype(torch, p):
    return torch.int64 if is64(p) else torch.int32


def run_pack(torch, plan, p, where, lwe_a, key_a, lin, m, k, beta, ell, batch, with_ws=False):
    """the call on word arrays (ciphertexts, coefficient-domain key) -> the output array; the output buffer starts out poisoned"""
    n = plan.ntt_size()
    kt = key_ntt(torch, plan, key_a) if lin else torch.empty(0, dtype=tdtype(torch, p), device="cuda")
    torch.cuda.synchronize()
    poison = np.full(batch * (k + 1) * n, POISON & (2 ** (8 * np.dtype(dt(p)).itemsize) - 1), dtype=dt(p))
    nws = plan.pack_workspace_bytes(lin, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.pack_keyswitch_batch(poison, lwe_a, host(kt, dt(p)).copy(), lin, m, k, beta, ell, workspace=ws)
        return poison
    out = dev(torch, poison)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.pack_keyswitch_batch(out, dev(torch, lwe_a), kt, lin, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out, dt(p))


def compose(torch, plan, p, lwe_a, key_a, lin, m, k, beta, ell, batch):
    """The header's sequence of public calls: out = the body polynomial; per chunk a numpy transpose into the polynomials P_i,
    gadget_decompose_batch(plain), the digits negated mod p on the host, external_product_batch(accumulate=True)."""
    n = plan.ntt_size()
    lw = lwe_a.reshape(batch, m, lin + 1)
    out = np.zeros((batch, k + 1, n), dtype=dt(p))
    out[:, k, :m] = lw[:, :, lin]
    out_t = dev(torch, out.reshape(-1))
    kt = key_ntt(torch, plan, key_a) if lin else None
    c = min(C(ell), lin)
    for i0 in range(0, lin, max(c, 1)):
        nw = min(c, lin - i0)
        polys = np.zeros((batch, nw, n), dtype=dt(p))
        polys[:, :, :m] = lw[:, :, i0:i0 + nw].transpose(0, 2, 1)
        terms = torch.zeros(batch * nw * ell * n, dtype=tdtype(torch, p), device="cuda")
        plan.gadget_decompose_batch(terms, dev(torch, polys.reshape(-1)), beta, ell, mode="plain")
        torch.cuda.synchronize()
        t = host(terms, dt(p))
        neg = np.where(t == 0, t, dt(p)(p) - t)
        plan.external_product_batch(out_t, dev(torch, neg), kt[i0 * ell * (k + 1) * n:(i0 + nw) * ell * (k + 1) * n], nw * ell, k + 1,
                                    accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def model(p, lwe_a, key_a, lin, m, k, n, beta, ell, batch):
    return np.array(model_pack_batch(lwe_a.tolist(), key_a.tolist(), p, lin, m, k, n, beta, ell, batch), dtype=dt(p))


def first_difference(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return (int(bad[0]), hex(int(got[bad[0]])), hex(int(want[bad[0]])), int(bad.size)) if bad.size else None


# -- 1. the call against the model across every tile and chunk edge ------------------------------------------------------------------------
def shapes(p):
    """(n, batch, m, lin, k, beta, ell).  n = 32: m 1 / inside / n; lin 0, 1, one below and above the tile TI, one below and above the
    chunk C, 2 C + 3; k 1 / 2; batch 1 / 3; base_log 1 and 31 (the bit length where the modulus has fewer than 31 bits), one digit as
    wide as the modulus (sh1 = 0).  n = 128: m one below and above the tile TT, and n (two tiles along t).  Where W is the word width,
    base_log * levels = W exactly."""
    W = wbits(p)
    wide = min(31, W)
    out = [(32, 1, 1, 0, 1, 5, 3),
           (32, 3, 32, 1, 2, W // 4, 4),
           (32, 1, 31, TI - 1, 1, 5, 3),
           (32, 3, 32, TI + 1, 2, 4, 3),
           (32, 1, 7, C(1) - 1, 1, wide, 1),
           (32, 1, 32, C(7) + 1, 2, 1, 7),
           (32, 3, 5, 2 * C(2) + 3, 1, 6, 2),
           (32, 1, 3, 2, 1, W, 1),
           (128, 1, TT - 1, 3, 1, 5, 3),
           (128, 2, TT + 1, TI + 1, 1, 4, 3),
           (128, 1, 128, 2, 2, W // 4, 4)]
    if W in (32, 64):
        out += [(32, 1, 9, 3, 1, 8, W // 8)]
    return out


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", [PM64, P32, P62, P30])
def test_pack_matches_model(p, where):
    torch = _torch()
    plans = {n: make_plan(p, n) for n in (32, 128)}
    for n, batch, m, lin, k, beta, ell in shapes(p):
        rng = np.random.default_rng(seed("pack", p, where, n, batch, m, lin, k, beta))
        lwe = random_words(rng, p, batch * m * (lin + 1))
        key = random_words(rng, p, lin * ell * (k + 1) * n)
        want = model(p, lwe, key, lin, m, k, n, beta, ell, batch)
        got = run_pack(torch, plans[n], p, where, lwe, key, lin, m, k, beta, ell, batch)
        assert np.array_equal(got, want), (p, where, n, batch, m, lin, k, beta, ell, "first bad word", first_difference(got, want))
        if lin == 0:                                            # the poison is gone: zero masks, zero tail of the body polynomial
            # (no chunk, no key: a workspace the caller brings is not touched, and without one the device path allocates none)
            again = run_pack(torch, plans[n], p, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=True)
            assert np.array_equal(again, want), (p, where, "lin = 0 with a workspace")
            o = got.reshape(batch, k + 1, n)
            assert not o[:, :k].any() and not o[:, k, m:].any() and np.array_equal(o[:, k, :m], lwe.reshape(batch, m))


# -- 2. every prime class against the public-call composition -----------------------------------------------------------------------------
@pytest.mark.parametrize("p", ALL)
def test_pack_equals_the_public_calls_for_every_prime_class(p):
    """n = 64 with k = 1, 2 (the fused chain) and k = 4 (five outputs: the composed external product); for the primes of EXACT also
    against the big-integer model, which the strict-range primes whose Barrett product wraps (PW63, PW31) need not meet."""
    torch = _torch()
    n, batch, m, lin, beta, ell = 64, 2, 9, TI + 2, 6, 3
    plan = make_plan(p, n)
    for k in (1, 2, 4):
        rng = np.random.default_rng(seed("classes", p, k))
        lwe = random_words(rng, p, batch * m * (lin + 1))
        key = random_words(rng, p, lin * ell * (k + 1) * n)
        got = run_pack(torch, plan, p, "device", lwe, key, lin, m, k, beta, ell, batch)
        want = compose(torch, plan, p, lwe, key, lin, m, k, beta, ell, batch)
        assert got.any() and np.array_equal(got, want), (p, k, "public calls", first_difference(got, want))
        if p in EXACT:
            want = model(p, lwe, key, lin, m, k, n, beta, ell, batch)
            assert np.array_equal(got, want), (p, k, "model", first_difference(got, want))


def test_pack_equals_the_public_calls_at_n_4096():
    """64-bit words at n = 4096: past the fused chain, the composed external product"""
    torch = _torch()
    p, n, batch, m, lin, k, beta, ell = P62, 4096, 2, 9, 3, 1, 6, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("classes", p, n))
    lwe = random_words(rng, p, batch * m * (lin + 1))
    key = random_words(rng, p, lin * ell * (k + 1) * n)
    got = run_pack(torch, plan, p, "device", lwe, key, lin, m, k, beta, ell, batch)
    want = compose(torch, plan, p, lwe, key, lin, m, k, beta, ell, batch)
    assert got.any() and np.array_equal(got, want), first_difference(got, want)


# -- 3. deterministic worst cases ---------------------------------------------------------------------------------------------------------
def worst_words(p, beta, ell):
    """{name: word} for the digit patterns the balanced lift of p reaches at this setting: `low` every lower digit -B/2 under a top
    digit +B/2; `high` every digit B/2 - 1; `bottom` the top digit -B/2 (over lower digits B/2 - 1); each asserted against digits()"""
    W, B = wbits(p), 1 << beta
    pats = {"low": [B // 2] + [-(B // 2)] * (ell - 1), "high": [B // 2 - 1] * ell, "bottom": [-(B // 2)] + [B // 2 - 1] * (ell - 1)}
    out = {}
    for name, ds in pats.items():
        v = sum(d << (W - beta * (l + 1)) for l, d in enumerate(ds))
        if abs(v) <= (p - 1) // 2:
            assert signed_digits(v % p, p, beta, ell) == ds, (p, beta, ell, name)
            out[name] = v % p
    return out


@pytest.mark.parametrize("p", [PM64, P62, P32, P30])
def test_pack_worst_cases(p):
    """Every lower digit -B/2 (stored negated: +B/2) under a top digit +B/2, every digit B/2 - 1, the top digit -B/2, and the words
    (p-1)/2, (p+1)/2, p-1 at the ends of the balanced lift, against key words p - 1 and (p+1)/2: a wrong select or a lost bit of y shows
    in every word.  Lin = C + 2, m = n = 32.  The setting (31, W // 31) exists where W >= 31."""
    torch = _torch()
    n, k, m, W = 32, 1, 32, wbits(p)
    plan = make_plan(p, n)
    reached = set()
    for beta, ell in [(4, 3), (1, 5)] + ([(31, W // 31)] if W >= 31 else []):
        lin = C(ell) + 2
        words = worst_words(p, beta, ell)
        reached |= set(words)
        words.update({"hp": (p - 1) // 2, "hp1": (p + 1) // 2, "top": p - 1})
        for name, word in words.items():
            lwe = np.full(m * (lin + 1), word, dtype=dt(p))
            for keyword in (p - 1, (p + 1) // 2):
                key = np.full(lin * ell * (k + 1) * n, keyword, dtype=dt(p))
                want = model(p, lwe, key, lin, m, k, n, beta, ell, 1)
                got = run_pack(torch, plan, p, "device", lwe, key, lin, m, k, beta, ell, 1)
                assert np.array_equal(got, want), (p, beta, ell, name, hex(keyword), first_difference(got, want))
    assert reached == {"low", "high", "bottom"}, (p, reached)


# -- 4. the NTT route and the direct route agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n", [(PM64, 1024), (P30, 1024), (P30, 8192)])
def test_pack_equals_keyswitch_rotate_and_sum(p, n):
    """n = 1024 runs the fused chain, n = 8192 on 32-bit words the composed one.  The existing keyswitch_batch on the same
    coefficient-domain key, viewed as Lin * levels rows of (k + 1) n words, gives KS(lwe_t) with the body word in the last place; moved
    to coefficient 0 of the body polynomial, rotated by X^t and summed over t mod p on the host it is the packed output, whose key is
    normalize(fwd(key))."""
    torch = _torch()
    plan = make_plan(p, n)
    m, lin, ell, beta, batch, k = 5, 20, 2, 8, 2, 1
    cols = (k + 1) * n
    rng = np.random.default_rng(seed("routes", p, n))
    lwe_a = random_words(rng, p, batch * m * (lin + 1))
    key_a = random_words(rng, p, lin * ell * cols)
    got = run_pack(torch, plan, p, "device", lwe_a, key_a, lin, m, k, beta, ell, batch).reshape(batch, k + 1, n)
    rows = torch.zeros(batch * m * cols, dtype=tdtype(torch, p), device="cuda")
    plan.keyswitch_batch(rows, dev(torch, lwe_a), dev(torch, key_a), lin, cols - 1, beta, ell)
    torch.cuda.synchronize()
    ks = host(rows, dt(p)).astype(object).reshape(batch, m, k + 1, n)
    body = lwe_a.astype(object).reshape(batch, m, lin + 1)[:, :, lin]
    ks[:, :, k, n - 1] -= body                                      # the body word leaves the last place ...
    ks[:, :, k, 0] += body                                          # ... for coefficient 0 of the body polynomial
    want = np.zeros((batch, k + 1, n), dtype=object)
    for t in range(m):                                              # + X^t KS(lwe_t)
        want[:, :, t:] += ks[:, t, :, :n - t]
        if t:
            want[:, :, :t] -= ks[:, t, :, n - t:]
    want = (want % p).astype(dt(p))
    assert got.any() and np.array_equal(got, want), (p, n, int((got != want).sum()))


# -- 5. decryption ------------------------------------------------------------------------------------------------------------------------
def negacyclic_matrix(S):
    """N with (N a)[c] = (a (*) S)[c] over the integers for a key S of 0 / 1 words: N[c][j] = S[c - j], negated past the wrap (int64)"""
    n = len(S)
    ext = np.concatenate([S, -S]).astype(np.int64)
    return ext[(np.arange(n)[:, None] - np.arange(n)[None, :]) % (2 * n)]


def times_binary(A, NS):
    """rows of A (words below 2^64) times the negacyclic matrix of a binary key, as exact Python ints: the product runs in int64 on the
    two 32-bit halves of the words (sums below n 2^32)"""
    A = A.astype(np.uint64)
    lo, hi = (A & np.uint64(0xFFFFFFFF)).astype(np.int64), (A >> np.uint64(32)).astype(np.int64)
    return lo.dot(NS.T).astype(object) + hi.dot(NS.T).astype(object) * (1 << 32)


def test_pack_decrypts_under_the_output_key():
    """PM64 (W = 64), n = 256, k = 1: 256 LWE ciphertexts of dimension 64 (3-bit messages at steps of floor(p / 8) under a binary key,
    noise below 2^40) packed under a noisy key (|e| < 2^20 per coefficient) with base_log 4, levels 6 into one GLWE ciphertext under a
    binary GLWE key.  The model's output decrypts coefficient t to message t -- asserted first, on the CPU -- and the device and host
    words are the model's.  Error per coefficient: the rounding of 64 mask words to 24 bits (s = 40), at most 64 * 2^39 = 2^45; the key
    noise, 64 * 6 rows times 256 digit coefficients of at most 8 times 2^20, below 2^40; the ciphertext's own noise, below 2^40:
    together far below the floor(p / 16) ~ 2^60 that half a message step allows."""
    torch = _torch()
    p, n, k, lin, m, beta, ell = PM64, 256, 1, 64, 256, 4, 6
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("decrypt"))
    s_in = rng.integers(0, 2, size=lin).astype(np.int64)
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    rows = lin * ell
    A = random_words(rng, p, rows * n).reshape(rows, n)
    body = times_binary(A, NS) + rng.integers(-2 ** 20 + 1, 2 ** 20, size=(rows, n)).astype(object)
    for i in range(lin):
        for l in range(1, ell + 1):
            body[i * ell + l - 1, 0] += int(s_in[i]) << (64 - beta * l)
    key = np.stack([A, (body % p).astype(np.uint64)], axis=1).reshape(-1)          # K[r][0] = mask, K[r][1] = body
    msgs = rng.integers(0, 8, size=m)
    step = p // 8
    a = random_words(rng, p, m * lin).reshape(m, lin)
    b = a.astype(object).dot(s_in.astype(object)) + msgs.astype(object) * step + rng.integers(-2 ** 40 + 1, 2 ** 40, size=m).astype(object)
    lwe = np.concatenate([a, (b % p).astype(np.uint64)[:, None]], axis=1).reshape(-1)
    want = model(p, lwe, key, lin, m, k, n, beta, ell, 1)
    out = want.reshape(k + 1, n)
    phase = (out[1].astype(object) - times_binary(out[0][None, :], NS)[0]) % p
    assert [int((8 * x + p // 2) // p) % 8 for x in phase] == [int(x) for x in msgs]      # the model, on the CPU
    for where in ("device", "host"):
        got = run_pack(torch, plan, p, where, lwe, key, lin, m, k, beta, ell, 1)
        assert np.array_equal(got, want), (where, first_difference(got, want))


# -- 6. bootstrap -> pack -------------------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


def addp(a, b, p):
    """a + b mod p on uint64 arrays of canonical words, p up to 2^64"""
    with np.errstate(over="ignore"):
        s = a + b
        return np.where((s < a) | (s >= np.uint64(p)), s - np.uint64(p), s)


def glwe_rows(torch, plan, p, rng, S, count, k, n, noise):
    """count GLWE encryptions of zero under S: (count, k + 1, n) words, body = sum_q A_q (*) S_q + e with |e| <= noise"""
    A = random_words(rng, p, count * k * n)
    prod = dev(torch, A)
    sk = dev(torch, np.tile(S.reshape(-1), count))
    plan.fwd_batch(sk)
    plan.mul_ntt_batch(prod, sk)
    torch.cuda.synchronize()
    prod = host(prod, np.uint64).reshape(count, k, n)
    body = np.zeros((count, n), dtype=np.uint64)
    for q in range(k):
        body = addp(body, prod[:, q], p)
    if noise:
        e = rng.integers(-noise, noise + 1, size=(count, n))
        body = addp(body, np.where(e < 0, np.uint64(p) - np.abs(e).astype(np.uint64), e.astype(np.uint64)), p)
    return np.concatenate([A.reshape(count, k, n), body[:, None, :]], axis=1)


def test_bootstrap_outputs_pack_into_one_glwe():
    """PM64, n = 1024, k = 1, L = 32: 8 messages of 2 bits under one padding bit (m -> m (p-1)/8, noise below 2^40), bootstrapped through
    the table of f with a noiseless bootstrapping key (base_log 8, levels 4), come out as LWE ciphertexts of dimension k n under the
    flattened GLWE key.  A packing key from that key back to the GLWE key (base_log 8, levels 3, |noise| < 2^20) packs them:
    coefficient t of the GLWE decrypts to f(m_t), every coefficient past the eighth to 0."""
    torch = _torch()
    p, n, k, beta, ell, L, pk_beta, pk_ell, count = PM64, 1024, 1, 8, 4, 32, 8, 3, 8
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("bootpack"))
    delta, big = (p - 1) // 8, k * n
    s = rng.integers(0, 2, size=L).astype(np.uint64)
    S = rng.integers(0, 2, size=(k, n)).astype(np.uint64)
    rows = (k + 1) * ell
    bsk = glwe_rows(torch, plan, p, rng, S, L * rows, k, n, 0).reshape(L, rows, k + 1, n)
    for q in range(k + 1):
        for l in range(1, ell + 1):
            bsk[:, q * ell + l - 1, q, 0] = addp(bsk[:, q * ell + l - 1, q, 0], s << np.uint64(64 - beta * l), p)
    pk = glwe_rows(torch, plan, p, rng, S, big * pk_ell, k, n, 2 ** 20 - 1).reshape(big, pk_ell, k + 1, n)
    for l in range(1, pk_ell + 1):
        pk[:, l - 1, k, 0] = addp(pk[:, l - 1, k, 0], S.reshape(-1) << np.uint64(64 - pk_beta * l), p)
    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = pbs_f((t % n) // (n // 4)) * delta
        lut[k * n + j] = v if t < n else (p - v) % p
    msgs = np.arange(count) & 3
    a = random_words(rng, p, count * L).reshape(count, L)
    b = a.astype(object).dot(s.astype(object)) + msgs.astype(object) * delta + rng.integers(-2 ** 40 + 1, 2 ** 40, size=count).astype(object)
    ct = np.concatenate([a, (b % p).astype(np.uint64)[:, None]], axis=1).reshape(-1)
    boot = torch.zeros(count * (big + 1), dtype=torch.int64, device="cuda")
    plan.bootstrap_batch(boot, dev(torch, ct), dev(torch, lut), key_ntt(torch, plan, bsk.reshape(-1)), L, k, beta, ell)
    glwe = dev(torch, np.full((k + 1) * n, 0x5A5A, dtype=np.uint64))
    plan.pack_keyswitch_batch(glwe, boot, key_ntt(torch, plan, pk.reshape(-1)), big, count, k, pk_beta, pk_ell)
    # phase = body - sum_q mask_q (*) S_q mod p
    prod = glwe[:k * n].clone()
    sk = dev(torch, S.reshape(-1))
    plan.fwd_batch(sk)
    plan.mul_ntt_batch(prod, sk)
    torch.cuda.synchronize()
    g, prod = host(glwe, np.uint64), host(prod, np.uint64).reshape(k, n)
    phase = g[k * n:].astype(object) - sum(prod[q].astype(object) for q in range(k))
    got = [int((8 * (int(x) % p) + p // 2) // p) % 8 for x in phase]
    assert got[:count] == [pbs_f(int(x)) for x in msgs], got[:count]
    assert not any(got[count:])


# -- 7. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_pack_with_a_caller_workspace():
    """captured once, replayed on fresh inputs written into the captured buffers"""
    torch = _torch()
    p, n, lin, m, k, beta, ell, batch = PM64, 1024, 50, 16, 1, 4, 3, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(14)
    lwe = dev(torch, random_words(rng, p, batch * m * (lin + 1)))
    kt = key_ntt(torch, plan, random_words(rng, p, lin * ell * (k + 1) * n))
    ws = torch.zeros(plan.pack_workspace_bytes(lin, ell, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros(batch * (k + 1) * n, dtype=torch.int64, device="cuda")
    plan.pack_keyswitch_batch(out, lwe, kt, lin, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.pack_keyswitch_batch(out, lwe, kt, lin, m, k, beta, ell, workspace=ws)
    fresh = dev(torch, random_words(rng, p, batch * m * (lin + 1)))
    eager = torch.zeros_like(out)
    plan.pack_keyswitch_batch(eager, fresh, kt, lin, m, k, beta, ell)
    lwe.copy_(fresh)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(out, eager)


# -- 8. with and without a caller workspace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,where", [(1024, "device"), (1024, "host"), (4096, "device")])
def test_with_and_without_a_workspace_give_identical_words(n, where):
    """n = 4096 on 64-bit words: the composed external product, which keeps its own scratch either way"""
    torch = _torch()
    p = P62
    plan = make_plan(p, n)
    lin, m, k, beta, ell, batch = 45, 9, 1, 7, 3, 2
    rng = np.random.default_rng(seed("ws", n, where))
    lwe = random_words(rng, p, batch * m * (lin + 1))
    key = random_words(rng, p, lin * ell * (k + 1) * n)
    one = run_pack(torch, plan, p, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=True)
    two = run_pack(torch, plan, p, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=False)
    assert np.array_equal(one, two) and not (one == np.uint64(0xA5A5A5A5A5A5A5A5)).any()


# -- 9. the C example -------------------------------------------------------------------------------------------------------------------------
def test_pack_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pack_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pack_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 8 and not any("WRONG" in ln for ln in lines), r.stdout
