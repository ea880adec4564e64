"""The LWE-to-GLWE packing keyswitch of the native plans (include/cntt_pack.h) on the MI355X.  Bit-exact throughout, no tolerance
anywhere: the call against a big-integer model (the matrix form that tests/test_native_pack_abi.py checks against the header's
formula and its phase identity, restated here) on shapes that cross every tile and chunk edge, on deterministic worst cases and on
encrypted messages; against the direct route through cntt_native_keyswitch_batch; on the outputs of a bootstrap; graph capture; with
and without a caller workspace; the C example."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from concrete_ntt_amd import native32, native64, native128, native_binary64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = {32: native32.Plan32, 64: native64.Plan32, 128: native128.Plan32}
# the decomposing transpose's tile (native_pack.hpp): TT ciphertexts x TI mask words per workgroup
TT = 64
TI = {32: 32, 64: 32, 128: 16}
# CNTT_PACK_TERMS (cntt_pack.h): terms of one external product at most
PACK_TERMS = 64


def C(plan, levels):
    """the chunk of mask words of one external product (cntt_pack.h), before the cap at Lin"""
    return max(1, min(plan.max_terms(), PACK_TERMS) // levels)


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# -- the model (as in tests/test_native_pack_abi.py) ----------------------------------------------------------------------------------
def digits(x, w, beta, ell):
    s = w - beta * ell
    state = x if s == 0 else ((x + (1 << (s - 1))) % (1 << w)) >> s
    B, out = 1 << beta, []
    for _ in range(ell):
        d = state % B
        state >>= beta
        if d >= B // 2:
            d -= B
            state += 1
        out.append(d)
    return out[::-1]


def model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch, dtype=object):
    """lwe: batch * m * (lin + 1) ints; key: lin * ell * (k + 1) * n ints, K[r][p] at (r * (k + 1) + p) * n -> batch * (k + 1) * n ints.
    Row t of D K is sum_r d_r(lwe_t) K[r]; the output is the body polynomial minus sum_t X^t (row t).  dtype object: Python ints,
    reduced at the end; np.uint32 / np.uint64 for w = 32 / 64: the arithmetic wraps modulo 2^w by itself."""
    M = 1 << w
    Kmat = np.array(key, dtype=dtype).reshape(lin * ell, (k + 1) * n) if lin else None
    out = []
    for g in range(batch):
        cts = lwe[g * m * (lin + 1):(g + 1) * m * (lin + 1)]
        acc = np.zeros((k + 1, n), dtype=dtype)
        if lin:
            D = np.array([[d if dtype is object else d % M for i in range(lin) for d in digits(cts[t * (lin + 1) + i], w, beta, ell)]
                          for t in range(m)], dtype=dtype)
            A = D.dot(Kmat).reshape(m, k + 1, n)
            for t in range(m):                                             # acc -= X^t A[t]
                acc[:, t:] -= A[t][:, :n - t]
                if t:
                    acc[:, :t] += A[t][:, n - t:]
        acc[k, :m] += np.array([cts[t * (lin + 1) + lin] for t in range(m)], dtype=dtype)
        out += [int(x) % M for x in acc.reshape(-1)]
    return out


# -- words <-> arrays ---------------------------------------------------------------------------------------------------------------
def to_array(plan, ints):
    if plan.WORD == 16:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=plan.word_dtype)


def to_ints(plan, a):
    if plan.WORD == 16:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[0::2], a[1::2])]
    return [int(x) for x in a]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def rand_ints(rng, w, count):
    raw = rng.bytes(count * (w // 8))
    return [int.from_bytes(raw[i * (w // 8):(i + 1) * (w // 8)], "little") for i in range(count)]


def random_words(rng, plan, count):
    return rng.integers(0, np.iinfo(plan.word_dtype).max, size=count * (2 if plan.WORD == 16 else 1), dtype=plan.word_dtype, endpoint=True)


def key_planes(torch, plan, key_words, where="device"):
    """the residue planes of coefficient-domain key words (an array), as one fwd_batch over all key polynomials writes them"""
    per = plan.ntt_size() * (2 if plan.WORD == 16 else 1)
    res = torch.int64 if plan.RES == 8 else torch.int32
    kr = [torch.empty(len(key_words) // per * plan.ntt_size(), dtype=res, device="cuda") for _ in range(plan.NPRIMES)]
    if len(key_words):
        plan.fwd_batch(dev(torch, key_words), kr, binary=plan.BINARY)
        torch.cuda.synchronize()
    return kr if where == "device" else [host(p, plan.res_dtype).copy() for p in kr]


def run_pack_arrays(torch, plan, where, la, ka, lin, m, k, beta, ell, batch, with_ws=False):
    """the call on word arrays (ciphertexts, coefficient-domain key) -> the output array; the output buffer starts out poisoned"""
    mult = 2 if plan.WORD == 16 else 1
    kr = key_planes(torch, plan, ka, where)
    poison = np.full(batch * (k + 1) * plan.ntt_size() * mult, 0xA5, dtype=plan.word_dtype)
    nws = plan.pack_workspace_bytes(lin, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.pack_keyswitch_batch(poison, la, kr, lin, m, k, beta, ell, workspace=ws)
        return poison
    out = dev(torch, poison)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.pack_keyswitch_batch(out, dev(torch, la), kr, lin, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out, plan.word_dtype)


def run_pack(torch, plan, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=False):
    """the call on int lists -> the output as ints"""
    return to_ints(plan, run_pack_arrays(torch, plan, where, to_array(plan, lwe), to_array(plan, key), lin, m, k, beta, ell, batch, with_ws))


def first_difference(got, want):
    bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
    return (bad[0], hex(got[bad[0]]), hex(want[bad[0]]), len(bad)) if bad else None


# -- 1. the call against the model across every tile and chunk edge ------------------------------------------------------------------------
def shapes(plan, w):
    """(n, batch, m, lin, k, beta, ell).  n = 32: m 1 / inside / n; lin 0, 1, one below and above the tile TI, one below and above the
    chunk C, 2 C + 3; k 1 / 2; batch 1 / 3; beta * ell = w and < w; beta 1 and 31, and one digit wider than 32 bits.  n = 128: m one
    below and above the tile TT, and n (two tiles along t)."""
    ti = TI[w]
    full = {32: (8, 4), 64: (16, 4), 128: (16, 8)}[w]          # beta * ell = w
    top = {32: (31, 1), 64: (31, 2), 128: (31, 4)}[w]           # beta = 31
    return [(32, 1, 1, 0, 1, 5, 3),
            (32, 3, 32, 1, 2, *full),
            (32, 1, 31, ti - 1, 1, 5, 3),
            (32, 3, 32, ti + 1, 2, 4, 3),
            (32, 1, 7, C(plan, top[1]) - 1, 1, *top),
            (32, 1, 32, C(plan, 7) + 1, 2, 1, 7),
            (32, 3, 5, 2 * C(plan, 2) + 3, 1, 6, 2),
            (32, 1, 32, C(plan, full[1]) + 1, 1, *full),
            (32, 1, 17, C(plan, 3) - 1, 2, 5, 3),
            (32, 1, 3, 2, 1, w // 2, 2),
            (128, 1, TT - 1, 3, 1, 5, 3),
            (128, 2, TT + 1, ti + 1, 1, 4, 3),
            (128, 1, 128, 2, 2, *full)]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w", [32, 64, 128])
def test_pack_matches_model(w, where):
    torch = _torch()
    plans = {n: WORDS[w].try_new(n) for n in (32, 128)}
    assert C(plans[32], 1) == PACK_TERMS                        # max_terms does not cap the chunk at these sizes
    for n, batch, m, lin, k, beta, ell in shapes(plans[32], w):
        plan = plans[n]
        rng = np.random.default_rng(seed(w, where, n, batch, m, lin, k))
        lwe = rand_ints(rng, w, batch * m * (lin + 1))
        key = rand_ints(rng, w, lin * ell * (k + 1) * n)
        want = model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch)
        got = run_pack(torch, plan, where, lwe, key, lin, m, k, beta, ell, batch)
        assert got == want, (w, where, n, batch, m, lin, k, beta, ell, "first bad word", first_difference(got, want))
        if lin == 0:                                            # the poison is gone: zero masks, zero tail of the body polynomial
            # (no chunk, no key: a workspace the caller brings is not touched, and without one the device path allocates none)
            assert run_pack(torch, plan, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=True) == want, (w, where, "lin = 0 with a workspace")
            for g in range(batch):
                o = got[g * (k + 1) * n:(g + 1) * (k + 1) * n]
                assert not any(o[:k * n]) and not any(o[k * n + m:]) and o[k * n:k * n + m] == [lwe[(g * m + t) * (lin + 1) + lin] for t in range(m)]


@pytest.mark.parametrize("cls,binary", [(native64.Plan52, False), (native_binary64.Plan32, True)])
def test_the_other_kinds_pack_too(cls, binary):
    """a Plan52 kind (the composed external product) and a binary kind (key words 0 / 1, fwd_binary_batch)"""
    torch = _torch()
    w, n, batch, m, lin, k, beta, ell = 64, 32, 2, 9, TI[64] + 2, 1, 6, 3
    plan = cls.try_new(n)
    rng = np.random.default_rng(seed(cls.__doc__))
    lwe = rand_ints(rng, w, batch * m * (lin + 1))
    key = [int(x) for x in rng.integers(0, 2, size=lin * ell * (k + 1) * n)] if binary else rand_ints(rng, w, lin * ell * (k + 1) * n)
    want = model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch)
    got = run_pack(torch, plan, "device", lwe, key, lin, m, k, beta, ell, batch)
    assert got == want, first_difference(got, want)


# -- 2. deterministic worst cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64, 128])
def test_pack_worst_cases(w):
    """Every digit -B/2 (stored negated: +B/2, the one value a signed digit cannot take) against all-ones key words, every digit B/2 - 1
    against 2^(w-1), and words 2^w - 1 that round up across the top (to all-zero digits when s > 0): a wrong sign fix-up or a lost
    carry shows in every word.  Lin = C + 2, m = n = 32."""
    torch = _torch()
    n, k, m = 32, 1, 32
    plan = WORDS[w].try_new(n)
    M = 1 << w
    for beta, ell in ((4, 3), (1, 5), (31, w // 32)):
        s, B = w - beta * ell, 1 << beta
        lin = C(plan, ell) + 2
        low = (sum(-(B // 2) << (beta * j) for j in range(ell)) % (1 << (beta * ell))) << s
        high = sum((B // 2 - 1) << (beta * (ell - 1 - j)) for j in range(ell)) << s
        assert digits(low, w, beta, ell) == [-B // 2] * ell and digits(high, w, beta, ell) == [B // 2 - 1] * ell
        assert s == 0 or digits(M - 1, w, beta, ell) == [0] * ell
        rng = np.random.default_rng(seed(w, beta, ell))
        for word in (low, high, M - 1):
            lwe = [word] * (m * (lin + 1))
            for keyword in (M - 1, 1 << (w - 1)):
                key = [keyword] * (lin * ell * (k + 1) * n)
                want = model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1)
                got = run_pack(torch, plan, "device", lwe, key, lin, m, k, beta, ell, 1)
                assert got == want, (w, beta, ell, hex(word), hex(keyword), first_difference(got, want))


# -- 3. the NTT route and the direct route agree ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 8192])
@pytest.mark.parametrize("w", [32, 64])
def test_pack_equals_keyswitch_rotate_and_sum(w, n):
    """Plan32 kinds: n = 1024 runs the fused external product, n = 8192 the composed one.  The existing keyswitch_batch on the same
    coefficient-domain key, viewed as Lin * levels rows of (k + 1) n words, gives KS(lwe_t) with the body word in the last place; moved
    to coefficient 0 of the body polynomial, rotated by X^t and summed over t in wrapping numpy arithmetic it is the packed output."""
    torch = _torch()
    plan = WORDS[w].try_new(n)
    m, lin, ell, beta, batch, k = 5, 20, 2, 8, 2, 1
    cols = (k + 1) * n
    rng = np.random.default_rng(seed("routes", w, n))
    lwe_a = random_words(rng, plan, batch * m * (lin + 1))
    key_a = random_words(rng, plan, lin * ell * cols)
    lwe_t = dev(torch, lwe_a)
    packed = torch.zeros(batch * cols, dtype=lwe_t.dtype, device="cuda")
    plan.pack_keyswitch_batch(packed, lwe_t, key_planes(torch, plan, key_a), lin, m, k, beta, ell)
    rows = torch.zeros(batch * m * cols, dtype=lwe_t.dtype, device="cuda")
    plan.keyswitch_batch(rows, lwe_t, dev(torch, key_a), lin, cols - 1, beta, ell)
    torch.cuda.synchronize()
    ks = host(rows, plan.word_dtype).reshape(batch, m, k + 1, n).copy()
    body = lwe_a.reshape(batch, m, lin + 1)[:, :, lin]
    with np.errstate(over="ignore"):
        ks[:, :, k, n - 1] -= body                                  # the body word leaves the last place ...
        ks[:, :, k, 0] += body                                      # ... for coefficient 0 of the body polynomial
        want = np.zeros((batch, k + 1, n), dtype=plan.word_dtype)
        for t in range(m):                                          # + X^t KS(lwe_t)
            want[:, :, t:] += ks[:, t, :, :n - t]
            if t:
                want[:, :, :t] -= ks[:, t, :, n - t:]
    got = host(packed, plan.word_dtype).reshape(batch, k + 1, n)
    assert got.any() and np.array_equal(got, want), (w, n, int((got != want).sum()))


# -- 4. decryption ------------------------------------------------------------------------------------------------------------------------
def negacyclic_matrix(S):
    """N with (N a)[c] = (a (*) S)[c] for wrapping uint64 words: N[c][j] = S[c - j], negated past the wrap"""
    n = len(S)
    ext = np.concatenate([S, (0 - S)]).astype(np.uint64)
    idx = (np.arange(n)[:, None] - np.arange(n)[None, :]) % (2 * n)
    return ext[idx]


def test_pack_decrypts_under_the_output_key():
    """w = 64, n = 256, k = 1: 256 LWE ciphertexts of dimension 64 (3-bit messages at 2^61 under a binary key, noise below 2^40) packed
    under a noisy key (|e| < 2^20 per coefficient) with base_log 4, levels 6 into one GLWE ciphertext under a binary GLWE key.  The
    model's output decrypts coefficient t to message t -- asserted first, on the CPU -- and the device and host words are the
    model's.  Error per coefficient: the rounding of 64 mask words to 24 bits, at most 64 * 2^39 = 2^45; the key noise, 64 * 6 rows
    times 256 digit coefficients of at most 8 times 2^20, below 2^40; the ciphertext's own noise, below 2^40: together far below the
    2^60 that half a message step allows."""
    torch = _torch()
    w, n, k, lin, m, beta, ell = 64, 256, 1, 64, 256, 4, 6
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(seed("decrypt"))
    u64 = np.uint64
    s_in = rng.integers(0, 2, size=lin, dtype=u64)
    S = rng.integers(0, 2, size=n, dtype=u64)
    NS = negacyclic_matrix(S)
    rows = lin * ell
    A = rng.integers(0, 2 ** 64 - 1, size=(rows, n), dtype=u64, endpoint=True)
    with np.errstate(over="ignore"):
        body = A.dot(NS.T) + rng.integers(-2 ** 20 + 1, 2 ** 20, size=(rows, n)).astype(np.int64).view(u64)
        for i in range(lin):
            for l in range(1, ell + 1):
                body[i * ell + l - 1, 0] += s_in[i] << u64(w - beta * l)
        key = np.stack([A, body], axis=1).reshape(-1)                # K[r][0] = mask, K[r][1] = body
        msgs = rng.integers(0, 8, size=m, dtype=u64)
        a = rng.integers(0, 2 ** 64 - 1, size=(m, lin), dtype=u64, endpoint=True)
        b = a.dot(s_in) + (msgs << u64(61)) + rng.integers(-2 ** 40 + 1, 2 ** 40, size=m).astype(np.int64).view(u64)
    lwe = [int(x) for x in np.concatenate([a, b[:, None]], axis=1).reshape(-1)]
    key = [int(x) for x in key]
    want = model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1, dtype=u64)
    out = np.array(want, dtype=u64).reshape(k + 1, n)
    with np.errstate(over="ignore"):
        phase = out[1] - NS.dot(out[0])
    assert [int(x) for x in (((phase >> u64(60)) + u64(1)) >> u64(1)) & u64(7)] == [int(x) for x in msgs]      # the model, on the CPU
    for where in ("device", "host"):
        got = run_pack(torch, plan, where, lwe, key, lin, m, k, beta, ell, 1)
        assert got == want, (where, first_difference(got, want))


# -- 5. bootstrap -> pack -------------------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


def table(fn, n, k):
    """trivial GLWE, body X^(-n/8) v0 with v0[j] = fn(j / (n/4)) 2^61"""
    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = fn((t % n) // (n // 4)) << 61
        lut[k * n + j] = v if t < n else (-v) % (1 << 64)
    return lut


def test_bootstrap_outputs_pack_into_one_glwe():
    """native64 Plan32, n = 1024, k = 1, L = 32: 8 messages of 2 bits under one padding bit, bootstrapped through the table of f with
    the noiseless bootstrapping key of tests/test_gpu_native_pbs.py (base_log 8, levels 4), come out as LWE ciphertexts of dimension
    k n under the flattened GLWE key.  A packing key from that key back to the GLWE key (base_log 8, levels 3, |noise| < 2^20) packs
    them: coefficient t of the GLWE decrypts to f(m_t), every coefficient past the eighth to 0."""
    torch = _torch()
    n, k, beta, ell, L, w, pk_beta, pk_ell, count = 1024, 1, 8, 4, 32, 64, 8, 3, 8
    plan = native64.Plan32.try_new(n)
    g = torch.Generator(device="cuda").manual_seed(2424)

    def rand64(*shape):
        return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device="cuda", generator=g)

    s = torch.randint(0, 2, (L,), dtype=torch.int64, device="cuda", generator=g)
    S = torch.randint(0, 2, (k, n), dtype=torch.int64, device="cuda", generator=g)
    rows = (k + 1) * ell
    bsk = torch.zeros((L, rows, k + 1, n), dtype=torch.int64, device="cuda")
    bsk[:, :, :k, :] = rand64(L, rows, k, n)
    A = bsk[:, :, :k, :].contiguous()
    prod = torch.zeros_like(A)
    plan.negacyclic_polymul_batch(prod.view(-1), A.view(-1), S.expand(L, rows, k, n).contiguous().view(-1))
    bsk[:, :, k, :] = prod.sum(dim=2)
    for p in range(k + 1):
        for l in range(1, ell + 1):
            bsk[:, p * ell + l - 1, p, 0] += s << (w - beta * l)
    kr = [torch.empty(bsk.numel(), dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(bsk.view(-1), kr)
    # the packing key: row (i, l) = (A, A (*) S + e + Sflat[i] 2^(w - pk_beta l) at coefficient 0), Sflat the flattened GLWE key
    big = k * n
    pk = torch.zeros((big * pk_ell, k + 1, n), dtype=torch.int64, device="cuda")
    pk[:, :k, :] = rand64(big * pk_ell, k, n)
    A = pk[:, :k, :].contiguous()
    prod = torch.zeros_like(A)
    plan.negacyclic_polymul_batch(prod.view(-1), A.view(-1), S.expand(big * pk_ell, k, n).contiguous().view(-1))
    pk[:, k, :] = prod.sum(dim=1) + torch.randint(-2 ** 20 + 1, 2 ** 20, (big * pk_ell, n), dtype=torch.int64, device="cuda", generator=g)
    shifts = torch.tensor([w - pk_beta * l for l in range(1, pk_ell + 1)], dtype=torch.int64, device="cuda")
    pk[:, k, 0] += (S.view(-1)[:, None] << shifts[None, :]).reshape(-1)
    pkr = [torch.empty(pk.numel(), dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(pk.view(-1), pkr)
    # the messages, under s
    msgs = torch.arange(count, dtype=torch.int64, device="cuda") & 3
    a = rand64(count, L)
    noise = torch.randint(-2 ** 40 + 1, 2 ** 40, (count,), dtype=torch.int64, device="cuda", generator=g)
    ct = torch.cat([a, ((a * s).sum(dim=1) + (msgs << 61) + noise)[:, None]], dim=1).contiguous().view(-1)
    boot = torch.zeros(count * (big + 1), dtype=torch.int64, device="cuda")
    plan.bootstrap_batch(boot, ct, dev(torch, table(pbs_f, n, k)), kr, L, k, beta, ell)
    glwe = torch.full(((k + 1) * n,), 0x5A5A, dtype=torch.int64, device="cuda")
    plan.pack_keyswitch_batch(glwe, boot, pkr, big, count, k, pk_beta, pk_ell)
    # phase = body - sum_q mask_q (*) S_q (int64 arithmetic wraps: mod 2^64)
    prod = torch.zeros(k * n, dtype=torch.int64, device="cuda")
    plan.negacyclic_polymul_batch(prod, glwe[:k * n].contiguous(), S.contiguous().view(-1))
    torch.cuda.synchronize()
    phase = glwe[k * n:] - prod.view(k, n).sum(dim=0)
    got = (((phase >> 60) + 1 >> 1) & 7).cpu().tolist()
    assert got[:count] == [pbs_f(int(x)) for x in msgs.cpu()], got[:count]
    assert not any(got[count:])


# -- 6. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_pack_with_a_caller_workspace():
    """captured once, replayed on fresh inputs written into the captured buffers"""
    torch = _torch()
    n, lin, m, k, beta, ell, batch = 1024, 50, 16, 1, 4, 3, 3
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(13)
    lwe = dev(torch, random_words(rng, plan, batch * m * (lin + 1)))
    kr = key_planes(torch, plan, random_words(rng, plan, lin * ell * (k + 1) * n))
    ws = torch.zeros(plan.pack_workspace_bytes(lin, ell, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros(batch * (k + 1) * n, dtype=torch.int64, device="cuda")
    plan.pack_keyswitch_batch(out, lwe, kr, lin, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.pack_keyswitch_batch(out, lwe, kr, lin, m, k, beta, ell, workspace=ws)
    fresh = dev(torch, random_words(rng, plan, batch * m * (lin + 1)))
    eager = torch.zeros_like(out)
    plan.pack_keyswitch_batch(eager, fresh, kr, lin, m, k, beta, ell)
    lwe.copy_(fresh)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(out, eager)


# -- 7. with and without a caller workspace ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,where", [(1024, "device"), (1024, "host"), (8192, "device")])
def test_with_ws_true_and_false_give_identical_words(n, where):
    torch = _torch()
    plan = native64.Plan32.try_new(n)
    lin, m, k, beta, ell, batch = 45, 9, 1, 7, 3, 2
    rng = np.random.default_rng(seed("ws", n, where))
    lwe = random_words(rng, plan, batch * m * (lin + 1))
    key = random_words(rng, plan, lin * ell * (k + 1) * n)
    one = run_pack_arrays(torch, plan, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=True)
    two = run_pack_arrays(torch, plan, where, lwe, key, lin, m, k, beta, ell, batch, with_ws=False)
    assert np.array_equal(one, two) and not (one == np.uint64(0xA5A5A5A5A5A5A5A5)).any()


# -- 8. the C example -------------------------------------------------------------------------------------------------------------------------
def test_pack_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pack"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pack")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 8 and not any("WRONG" in ln for ln in lines), r.stdout
