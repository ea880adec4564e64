"""The programmable bootstrap of the prime plans (include/cntt_prime_pbs.h) on the MI355X.  Bit-exact: decomposition, modulus switch
and sample extraction against the plain-int model of tests/test_prime_pbs_model.py; cntt_prime*_blind_rotate_batch against the
per-iteration public calls it replaces (both buffers compared whole) and, at n <= 64, against the big-integer model;
cntt_prime*_bootstrap_batch against its three steps; graph capture; the C example.  The one check with a tolerance is the functional
test, whose bound is derived in its docstring.

Strict-range primes (2^62 <= p < 2^63, 2^30 <= p < 2^31): the reference's Barrett wrap can make mul_accumulate
differ from the exact product mod p.  Whether it does is a property of the prime, not of the range -- P63 and P31 lie right below
2^63 and 2^31, where the estimate never passes the word -- so the big-integer product model runs for the primes of EXACT, which a probe
on the CPU oracle selects (random_cases.model_applies); a prime outside it (PW63, PW31: strict-range primes whose products do wrap) runs the comparisons
against the public calls and the decomposition / modswitch / extract model checks only."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from concrete_ntt_amd import prime32, prime64
from test_prime_pbs_model import (P30, P32, P50, P62, P63, PM64, digits, edge_words, model_extract, model_modswitch, model_terms_element,
                                  modswitch_words, negacyclic, settings, source, wbits)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PG64 = 9224497936763846657          # 64-bit Montgomery class: p >= 2^63 and not 2^64 - c
P51 = 2251799813554177              # below 2^51 (the second 64-bit class on doubles)
P31 = 2147352577                    # 32-bit strict range
PA62 = 2305843009214414849          # lazy, just above 2^61: the reference's Barrett estimate reaches 2p (the parity fix in inv)
PA30 = 536903681                    # the same on 32-bit words, just above 2^29
PW63 = 8717305756806021121          # strict range, where the reference's Barrett product does wrap: the probe rejects it
PW31 = 2088517633                   # the same on 32-bit words (1 mod 2^14 only)
ALL = [P62, PM64, P50, P63, P30, P32, PG64, P51, P31, PA62, PA30, PW63, PW31]
# the primes for which the big-integer model applies: the oracle's fwd / mul_accumulate / inv composition equals the exact product on
# the fixed probe of random_cases.model_applies (asserted in tests/test_random_cases.py, on the CPU)
EXACT = [P62, PM64, P50, P63, P30, P32, PG64, P51, P31, PA62, PA30]


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def is64(p):
    return p >= 1 << 32


def make_plan(p, n):
    plan = (prime64 if is64(p) else prime32).Plan.try_new(n, p)
    assert plan is not None, (p, n)
    return plan


def min_n(p):
    return 16 if is64(p) else 32


def dt(p):
    return np.uint64 if is64(p) else np.uint32


def max_logn(p):
    """the largest log2 n with p = 1 mod 2n"""
    return ((p - 1) & -(p - 1)).bit_length() - 2


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def zeros(torch, p, count):
    return torch.zeros(count, dtype=torch.int64 if is64(p) else torch.int32, device="cuda")


def random_words(rng, p, count):
    return rng.integers(0, p, size=count, dtype=np.uint64).astype(dt(p))


def rot_values(rng, n, batch, shift=0):
    fixed = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    return np.array([fixed[(b + shift) % 6] if b < 6 else int(rng.integers(0, 2 * n)) for b in range(batch)], dtype=np.uint32)


def rot_rows(rng, n, L, batch):
    return np.concatenate([rot_values(rng, n, batch, shift=i) for i in range(L + 1)])


def workspace(torch, plan, L, k, levels, batch):
    return torch.zeros(plan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")


def key_ntt(torch, plan, key_words):
    """n^-1 fwd(key): the header's key convention"""
    t = dev(torch, key_words)
    plan.fwd_batch(t)
    plan.normalize_batch(t)
    return t


# -- 1. decomposition against the model -------------------------------------------------------------------------------------------------
WHOLE = 2048       # up to this many source words the model replays every word; beyond it a sample


def sample_positions(rng, n, a, count):
    pos = {0, 1, n - 1, a % n, (a - 1) % n, (a + 1) % n}
    pos |= {int(x) for x in rng.integers(0, n, size=count)}
    return sorted(pos)


def check_decomposition(torch, plan, p, n, mode, beta, ell, batch, npolys, rng, shift):
    polys = random_words(rng, p, batch * npolys * n)
    edges = edge_words(p, beta, ell)
    m = min(len(edges), polys.size)
    polys[:m] = np.array(edges[:m], dtype=dt(p))
    if polys.size >= 2 * m:      # the same words again where the rotation wraps them round
        polys[-m:] = np.array(edges[:m], dtype=dt(p))
    rot = rot_values(rng, n, batch, shift)
    terms = zeros(torch, p, polys.size * ell)
    plan.gadget_decompose_batch(terms, dev(torch, polys), beta, ell, rot=None if mode == "plain" else dev(torch, rot), mode=mode)
    torch.cuda.synchronize()
    got = host(terms, dt(p))
    f = polys.tolist()
    if polys.size <= WHOLE:
        for b in range(batch):
            elem = [f[(b * npolys + q) * n:(b * npolys + q + 1) * n] for q in range(npolys)]
            want = [x for t in model_terms_element(elem, int(rot[b]), p, beta, ell, mode) for x in t]
            lo = b * npolys * ell * n
            assert [int(x) for x in got[lo:lo + npolys * ell * n]] == want, (p, n, mode, beta, ell, batch, npolys, "element", b)
        return
    per_poly = max(8, WHOLE // (batch * npolys))
    for q in range(batch * npolys):
        a = 0 if mode == "plain" else int(rot[q // npolys])
        fq = f[q * n:(q + 1) * n]
        for i in sample_positions(rng, n, a, per_poly):
            x = fq[i]
            if mode != "plain":
                t = (i - a) % (2 * n)
                x = (-fq[t % n]) % p if t >= n else fq[t % n]
                if mode == "cmux":
                    x = (x - fq[i]) % p
            want = digits(x, p, beta, ell)
            have = [int(got[(q * ell + l) * n + i]) for l in range(ell)]
            assert have == want, (p, n, mode, beta, ell, batch, npolys, "polynomial", q, "coefficient", i, "exponent", a)


@pytest.mark.parametrize("n", [16, 64, 1024, 4096])
@pytest.mark.parametrize("p", ALL)
def test_decomposition_matches_model(p, n):
    """all three modes, the exponents 0, 1, n - 1, n, n + 1, 2n - 1 (one per batch element, cycled), every valid setting of the list --
    (16, 4) at W = 64 and (W, 1) are the cases whose sum passes the word -- batch 1 / 3 / 33 and 1 / 3 polynomials per element; the
    inputs carry 0, 1, p - 1, (p - 1) / 2 +- 1 and the words whose rounding lands on +- B^levels / 2.  n = 16 is n = 32 on 32-bit words
    (the smallest prime32 plan)."""
    torch = _torch()
    n = max(n, min_n(p))
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("dec", p, n))
    shapes = [(1, 1), (1, 3), (3, 1), (3, 3), (33, 1), (33, 3)]
    shift = 0
    for mode in ("plain", "rotate", "cmux"):
        for beta, ell in settings(p):
            for batch, npolys in shapes:
                check_decomposition(torch, plan, p, n, mode, beta, ell, batch, npolys, rng, shift)
                shift += 1


def test_decomposition_on_the_host_path_and_noncanonical_words_do_not_fault():
    torch = _torch()
    p, n = PM64, 64
    plan = make_plan(p, n)
    rng = np.random.default_rng(5)
    polys = random_words(rng, p, 3 * n)
    rot = np.array([n + 1], dtype=np.uint32)
    terms = np.zeros(polys.size * 4, dtype=np.uint64)
    plan.gadget_decompose_batch(terms, polys, 16, 4, rot=rot, mode="cmux")
    elem = [[int(x) for x in polys[q * n:(q + 1) * n]] for q in range(3)]
    assert [int(x) for x in terms] == [x for t in model_terms_element(elem, n + 1, p, 16, 4) for x in t]
    # words >= p: unspecified values, but the call completes and a canonical element of the same batch is unaffected
    bad = np.concatenate([np.full(n, 2 ** 64 - 1, dtype=np.uint64), polys[:n]])
    out = zeros(torch, p, 2 * n * 4)
    plan.gadget_decompose_batch(out, dev(torch, bad), 16, 4, rot=dev(torch, np.array([3, 3], dtype=np.uint32)), mode="cmux")
    torch.cuda.synchronize()
    want = [x for t in model_terms_element([elem[0]], 3, p, 16, 4) for x in t]
    assert [int(x) for x in host(out, np.uint64)[4 * n:]] == want


STREAM_BYTES = 384 << 20   # the library's streaming threshold (host_common.hpp)


def sampled_elements(rng, batch, count=32):
    return sorted({0, batch - 1} | {int(x) for x in rng.integers(0, batch, size=count)})


def device_words(torch, p, count, g):
    t = torch.randint(0, p, (count,), dtype=torch.int64, device="cuda", generator=g)
    return t if is64(p) else t.to(torch.int32)


@pytest.mark.parametrize("p", [P62, P30])
def test_decomposition_of_a_streaming_batch(p):
    """prime_gadget_kernel<T, true> on both word types: the first batch whose terms pass the streaming threshold (non-temporal stores)
    at n = 1024, 2 polynomials per element, 4 levels, against the same call made in two halves, which do not stream, on every word, and
    against the model on the first, the last and 32 sampled elements."""
    torch = _torch()
    n, npolys, beta, ell = 1024, 2, 7, 4
    per = npolys * n
    batch = STREAM_BYTES // (npolys * ell * n * dt(p)().itemsize) + 1
    plan = make_plan(p, n)
    g = torch.Generator(device="cuda").manual_seed(5)
    polys = device_words(torch, p, batch * per, g)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=g)
    terms = torch.empty(batch * per * ell, dtype=polys.dtype, device="cuda")
    plan.gadget_decompose_batch(terms, polys, beta, ell, rot=rot, mode="cmux")
    half = batch // 2
    small = torch.empty((batch - half) * per * ell, dtype=polys.dtype, device="cuda")
    plan.gadget_decompose_batch(small[:half * per * ell], polys[:half * per], beta, ell, rot=rot[:half], mode="cmux")
    assert torch.equal(small[:half * per * ell], terms[:half * per * ell])
    plan.gadget_decompose_batch(small, polys[half * per:], beta, ell, rot=rot[half:], mode="cmux")
    assert torch.equal(small, terms[half * per * ell:])
    rot_h = rot.cpu().tolist()
    for b in sampled_elements(np.random.default_rng(seed("stream", p)), batch):
        f = host(polys[b * per:(b + 1) * per], dt(p)).tolist()
        want = [x for t in model_terms_element([f[q * n:(q + 1) * n] for q in range(npolys)], rot_h[b], p, beta, ell) for x in t]
        assert host(terms[b * per * ell:(b + 1) * per * ell], dt(p)).tolist() == want, (p, "element", b)


@pytest.mark.parametrize("p,per_element", [(P62, False), (P30, True)])
def test_blind_rotate_set_up_of_a_streaming_batch(p, per_element):
    """prime_pbs_init_kernel<T, true> on both word types: blind_rotate_batch with lwe_dim = 0 is the set-up alone (acc = X^rot lut: no
    digits, no key); the first batch whose accumulator passes the streaming threshold at n = 1024, k = 1, against the same call in two
    halves on every word and against the model on the first, the last and 32 sampled elements."""
    torch = _torch()
    n, k = 1024, 1
    per = (k + 1) * n
    batch = STREAM_BYTES // (per * dt(p)().itemsize) + 1
    plan = make_plan(p, n)
    g = torch.Generator(device="cuda").manual_seed(6)
    lut = device_words(torch, p, (batch if per_element else 1) * per, g)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=g)
    nokey = torch.empty(0, dtype=lut.dtype, device="cuda")
    acc = torch.empty(batch * per, dtype=lut.dtype, device="cuda")
    plan.blind_rotate_batch(acc, lut, rot, nokey, 0, k, 7, 3, lut_per_element=per_element)
    half = batch // 2
    small = torch.empty((batch - half) * per, dtype=lut.dtype, device="cuda")
    plan.blind_rotate_batch(small[:half * per], lut[:half * per] if per_element else lut, rot[:half], nokey, 0, k, 7, 3, lut_per_element=per_element)
    assert torch.equal(small[:half * per], acc[:half * per])
    plan.blind_rotate_batch(small, lut[half * per:] if per_element else lut, rot[half:], nokey, 0, k, 7, 3, lut_per_element=per_element)
    assert torch.equal(small, acc[half * per:])
    rot_h = rot.cpu().tolist()
    for b in sampled_elements(np.random.default_rng(seed("stream-init", p)), batch):
        f = host(lut[b * per:(b + 1) * per] if per_element else lut, dt(p)).tolist()
        want = [x for q in range(k + 1) for x in source(f[q * n:(q + 1) * n], rot_h[b], p, "rotate")]
        assert host(acc[b * per:(b + 1) * per], dt(p)).tolist() == want, (p, "element", b)


# -- 2. modulus switch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", range(4, 16))
@pytest.mark.parametrize("p", ALL)
def test_modswitch_matches_model(p, logn):
    torch = _torch()
    if (1 << logn) < min_n(p):
        logn = 5          # the smallest prime32 plan (the case runs twice rather than being skipped)
    logn = min(logn, max_logn(p))          # PA30 = 1 mod 2^15, PW31 = 1 mod 2^14 only: their largest plan, likewise
    plan = make_plan(p, 1 << logn)
    rng = np.random.default_rng(seed("ms", p, logn))
    special = modswitch_words(p, logn, rng)
    for L in (0, 1, 31, 32, 33):
        for batch in (1, 33):
            count = batch * (L + 1)
            words = [special[(i // 2 + L) % len(special)] if i % 2 == 0 else int(rng.integers(0, p, dtype=np.uint64)) for i in range(count)]
            lwe = np.array(words, dtype=dt(p))
            rot_t = torch.full((count,), -1, dtype=torch.int32, device="cuda")
            plan.lwe_modswitch_batch(rot_t, dev(torch, lwe), L)
            torch.cuda.synchronize()
            assert [int(x) for x in host(rot_t, np.uint32)] == model_modswitch(words, L, batch, p, logn), (p, logn, L, batch)


# -- 3. sample extraction ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", ALL)
def test_sample_extract_matches_model(p, where):
    torch = _torch()
    n, batch = 64, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ext", p))
    for k in (1, 2):
        glwe = random_words(rng, p, batch * (k + 1) * n)
        glwe[0], glwe[n - 1], glwe[1] = 0, p - 1, 1
        g = [int(x) for x in glwe]
        for index in (0, 1, n - 1):
            if where == "host":
                out = np.zeros(batch * (k * n + 1), dtype=dt(p))
                plan.sample_extract_batch(out, glwe.copy(), k, index)
                got = [int(x) for x in out]
            else:
                out = zeros(torch, p, batch * (k * n + 1))
                plan.sample_extract_batch(out, dev(torch, glwe), k, index)
                torch.cuda.synchronize()
                got = [int(x) for x in host(out, dt(p))]
            want = []
            for b in range(batch):
                base = b * (k + 1) * n
                want += model_extract([g[base + q * n:base + (q + 1) * n] for q in range(k + 1)], index, p)
            assert got == want, (p, k, index, where)


# -- 4. blind rotation against the loop of public calls ----------------------------------------------------------------------------------
def per_iteration_reference(torch, plan, p, lut_t, per_element, rot_t, bsk, L, k, beta, ell, batch):
    n, npolys = plan.ntt_size(), k + 1
    tiled = lut_t if per_element else lut_t.repeat(batch)
    acc = torch.zeros_like(tiled)
    plan.gadget_decompose_batch(acc, tiled, wbits(p), 1, rot=rot_t[L * batch:], mode="rotate")   # X^a f: its one full-width digit
    terms = torch.zeros(acc.numel() * ell, dtype=acc.dtype, device="cuda")
    slice_ = npolys * ell * npolys * n
    for i in range(L):
        plan.gadget_decompose_batch(terms, acc, beta, ell, rot=rot_t[i * batch:(i + 1) * batch], mode="cmux")
        plan.external_product_batch(acc, terms, bsk[i * slice_:(i + 1) * slice_], npolys * ell, npolys, accumulate=True)
    torch.cuda.synchronize()
    return acc


def check_blind_rotate(torch, p, n, k, L, batch, per_element, with_ws, beta=7, ell=3, where="device"):
    """where = "host": the call on host slices (a host-side workspace is checked and then ignored), the reference on the device"""
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("br", p, n, k, L, batch, per_element, with_ws))
    lut_t = dev(torch, random_words(rng, p, (batch if per_element else 1) * (k + 1) * n))
    rot_t = dev(torch, rot_rows(rng, n, L, batch))
    bsk = dev(torch, random_words(rng, p, L * (k + 1) * ell * (k + 1) * n))      # any canonical words do for this comparison
    acc = dev(torch, random_words(rng, p, batch * (k + 1) * n))                  # written only: the prior content must not matter
    if where == "host":
        acc_h = host(acc, dt(p)).copy()
        ws = np.zeros(plan.pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8) if with_ws else None
        plan.blind_rotate_batch(acc_h, host(lut_t, dt(p)).copy(), host(rot_t, np.uint32).copy(), host(bsk, dt(p)).copy(), L, k, beta, ell,
                                workspace=ws, lut_per_element=per_element)
        acc = dev(torch, acc_h)
    else:
        ws = workspace(torch, plan, L, k, ell, batch) if with_ws else None
        plan.blind_rotate_batch(acc, lut_t, rot_t, bsk, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    want = per_iteration_reference(torch, plan, p, lut_t, per_element, rot_t, bsk, L, k, beta, ell, batch)
    assert torch.equal(acc, want), (p, n, k, L, batch, per_element, with_ws, where, "blind_rotate_batch differs from the per-iteration calls")
    assert L == 0 or bool(acc.any())


COVER = [(0, 1, False, False), (1, 3, True, True), (5, 3, False, True), (5, 1, True, False)]      # (L, batch, per-element lut, workspace)
# the host path with and without a workspace, and lwe_dim = 0 (the set-up alone: no digits, no key, a workspace the call does not
# touch) on the two paths COVER leaves out: (L, batch, per-element lut, workspace, where)
COVER_FRAMES = [(2, 2, False, True, "host"), (2, 2, True, False, "host"), (0, 2, False, True, "device"), (0, 2, True, False, "host")]


@pytest.mark.parametrize("n,k", [(1024, 1), (1024, 2), (64, 1), (64, 2), (4096, 1), (1024, 4), (64, 4)])
@pytest.mark.parametrize("p", ALL)
def test_blind_rotate_equals_per_iteration_calls(p, n, k):
    """n = 1024 and 64: the fused chain; n = 4096 on 64-bit words and k + 1 = 5: the composed path"""
    torch = _torch()
    for L, batch, per_element, with_ws in COVER:
        check_blind_rotate(torch, p, n, k, L, batch, per_element, with_ws)
    if (n, k) == (64, 1):
        for L, batch, per_element, with_ws, where in COVER_FRAMES:
            check_blind_rotate(torch, p, n, k, L, batch, per_element, with_ws, where=where)


@pytest.mark.parametrize("p", [P30, P32])
def test_blind_rotate_equals_per_iteration_calls_composed_u32(p):
    torch = _torch()
    check_blind_rotate(torch, p, 8192, 1, 5, 3, False, True)
    check_blind_rotate(torch, p, 8192, 2, 1, 1, True, False)


# -- 5. blind rotation against the big-integer model --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("p", EXACT)
def test_blind_rotate_matches_big_integer_model(p, n):
    """acc' = acc + sum_j digit_j(X^a acc - acc) (*) key_j mod p with schoolbook negacyclic products on Python ints; the key buffer
    holds n^-1 fwd(key) (fwd_batch, then normalize_batch), as the header prescribes."""
    torch = _torch()
    n = max(n, min_n(p))
    k, L, batch = 1, 2, 2
    beta, ell = (16, 4) if wbits(p) == 64 else (7, 3)
    npolys = k + 1
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("model", p, n))
    lut_a = random_words(rng, p, npolys * n)
    rot = rot_rows(rng, n, L, batch)
    key_a = random_words(rng, p, L * npolys * ell * npolys * n)
    acc_t = zeros(torch, p, batch * npolys * n)
    plan.blind_rotate_batch(acc_t, dev(torch, lut_a), dev(torch, rot), key_ntt(torch, plan, key_a), L, k, beta, ell)
    torch.cuda.synchronize()
    got = [int(x) for x in host(acc_t, dt(p))]
    lut_i, key_i = [int(x) for x in lut_a], [int(x) for x in key_a]
    keyp = [key_i[j * n:(j + 1) * n] for j in range(len(key_i) // n)]
    for b in range(batch):
        acc = [source(lut_i[q * n:(q + 1) * n], int(rot[L * batch + b]), p, "rotate") for q in range(npolys)]
        for i in range(L):
            terms = model_terms_element(acc, int(rot[i * batch + b]), p, beta, ell)
            base = i * npolys * ell * npolys
            new = []
            for o in range(npolys):
                add = [0] * n
                for j, t in enumerate(terms):
                    add = [(x + y) % p for x, y in zip(add, negacyclic(t, keyp[base + j * npolys + o], p))]
                new.append([(x + y) % p for x, y in zip(acc[o], add)])
            acc = new
        assert got[b * npolys * n:(b + 1) * npolys * n] == [x for q in acc for x in q], (p, n, "element", b)


# -- 6. bootstrap == its three steps -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,n,where,with_ws", [(P62, 1024, "device", True), (P62, 1024, "device", False), (PM64, 64, "device", True),
                                               (P63, 4096, "device", False), (P30, 1024, "host", False), (PM64, 1024, "host", True),
                                               (P32, 64, "device", True)])
def test_bootstrap_equals_its_three_steps(p, n, where, with_ws):
    check_bootstrap_steps(p, n, where, with_ws, L=4, batch=5)


@pytest.mark.parametrize("p,where,with_ws", [(P62, "device", True), (P62, "device", False), (P30, "host", True)])
def test_bootstrap_without_mask_words_equals_its_three_steps(p, where, with_ws):
    """lwe_dim = 0: the body alone -- no iteration, no key, and of the workspace only rot_t and the accumulator"""
    check_bootstrap_steps(p, 64, where, with_ws, L=0, batch=2)


def check_bootstrap_steps(p, n, where, with_ws, L, batch):
    torch = _torch()
    plan = make_plan(p, n)
    k, beta, ell = 1, 7, 3
    rng = np.random.default_rng(seed("boot", p, n, where))
    lwe_a = random_words(rng, p, batch * (L + 1))
    lut_a = random_words(rng, p, (k + 1) * n)
    key_a = random_words(rng, p, L * (k + 1) * ell * (k + 1) * n)
    if where == "host":
        to, fro = (lambda a: a.copy()), (lambda a, d: a)
        ws = np.zeros(plan.pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8) if with_ws else None
    else:
        to, fro = (lambda a: dev(torch, a)), host
        ws = workspace(torch, plan, L, k, ell, batch) if with_ws else None
    lwe_t, lut_t, bsk = to(lwe_a), to(lut_a), to(key_a)
    one = to(np.zeros(batch * (k * n + 1), dtype=dt(p)))
    plan.bootstrap_batch(one, lwe_t, lut_t, bsk, L, k, beta, ell, workspace=ws)
    rot_t = to(np.zeros((L + 1) * batch, dtype=np.uint32))
    acc = to(np.zeros(batch * (k + 1) * n, dtype=dt(p)))
    steps = to(np.zeros(batch * (k * n + 1), dtype=dt(p)))
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    plan.blind_rotate_batch(acc, lut_t, rot_t, bsk, L, k, beta, ell)
    plan.sample_extract_batch(steps, acc, k, 0)
    if where == "device":
        torch.cuda.synchronize()
    assert np.array_equal(fro(one, dt(p)), fro(steps, dt(p))), (p, n, where, with_ws)
    assert fro(one, dt(p)).any()


# -- 7. graph capture ----------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_bootstrap_with_a_caller_workspace():
    torch = _torch()
    p, n, L, k, beta, ell, batch = P62, 1024, 8, 1, 8, 3, 37
    plan = make_plan(p, n)
    rng = np.random.default_rng(7)
    lwe = dev(torch, random_words(rng, p, batch * (L + 1)))
    lut = dev(torch, random_words(rng, p, (k + 1) * n))
    bsk = dev(torch, random_words(rng, p, L * (k + 1) * ell * (k + 1) * n))
    ws = workspace(torch, plan, L, k, ell, batch)
    eager = zeros(torch, p, batch * (k * n + 1))
    plan.bootstrap_batch(eager, lwe, lut, bsk, L, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.bootstrap_batch(out, lwe, lut, bsk, L, k, beta, ell, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    first = out.clone()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(first, eager) and torch.equal(out, eager)


# -- 8. the bootstrap bootstraps ---------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


@pytest.mark.parametrize("p", [P62, PM64])
def test_bootstrap_evaluates_the_table_on_encrypted_messages(p):
    """n = 1024, k = 1, L = 8, base_log 8, levels 4; binary LWE / GLWE keys, a noiseless bootstrapping key: row (q, l) is a GLWE
    encryption of zero (uniform mask, body = sum_c A_c S_c, the products from mul_ntt_batch) with s_i 2^(W - base_log l) mod p added to
    coefficient 0 of polynomial q.  4 messages under one padding bit, enc(m) = round(m p / 8); the table is X^(-n/8) v0 with
    v0[j] = enc(f(j div n/4)): boxes of n / 4 coefficients shifted by half a box; input noise below 2^20.  Phase convention: body -
    sum a s; coefficient 0 of X^(-m) v is v[m].

    The bound, derived and not measured.  Box selection: the modulus switch errs by at most 1/2 per word, so the exponent sum by at
    most (L + 1) / 2 = 4.5, plus the noise 2^20 * 2n / p < 1 and the rounding of enc (< 1): below half a box = 128, so the right box is
    read and the table contributes enc(f(m)) exactly.  With a noiseless key the only error left is the gadget rounding: at most
    2^(s-1) per word with s = W - base_log levels, which enters the phase through the body (once) and through k products with a binary
    key polynomial (n coefficients each), once per iteration whose key bit is set:
        |phase - enc(f(m))| <= L (1 + k n) 2^(W - base_log levels - 1)."""
    torch = _torch()
    n, k, beta, ell, L, reps = 1024, 1, 8, 4, 8, 8
    W = wbits(p)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("functional", p))
    s = [int(x) for x in rng.integers(0, 2, size=L)]
    S = rng.integers(0, 2, size=k * n).astype(np.uint64)
    rows = (k + 1) * ell
    key = np.zeros((L, rows, k + 1, n), dtype=np.uint64)
    key[:, :, :k, :] = random_words(rng, p, L * rows * k * n).reshape(L, rows, k, n)
    # body = sum_c A_c S_c through the plan: mul_ntt_batch multiplies by the polynomial whose forward transform it is given
    S_ntt = dev(torch, np.ascontiguousarray(np.broadcast_to(S.reshape(1, 1, k, n), (L, rows, k, n))).reshape(-1))
    plan.fwd_batch(S_ntt)
    prod = dev(torch, np.ascontiguousarray(key[:, :, :k, :]).reshape(-1))
    plan.mul_ntt_batch(prod, S_ntt)
    torch.cuda.synchronize()
    prod_h = host(prod, np.uint64).reshape(L, rows, k, n)
    for i in range(L):
        for j in range(rows):
            body = [0] * n
            for c in range(k):
                body = [(x + int(y)) % p for x, y in zip(body, prod_h[i, j, c])]
            key[i, j, k, :] = np.array(body, dtype=np.uint64)
    for i in range(L):
        for q in range(k + 1):
            for l in range(1, ell + 1):
                j = q * ell + l - 1
                key[i, j, q, 0] = (int(key[i, j, q, 0]) + s[i] * pow(2, W - beta * l, p)) % p
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
    plan.bootstrap_batch(lwe_out, dev(torch, lwe_in.reshape(-1)), dev(torch, lut), bsk, L, k, beta, ell)
    torch.cuda.synchronize()
    ct = host(lwe_out, np.uint64).reshape(batch, k * n + 1)
    Si = [int(x) for x in S]
    bound = L * (1 + k * n) * 2 ** (W - beta * ell - 1)
    worst = 0
    for b in range(batch):
        phase = (int(ct[b, k * n]) - sum(int(x) * y for x, y in zip(ct[b, :k * n], Si))) % p
        err = (phase - enc(pbs_f(msgs[b]))) % p
        err = err if err <= p // 2 else err - p
        worst = max(worst, abs(err))
        assert ((16 * phase + p) // (2 * p)) % 8 == pbs_f(msgs[b]), (p, b, msgs[b], phase)          # round(phase 8 / p) mod 8
    print("largest |phase error| = %d, bound = %d" % (worst, bound))
    assert worst <= bound, (worst, bound)


# -- 9. the C example -----------------------------------------------------------------------------------------------------------------------
def test_pbs_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pbs_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pbs_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 4 and not any("WRONG" in ln for ln in lines), r.stdout
