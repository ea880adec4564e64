"""The ring automorphism, the Galois keyswitch and the trace of the native plans (include/cntt_automorphism.h) on the MI355X.  Bit-exact
throughout, no tolerance anywhere but in the one functional test: call 1 against the plain-int model for the three word types, both
settings of the "autom_lds" switch, the staging edge and a second grid trip; call 2 against the model's permutation of what
cntt_native_fwd_batch wrote, against cntt_native_fwd_batch of sigma_t f where sigma_t negates only zero words, and through
cntt_native_inv_batch; call 3 against the sequence of public calls the header defines it by and against the model; call 4 against
`steps` calls of 3, the closed form on noise-free keys and encrypted messages under noisy keys, whose derived noise bound stands in the
test's docstring; the C example.

The plans start at n = 32 (30-bit residue primes) and n = 16 (50-bit ones), so the smallest polynomial any call here can see is n = 16
on a Plan52 kind: the kernels' one-vector-per-polynomial corner (n = 4 on 32-bit words) cannot be reached through a plan."""
import os
import random
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_automorphism_model import (autom_gather, autom_gather_np, automorphism_key, model_autoks, ntt_permutation, phase, trace_exponents,
                                       trace_keys)
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, per, random_words, seed, to_array, to_ints, wbits
from test_gpu_prime_pack import first_difference, negacyclic_matrix, times_binary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_BINARY = ["native32_plan32", "native64_plan32", "native128_plan32", "native32_plan52", "native64_plan52"]


def min_n(kind):
    return 16 if kind.endswith("plan52") else 32


def negw(plan, a):
    """-a mod 2^w on a word array"""
    with np.errstate(over="ignore"):
        if plan.WORD != 16:
            return (np.zeros_like(a) - a).astype(plan.word_dtype)
        out = np.empty_like(a)
        out[0::2] = np.uint64(0) - a[0::2]
        out[1::2] = ~a[1::2] + (a[0::2] == 0).astype(np.uint64)
        return out


def addw(plan, a, b):
    with np.errstate(over="ignore"):
        if plan.WORD != 16:
            return (a + b).astype(plan.word_dtype)
        out = np.empty_like(a)
        out[0::2] = a[0::2] + b[0::2]
        out[1::2] = a[1::2] + b[1::2] + (out[0::2] < a[0::2]).astype(np.uint64)
        return out


def sigma(plan, a, t):
    """sigma_t on a word array of whole polynomials, numpy: the gather form of the header"""
    n = plan.ntt_size()
    u = np.arange(n, dtype=np.int64) * pow(t, -1, 2 * n) % (2 * n)
    if plan.WORD != 16:
        return autom_gather_np(a.reshape(-1, n), t).reshape(-1)
    x = a.reshape(-1, n, 2)[:, u % n, :]
    neg = negw(plan, np.ascontiguousarray(x).reshape(-1)).reshape(x.shape)
    return np.where((u >= n)[None, :, None], neg, x).reshape(-1)


def poison(plan, words):
    return np.full(words * (2 if plan.WORD == 16 else 1), 0x5A5A5A5A5A5A5A5A & np.iinfo(plan.word_dtype).max, dtype=plan.word_dtype)


def exponents(rng, n):
    return [1, 3, n + 1, 2 * n - 1, 2 * int(rng.integers(n)) + 1]


# -- 1. the coefficient-domain map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("kind,n", [("native32_plan52", 16), ("native64_plan52", 16), ("native32_plan32", 32), ("native64_plan32", 32),
                                    ("native128_plan32", 32), ("native32_plan32", 64), ("native64_plan32", 64), ("native128_plan32", 64)])
def test_automorphism_matches_the_model(kind, n, lds):
    """u32, u64 and u128 words at the smallest sizes the plans have, t in {1, 3, n + 1, 2n - 1, random}, device and host path; the numpy
    gather itself is pinned to the plain-int model on the first polynomial"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("autom", kind, n))
    a = random_words(rng, plan, 5 * n)
    a[:per(plan) // 4] = 0
    a[per(plan) // 4:per(plan) // 2] = np.iinfo(plan.word_dtype).max
    with cntt.debug_switches(autom_lds=lds):
        for t in exponents(rng, n):
            want = sigma(plan, a, t)
            assert to_ints(plan, want[:per(plan)]) == autom_gather(to_ints(plan, a[:per(plan)]), t, wbits(plan))
            out_t = dev(torch, poison(plan, 5 * n))
            plan.automorphism_batch(out_t, dev(torch, a), t)
            torch.cuda.synchronize()
            got = host(out_t, plan.word_dtype)
            assert np.array_equal(got, want), (kind, n, t, first_difference(got, want))
            out_h = poison(plan, 5 * n)
            plan.automorphism_batch(out_h, a, t)
            assert np.array_equal(out_h, want), (kind, n, t, "host")


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("kind,n", [("native128_plan32", 4096), ("native128_plan32", 8192), ("native64_plan32", 8192), ("native64_plan32", 16384),
                                    ("native32_plan32", 16384), ("native32_plan32", 32768)])
def test_automorphism_at_the_staging_edge(kind, n, lds):
    """the last polynomial of each word type that is staged through LDS (64 KiB) and the first that is not"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("autom-edge", kind, n))
    a = random_words(rng, plan, 3 * n)
    with cntt.debug_switches(autom_lds=lds):
        for t in (n + 1, 2 * n - 1, 2 * int(rng.integers(n)) + 1):
            out_t = dev(torch, poison(plan, 3 * n))
            plan.automorphism_batch(out_t, dev(torch, a), t)
            torch.cuda.synchronize()
            got, want = host(out_t, plan.word_dtype), sigma(plan, a, t)
            assert np.array_equal(got, want), (kind, n, t, first_difference(got, want))


@pytest.mark.parametrize("kind", ["native32_plan32", "native64_plan32", "native128_plan32"])
def test_automorphism_makes_a_second_grid_trip(kind):
    """more polynomials than cntt_native_automorphism_grid returns, at n = 32: the tail is served by a second, ragged trip"""
    torch = _torch()
    n = 32
    plan = KINDS[kind].try_new(n)
    cap = cntt.lib().cntt_native_automorphism_grid(1 << 30, 5, plan.WORD)
    polys = cap + 5
    assert cntt.lib().cntt_native_automorphism_grid(polys, 5, plan.WORD) == cap
    rng = np.random.default_rng(seed("autom-trip", kind))
    a = random_words(rng, plan, polys * n)
    for lds in (1, 0):
        with cntt.debug_switches(autom_lds=lds):
            out_t = dev(torch, poison(plan, polys * n))
            plan.automorphism_batch(out_t, dev(torch, a), 2 * n - 3)
            torch.cuda.synchronize()
            got, want = host(out_t, plan.word_dtype), sigma(plan, a, 2 * n - 3)
            assert np.array_equal(got, want), (kind, lds, first_difference(got, want))


# -- 2. the slot permutation of the residue planes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("n", [32, 2048])
@pytest.mark.parametrize("kind", ["native64_plan32", "native64_plan52"])
def test_automorphism_ntt_against_fwd_batch(kind, n, lds):
    """One kind per residue width.  On what cntt_native_fwd_batch wrote, call 2 is the model's permutation, plane for plane and word for
    word; cntt_native_inv_batch of its output is sigma_t f; and where sigma_t negates only zero words -- f zeroed at the sources
    u >= n -- it equals cntt_native_fwd_batch(sigma_t f) word for word.  (On words it does negate the two differ by the planes of 2^w
    times a 0 / 1 polynomial, as the header says: the transform reads words as unsigned integers.)"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("autom-ntt", kind, n))
    polys = 3
    res_t = torch.int64 if plan.RES == 8 else torch.int32

    def planes():
        return [torch.zeros(polys * n, dtype=res_t, device="cuda") for _ in range(plan.NPRIMES)]

    with cntt.debug_switches(autom_lds=lds):
        for t in exponents(rng, n):
            f = random_words(rng, plan, polys * n)
            fhat, out = planes(), planes()
            plan.fwd_batch(dev(torch, f), fhat)
            plan.automorphism_ntt_batch(out, fhat, t)
            torch.cuda.synchronize()
            src = ntt_permutation(t, n)
            for i in range(plan.NPRIMES):
                got, want = host(out[i], plan.res_dtype), host(fhat[i], plan.res_dtype).reshape(polys, n)[:, src].reshape(-1)
                assert np.array_equal(got, want), (kind, n, t, i, first_difference(got, want))
            # both plane sets stand for sigma_t f mod 2^w: inv_batch returns the same words from either
            direct = planes()
            plan.fwd_batch(dev(torch, sigma(plan, f, t)), direct)
            back, back_direct = (torch.zeros(polys * n, dtype=torch.int64, device="cuda") for _ in range(2))
            plan.inv_batch(back, out)
            plan.inv_batch(back_direct, direct)
            torch.cuda.synchronize()
            assert bool(back.any()) and torch.equal(back, back_direct), (kind, n, t, "inv")
            # the word-for-word identity with fwd_batch where no non-zero word is negated
            u = np.arange(n, dtype=np.int64) * pow(t, -1, 2 * n) % (2 * n)
            g = f.reshape(polys, n).copy()
            g[:, (u % n)[u >= n]] = 0
            g = g.reshape(-1)
            ghat, direct = planes(), planes()
            plan.fwd_batch(dev(torch, g), ghat)
            plan.automorphism_ntt_batch(out, ghat, t)
            plan.fwd_batch(dev(torch, sigma(plan, g, t)), direct)
            torch.cuda.synchronize()
            for i in range(plan.NPRIMES):
                assert torch.equal(out[i], direct[i]) and bool(out[i].any()), (kind, n, t, i, "fwd of sigma")
    # the host path, once
    f = random_words(rng, plan, polys * n)
    fhat = [np.zeros(polys * n, dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
    out = [np.full(polys * n, 7, dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
    plan.fwd_batch(f.copy(), fhat)
    plan.automorphism_ntt_batch(out, fhat, n + 1)
    src = ntt_permutation(n + 1, n)
    for i in range(plan.NPRIMES):
        assert np.array_equal(out[i], fhat[i].reshape(polys, n)[:, src].reshape(-1)), (kind, n, i, "host")


# -- 3. the Galois keyswitch -------------------------------------------------------------------------------------------------------------
def ak_planes(torch, plan, rng, k, ell, keys=1):
    """the residue planes of `keys` random automorphism keys: the statements are about the words"""
    return key_planes(torch, plan, random_words(rng, plan, keys * k * ell * (k + 1) * plan.ntt_size()))


def run_autoks(torch, plan, where, ct, kr, t, k, beta, ell, add, with_ws=False, stream=None):
    n = plan.ntt_size()
    batch = ct.size // ((k + 1) * per(plan))
    out = poison(plan, batch * (k + 1) * n)
    nws = plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws and nws else None
        plan.glwe_automorphism_keyswitch_batch(out, ct, [host(p, plan.res_dtype).copy() for p in kr] if k else None, t, k, beta, ell, add, workspace=ws)
        return out
    out_t, ct_t = dev(torch, out), dev(torch, ct)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    if stream is None:
        plan.glwe_automorphism_keyswitch_batch(out_t, ct_t, kr if k else None, t, k, beta, ell, add, workspace=ws)
    else:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            plan.glwe_automorphism_keyswitch_batch(out_t, ct_t, kr, t, k, beta, ell, add, workspace=ws)
        stream.synchronize()
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def compose_autoks(torch, plan, ct, kr, t, k, beta, ell, add):
    """The header's sequence of public calls: the prefill on the host, automorphism_batch on the k masks, gadget_decompose_batch(plain),
    every digit negated mod 2^w, external_product_batch(accumulate=True)."""
    pe = per(plan)
    batch = ct.size // ((k + 1) * pe)
    c = ct.reshape(batch, k + 1, pe)
    out = np.zeros_like(c)
    out[:, k] = sigma(plan, np.ascontiguousarray(c[:, k]).reshape(-1), t).reshape(batch, pe)
    if add:
        out = addw(plan, out.reshape(-1), ct).reshape(batch, k + 1, pe)
    out_t = dev(torch, out.reshape(-1))
    if k:
        masks = dev(torch, np.ascontiguousarray(c[:, :k]).reshape(-1))
        perm = torch.zeros_like(masks)
        plan.automorphism_batch(perm, masks, t)
        terms = torch.zeros(perm.numel() * ell, dtype=perm.dtype, device="cuda")
        plan.gadget_decompose_batch(terms, perm, beta, ell, mode="plain")
        if plan.WORD == 16:
            torch.cuda.synchronize()
            terms = dev(torch, negw(plan, host(terms, np.uint64)))
        else:
            terms = -terms                                             # wraps: the negation mod 2^w
        plan.external_product_batch(out_t, terms, kr, k * ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def worst_words(plan, beta, ell):
    """all ones, 2^(w-1), and the word whose every digit is -B/2"""
    w = wbits(plan)
    low = sum((-(1 << (beta - 1))) << (w - beta * l) for l in range(1, ell + 1)) % (1 << w)
    return [(1 << w) - 1, 1 << (w - 1), low]


def ciphertexts(rng, plan, polys, beta, ell):
    """random words; the first three polynomials are filled with the worst-case words, and zeros are sprinkled over the rest"""
    pe, n = per(plan), plan.ntt_size()
    a = random_words(rng, plan, polys * n)
    for i, x in enumerate(worst_words(plan, beta, ell)[:polys]):
        a[i * pe:(i + 1) * pe] = to_array(plan, [x] * n)
    a[min(3, polys) * pe::11] = 0
    return a


def gadgets(w):
    """(base_log, levels): full-word digits (s = 0); rounded digits (s > 0); base_log * levels far below w"""
    return [(w // 4, 4), (7, 3), (2, 2)] + ([(40, 1)] if w == 64 else [(45, 2)] if w == 128 else [])


@pytest.mark.parametrize("kind", NON_BINARY)
def test_autoks_equals_the_public_calls_for_every_kind(kind):
    """the smallest size of the kind, k = 0, 1, 2, batch 3, with and without add_input, with a caller workspace and with NULL; the first
    case also against the plain-int model of the formula"""
    torch = _torch()
    plan = KINDS[kind].try_new(min_n(kind))
    n, pe, w = plan.ntt_size(), per(plan), wbits(plan)
    rng = np.random.default_rng(seed("autoks", kind))
    for k in (0, 1, 2):
        for gi, (beta, ell) in enumerate(gadgets(w)):
            assert k * ell <= plan.max_terms()
            key_words = random_words(rng, plan, k * ell * (k + 1) * n)
            kr = key_planes(torch, plan, key_words)
            ct = ciphertexts(rng, plan, 3 * (k + 1), beta, ell)
            for t in (3, n + 1, 2 * n - 1)[:2 if gi else 3]:
                for add in (False, True):
                    want = compose_autoks(torch, plan, ct, kr, t, k, beta, ell, add)
                    for with_ws in (False, True):
                        got = run_autoks(torch, plan, "device", ct, kr, t, k, beta, ell, add, with_ws)
                        assert got.any() and np.array_equal(got, want), (kind, n, k, beta, ell, t, add, with_ws, first_difference(got, want))
            if gi == 1 and k == 1:
                one = to_ints(plan, ct[:(k + 1) * pe])
                model = model_autoks(one, to_ints(plan, key_words), w, 3, k, n, beta, ell, True)
                got = run_autoks(torch, plan, "device", ct, kr, 3, k, beta, ell, True)
                assert to_ints(plan, got[:(k + 1) * pe]) == model, (kind, "model")


@pytest.mark.parametrize("kind,n,k", [("native32_plan32", 4096, 1), ("native64_plan32", 4096, 2), ("native64_plan52", 16, 1), ("native32_plan32", 8192, 1),
                                      ("native64_plan32", 8192, 1), ("native128_plan32", 8192, 1)])
def test_autoks_size_classes(kind, n, k):
    """n = 4096, the last fused size (and the last staged 128-bit polynomial is covered by call 1); n = 16 on a Plan52 kind and n = 8192:
    the composed external product; both settings of the switch"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("autoks-large", kind, n))
    beta, ell, batch = 7, 2, 2
    kr = ak_planes(torch, plan, rng, k, ell)
    ct = ciphertexts(rng, plan, batch * (k + 1), beta, ell)
    t = 2 * int(rng.integers(n)) + 1
    for add in (False, True):
        want = compose_autoks(torch, plan, ct, kr, t, k, beta, ell, add)
        for lds in (1, 0):
            with cntt.debug_switches(autom_lds=lds):
                got = run_autoks(torch, plan, "device", ct, kr, t, k, beta, ell, add, with_ws=bool(lds))
            assert got.any() and np.array_equal(got, want), (kind, n, add, lds, first_difference(got, want))


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32"])
def test_autoks_on_the_host_path_and_on_a_stream(kind):
    torch = _torch()
    beta, ell, batch, n = 6, 3, 3, 64
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("autoks-host", kind))
    for k in (1, 0):
        kr = ak_planes(torch, plan, rng, k, ell)
        ct = ciphertexts(rng, plan, batch * (k + 1), beta, ell)
        want = compose_autoks(torch, plan, ct, kr, n + 1, k, beta, ell, True)
        for with_ws in (True, False):
            got = run_autoks(torch, plan, "host", ct, kr, n + 1, k, beta, ell, True, with_ws)
            assert got.any() and np.array_equal(got, want), (kind, k, with_ws, first_difference(got, want))
    got = run_autoks(torch, plan, "device", ct, kr, n + 1, 0, beta, ell, True, True)
    assert np.array_equal(got, want)
    k = 1
    kr = ak_planes(torch, plan, rng, k, ell)
    ct = ciphertexts(rng, plan, batch * (k + 1), beta, ell)
    want = compose_autoks(torch, plan, ct, kr, 5, k, beta, ell, False)
    got = run_autoks(torch, plan, "device", ct, kr, 5, k, beta, ell, False, True, stream=torch.cuda.Stream())
    assert got.any() and np.array_equal(got, want), (kind, "stream", first_difference(got, want))


@pytest.mark.parametrize("kind", ["native64_plan32", "native32_plan32"])
def test_autoks_makes_a_second_grid_trip(kind):
    torch = _torch()
    n, k, beta, ell = 32, 1, 5, 2
    plan = KINDS[kind].try_new(n)
    cap = cntt.lib().cntt_native_automorphism_grid(1 << 30, 5, plan.WORD)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_native_automorphism_grid(batch * (k + 1), 5, plan.WORD) == cap < batch * (k + 1) < 2 * cap
    rng = np.random.default_rng(seed("autoks-ragged", kind))
    kr = ak_planes(torch, plan, rng, k, ell)
    ct = random_words(rng, plan, batch * (k + 1) * n)
    got = run_autoks(torch, plan, "device", ct, kr, 2 * n - 1, k, beta, ell, True)
    want = compose_autoks(torch, plan, ct, kr, 2 * n - 1, k, beta, ell, True)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], poison(plan, 3 * (k + 1) * n))


def test_graph_capture_of_the_trace_with_a_caller_workspace():
    """native64 Plan32, n = 1024, k = 1: the whole trace (10 keyswitches) captured once and replayed twice on fresh inputs"""
    torch = _torch()
    n, k, beta, ell, batch, steps = 1024, 1, 8, 3, 2, 10
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(27)
    kr = ak_planes(torch, plan, rng, k, ell, steps)
    ct = dev(torch, random_words(rng, plan, batch * (k + 1) * n))
    ws = torch.zeros(plan.glwe_trace_workspace_bytes(k, ell, batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(plan, batch * (k + 1) * n))
    plan.glwe_trace_batch(out, ct, kr, steps, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.glwe_trace_batch(out, ct, kr, steps, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, plan, batch * (k + 1) * n))
        eager = torch.zeros_like(out)
        plan.glwe_trace_batch(eager, fresh, kr, steps, k, beta, ell)
        ct.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 4. the trace ------------------------------------------------------------------------------------------------------------------------
def run_trace(torch, plan, ct, kr, steps, k, beta, ell, with_ws):
    n = plan.ntt_size()
    batch = ct.size // ((k + 1) * per(plan))
    out_t = dev(torch, poison(plan, batch * (k + 1) * n))
    ws = torch.zeros(max(plan.glwe_trace_workspace_bytes(k, ell, batch), 16), dtype=torch.uint8, device="cuda") if with_ws else None
    keys = [p[:steps * k * ell * (k + 1) * n] for p in kr] if k and steps else None   # the first `steps` keys
    plan.glwe_trace_batch(out_t, dev(torch, ct), keys, steps, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


@pytest.mark.parametrize("kind,n,k", [("native64_plan32", 32, 1), ("native32_plan32", 64, 2), ("native128_plan32", 32, 1), ("native64_plan52", 64, 0)])
def test_trace_equals_steps_calls_of_the_keyswitch(kind, n, k):
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    logn, beta, ell, batch = n.bit_length() - 1, 6, 2, 3
    rng = np.random.default_rng(seed("trace", kind, n))
    kr = ak_planes(torch, plan, rng, k, ell, logn)
    per_key = k * ell * (k + 1) * n
    ct = ciphertexts(rng, plan, batch * (k + 1), beta, ell)
    for steps in (0, 1, logn):
        cur = ct
        for r, t in enumerate(trace_exponents(n, steps)):
            cur = run_autoks(torch, plan, "device", cur, [p[r * per_key:(r + 1) * per_key] for p in kr], t, k, beta, ell, True)
        for with_ws in (True, False):
            got = run_trace(torch, plan, ct, kr, steps, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, cur), (kind, n, steps, with_ws, first_difference(got, cur))
    # the host path, the full trace
    out = poison(plan, batch * (k + 1) * n)
    plan.glwe_trace_batch(out, ct, [host(p, plan.res_dtype).copy() for p in kr] if k else None, logn, k, beta, ell)
    assert np.array_equal(out, cur), (kind, n, "host")


@pytest.mark.parametrize("w,n", [(64, 32), (32, 64)])
def test_trace_on_noise_free_keys_is_the_closed_form(w, n):
    """s = 0, k = 1, binary key: coefficient i of the phase becomes 2^steps phase[i] mod 2^w where 2^steps divides i and 0 elsewhere"""
    torch = _torch()
    kind = "native%d_plan32" % w
    plan = KINDS[kind].try_new(n)
    logn, k, beta, ell = n.bit_length() - 1, 1, w // 4, 4
    rnd = random.Random("native-trace-closed/%d" % w)
    S = [[rnd.randrange(2) for _ in range(n)]]
    keys = trace_keys(rnd, w, S, logn, n, beta, ell)
    kr = key_planes(torch, plan, to_array(plan, keys))
    ct = [rnd.randrange(1 << w) for _ in range((k + 1) * n)]
    ph = phase(ct, S, w)
    for steps in (0, 1, logn):
        got = run_trace(torch, plan, to_array(plan, ct), kr, steps, k, beta, ell, True)
        want = [(ph[i] << steps) % (1 << w) if i % (1 << steps) == 0 else 0 for i in range(n)]
        assert phase(to_ints(plan, got), S, w) == want, (w, n, steps)


def test_trace_decodes_every_message_under_noisy_keys():
    """native64 Plan32, n = 64, k = 1, binary key, base_log 16, levels 4 (s = 0: no rounding), the full trace of steps = log2 n = 6.
    One ciphertext per 3-bit message value m: the constant coefficient of the plaintext is m at bit 64 - 6 - 3 = 55 -- six bits of headroom
    below the message, as the header asks -- the other coefficients carry random 3-bit values there, and the encryption noise is below
    E0 = 2^10.  The keys have noise below E = 2^10 per coefficient.  After the trace the constant coefficient of the phase is
    2^6 (2^55 m + e) = 2^61 m + error, decoded from the top three bits, correct for EVERY message.
    Error bound, derived: one keyswitch adds sum over its k * levels term polynomials of digit (*) row noise, each coefficient a sum of n
    products of a digit (at most B / 2 = 2^15 in size) and a noise word (below E): at most KS = k levels n (B / 2) E = 4 * 64 * 2^15 * 2^10 =
    2^33.  A stage maps an error e to e + sigma(e) + ks, at most 2 |e| + KS, so after 6 stages it is at most 2^6 E0 + (2^6 - 1) KS <
    2^16 + 2^39, asserted; half a message step is 2^60.  The measured worst error is printed next to it."""
    torch = _torch()
    n, k, beta, ell, w = 64, 1, 16, 4, 64
    logn = 6
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(seed("native-trace-noisy"))
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    E0 = E = 1 << 10
    key = []
    for t in trace_exponents(n, logn):
        rot = np.array(autom_gather([int(s) for s in S], t, w), dtype=object)          # sigma_t(S) mod 2^64: words 0, 1 and 2^64 - 1
        A = rng.integers(0, 2 ** 64, size=(ell, n), dtype=np.uint64).astype(object)
        body = times_binary(A, NS) + rng.integers(-E + 1, E, size=(ell, n)).astype(object)
        for l in range(1, ell + 1):
            body[l - 1] += rot * (1 << (w - beta * l))
        key.append(np.stack([(A % 2 ** 64).astype(np.uint64), (body % 2 ** 64).astype(np.uint64)], axis=1).reshape(-1))
    kr = key_planes(torch, plan, np.concatenate(key))
    msgs = np.arange(8)
    plain = rng.integers(0, 8, size=(8, n)).astype(object)
    plain[:, 0] = msgs
    a = rng.integers(0, 2 ** 64, size=(8, n), dtype=np.uint64).astype(object)
    b = times_binary(a, NS) + plain * (1 << 55) + rng.integers(-E0 + 1, E0, size=(8, n)).astype(object)
    ct = np.stack([(a % 2 ** 64).astype(np.uint64), (b % 2 ** 64).astype(np.uint64)], axis=1).reshape(-1)
    got = run_trace(torch, plan, ct, kr, logn, k, beta, ell, True).reshape(8, 2, n)
    ph = (got[:, 1].astype(object) - times_binary(got[:, 0], NS)) % 2 ** 64
    const = [int(x) for x in ph[:, 0]]
    dec = [(((x >> 60) + 1) >> 1) & 7 for x in const]
    assert dec == msgs.tolist(), dec
    err = [(x - (m << 61)) % 2 ** 64 for x, m in zip(const, msgs.tolist())]
    others = [int(x) for x in ph[:, 1:].reshape(-1)]                                    # the coefficients the trace kills hold error only
    worst = max(min(e, 2 ** 64 - e) for e in err + others)
    bound = (1 << logn) * E0 + ((1 << logn) - 1) * k * ell * n * (1 << (beta - 1)) * E
    assert bound == (1 << 16) + 63 * (1 << 33)
    print("native trace n = %d: worst error 2^%.2f over 8 messages x %d coefficients, derived bound 2^%.2f" % (n, np.log2(max(worst, 1)), n, np.log2(bound)))
    assert worst < bound


# -- 5. the C example ----------------------------------------------------------------------------------------------------------------------
def test_trace_native_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "trace_native"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "trace_native")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
