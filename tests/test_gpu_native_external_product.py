"""cntt_native_external_product_batch (include/cntt_ext.h) on the MI355X, bit-exact against the CPU oracle:
    out[b][o] (+)= sum_j terms[b][j] (*) key[j][o]   mod 2^w
expected = the sum mod 2^w of the oracle's negacyclic_polymul (the reference's per-kind CRT) over the terms.  The key goes in as the
residues cntt_native_fwd_batch (fwd_binary for the binary kinds) writes.  Covers the ten kinds, the fused kernel (Plan32, n <= 4096)
and the composed pipeline (larger n, Plan52, switch "native_ext" = 0), the exactness bound at cntt_native_max_terms(), the empty
sum, host slices and one hipGraph capture."""
import zlib

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import (native32, native64, native128, native_binary32, native_binary64, native_binary128)

pytestmark = pytest.mark.gpu

KINDS = {"native32_plan32": native32.Plan32, "native64_plan32": native64.Plan32, "native128_plan32": native128.Plan32,
         "native_binary32_plan32": native_binary32.Plan32, "native_binary64_plan32": native_binary64.Plan32,
         "native_binary128_plan32": native_binary128.Plan32, "native32_plan52": native32.Plan52,
         "native64_plan52": native64.Plan52, "native_binary32_plan52": native_binary32.Plan52,
         "native_binary64_plan52": native_binary64.Plan52}
PLAN32 = sorted(k for k in KINDS if k.endswith("plan32"))
FUSED_N = [32, 64, 128, 256, 512, 1024, 2048, 4096]


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def wpp(plan):
    """u32 / u64 array elements per polynomial (128-bit words: two u64)."""
    return plan.ntt_size() * (2 if plan.WORD == 16 else 1)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def random_words(rng, plan, npoly, binary=False):
    dt = plan.word_dtype
    if binary:   # binary operand: coefficients 0 / 1 (128-bit words: low word only)
        w = np.zeros(npoly * wpp(plan), dtype=dt)
        bits = rng.integers(0, 2, size=npoly * plan.ntt_size()).astype(dt)
        if plan.WORD == 16:
            w[0::2] = bits
        else:
            w[:] = bits
        return w
    return rng.integers(0, np.iinfo(dt).max, size=npoly * wpp(plan), dtype=dt, endpoint=True)


def wadd(a, b, word):
    """a + b modulo 2^bits(word), elementwise over flat word arrays."""
    if word != 16:
        return a + b   # numpy wraps
    lo = a[0::2] + b[0::2]
    carry = (lo < a[0::2]).astype(np.uint64)
    out = np.empty_like(a)
    out[0::2] = lo
    out[1::2] = a[1::2] + b[1::2] + carry
    return out


def expected(oracle, kind, plan, terms, keyw, batch, nterms, nout):
    """sum_j oracle negacyclic_polymul(terms[b][j], key[j][o]) mod 2^w, as batch*nout polynomials."""
    ref = oracle.Native(kind, plan.ntt_size())
    w = wpp(plan)
    T = terms.reshape(batch, nterms, w)
    K = keyw.reshape(nterms, nout, w)
    lhs = np.ascontiguousarray(np.broadcast_to(T[:, :, None, :], (batch, nterms, nout, w))).reshape(-1)
    rhs = np.ascontiguousarray(np.broadcast_to(K[None, :, :, :], (batch, nterms, nout, w))).reshape(-1)
    prod = np.zeros_like(lhs)
    ref.negacyclic_polymul_batch(prod, lhs, rhs, batch * nterms * nout, 8)
    prod = prod.reshape(batch, nterms, nout * w)
    acc = np.zeros((batch, nout * w), dtype=terms.dtype)
    for j in range(nterms):
        acc = np.stack([wadd(acc[b], prod[b, j], plan.WORD) for b in range(batch)])
    return acc.reshape(-1)


def key_residues(torch, plan, keyw, npoly):
    res_t = torch.int64 if plan.RES == 8 else torch.int32
    kr = [torch.empty(npoly * plan.ntt_size(), dtype=res_t, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(dev(torch, keyw), kr, binary=plan.BINARY)
    return kr


def run_ext(torch, plan, out_np, terms, kr, nterms, nout, accumulate):
    out = dev(torch, out_np.copy())
    plan.external_product_batch(out, dev(torch, terms), kr, nterms, nout, accumulate=accumulate)
    torch.cuda.synchronize()
    return host(out, plan.word_dtype)


def batch_for(n):
    # ragged: one more element than whole workgroups hold (256 threads x 16 coefficients = 4096 / n elements per workgroup)
    return 4096 // n + 1 if n <= 2048 else 2 if n <= 16384 else 1


@pytest.mark.parametrize("jo", [(1, 1), (3, 2), (4, 4), (2, 5)])
@pytest.mark.parametrize("n", [32, 256, 1024, 4096, 16384, 32768])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_external_product_matches_oracle(oracle, kind, n, jo):
    torch = _torch()
    nterms, nout = jo
    plan = KINDS[kind].try_new(n)
    assert plan is not None
    nterms = min(nterms, plan.max_terms())   # native_binary32 Plan52 (one 50-bit prime) allows 3 terms at n = 32768
    batch = batch_for(n)
    if n >= 16384 and nterms * nout > 8:
        batch = 1
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d/%d" % (kind, n, nterms, nout)).encode()))
    terms = random_words(rng, plan, batch * nterms)
    keyw = random_words(rng, plan, nterms * nout, binary=plan.BINARY)
    kr = key_residues(torch, plan, keyw, nterms * nout)
    want = expected(oracle, kind, plan, terms, keyw, batch, nterms, nout)
    prior = random_words(rng, plan, batch * nout)
    got = run_ext(torch, plan, prior, terms, kr, nterms, nout, False)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s n=%d J=%d O=%d: %d words differ, first at %d" % (kind, n, nterms, nout, bad.size, bad[0])
    got = run_ext(torch, plan, prior, terms, kr, nterms, nout, True)
    assert np.array_equal(got, wadd(prior, want, plan.WORD)), (kind, n, jo, "accumulate")


@pytest.mark.parametrize("n", [32, 1024, 16384])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_term_one_output_is_negacyclic_polymul_batch(kind, n):
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    batch = batch_for(n) + 2
    rng = np.random.default_rng(n + len(kind))
    lhs = random_words(rng, plan, batch)
    rhs = random_words(rng, plan, 1, binary=plan.BINARY)
    kr = key_residues(torch, plan, rhs, 1)
    got = run_ext(torch, plan, np.zeros_like(lhs), lhs, kr, 1, 1, False)
    prod = torch.zeros(lhs.size, dtype=torch.int32 if plan.WORD == 4 else torch.int64, device="cuda")
    plan.negacyclic_polymul_batch(prod, dev(torch, lhs), dev(torch, np.tile(rhs, batch)))
    assert np.array_equal(got, host(prod, plan.word_dtype)), kind


@pytest.mark.parametrize("n", FUSED_N)
@pytest.mark.parametrize("kind", PLAN32)
def test_fused_equals_composed(kind, n):
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    nterms, nout = 3, 3
    batch = batch_for(n) + 5
    rng = np.random.default_rng(7 * n + len(kind))
    terms = random_words(rng, plan, batch * nterms)
    kr = key_residues(torch, plan, random_words(rng, plan, nterms * nout, binary=plan.BINARY), nterms * nout)
    prior = random_words(rng, plan, batch * nout)
    for acc in (False, True):
        fused = run_ext(torch, plan, prior, terms, kr, nterms, nout, acc)
        with cntt.debug_switches(native_ext=0):
            composed = run_ext(torch, plan, prior, terms, kr, nterms, nout, acc)
        assert np.array_equal(fused, composed), (kind, n, acc)


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("kind", ["native32_plan32", "native64_plan32", "native_binary64_plan32"])
def test_exact_at_max_terms_and_einval_past_it(oracle, kind, n):
    """All-(2^w - 1) terms against an all-ones key (binary kinds: all 1): coefficient n - 1 of every product is the largest positive
    value n A^2 (n A), so the sum reaches T n A^2 -- the bound max_terms() is computed for.  Identical terms: expected = T x one
    oracle product mod 2^w."""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    T = plan.max_terms()
    dt = plan.word_dtype
    ones = np.full(n, np.iinfo(dt).max, dtype=dt)
    key = np.ones(n, dtype=dt) if plan.BINARY else ones
    ref = oracle.Native(kind, n)
    one = np.zeros(n, dtype=dt)
    ref.negacyclic_polymul(one, ones, key)
    want = (one.astype(np.uint64) * np.uint64(T)).astype(dt)
    tt = torch.int32 if dt == np.uint32 else torch.int64
    terms = torch.full(((T + 1) * n,), -1, dtype=tt, device="cuda")
    keys = dev(torch, np.tile(key, T + 1))
    kr = [torch.empty((T + 1) * n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(keys, kr, binary=plan.BINARY)
    del keys
    for path in (1, 0):
        with cntt.debug_switches(native_ext=path):
            out = torch.zeros(n, dtype=tt, device="cuda")
            plan.external_product_batch(out, terms[:T * n], [r[:T * n] for r in kr], T, 1)
            torch.cuda.synchronize()
            got = host(out, dt)
            assert np.array_equal(got, want), (kind, n, T, "native_ext=%d" % path, np.nonzero(got != want)[0][:4])
    out = torch.full((n,), 5, dtype=tt, device="cuda")
    with pytest.raises(cntt.Panic):
        plan.external_product_batch(out, terms, kr, T + 1, 1)
    torch.cuda.synchronize()
    assert (host(out, dt) == 5).all()


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32", "native64_plan52"])
def test_empty_sum_and_empty_batch(kind):
    torch = _torch()
    plan = KINDS[kind].try_new(256)
    rng = np.random.default_rng(3)
    prior = random_words(rng, plan, 2 * 3)
    kr0 = [torch.empty(0, dtype=torch.int32 if plan.RES == 4 else torch.int64, device="cuda") for _ in range(plan.NPRIMES)]
    empty_terms = np.zeros(0, dtype=plan.word_dtype)
    assert (run_ext(torch, plan, prior, empty_terms, kr0, 0, 3, False) == 0).all()
    assert np.array_equal(run_ext(torch, plan, prior, empty_terms, kr0, 0, 3, True), prior)
    # batch == 0: a no-op
    kr = key_residues(torch, plan, random_words(rng, plan, 2 * 3, binary=plan.BINARY), 6)
    out = dev(torch, np.zeros(0, dtype=plan.word_dtype))
    plan.external_product_batch(out, dev(torch, empty_terms), kr, 2, 3)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1024, 16384])
@pytest.mark.parametrize("kind", ["native64_plan32", "native_binary128_plan32", "native32_plan52"])
def test_host_slices(oracle, kind, n):
    plan = KINDS[kind].try_new(n)
    nterms, nout, batch = 2, 2, 3
    rng = np.random.default_rng(11 + n)
    terms = random_words(rng, plan, batch * nterms)
    keyw = random_words(rng, plan, nterms * nout, binary=plan.BINARY)
    kr = [np.zeros(nterms * nout * n, dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
    plan.fwd_batch(keyw, kr, binary=plan.BINARY)
    want = expected(oracle, kind, plan, terms, keyw, batch, nterms, nout)
    prior = random_words(rng, plan, batch * nout)
    out = prior.copy()
    plan.external_product_batch(out, terms, kr, nterms, nout)
    assert np.array_equal(out, want), kind
    out = prior.copy()
    plan.external_product_batch(out, terms, kr, nterms, nout, accumulate=True)
    assert np.array_equal(out, wadd(prior, want, plan.WORD)), kind


def test_graph_capture_of_the_fused_call():
    torch = _torch()
    plan = native64.Plan32.try_new(1024)
    nterms, nout, batch = 4, 2, 37
    rng = np.random.default_rng(5)
    terms = dev(torch, random_words(rng, plan, batch * nterms))
    kr = key_residues(torch, plan, random_words(rng, plan, nterms * nout), nterms * nout)
    eager = torch.zeros(batch * nout * 1024, dtype=torch.int64, device="cuda")
    plan.external_product_batch(eager, terms, kr, nterms, nout)   # also builds the plan's device tables ahead of the capture
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.external_product_batch(out, terms, kr, nterms, nout)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
