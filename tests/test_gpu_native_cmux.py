"""The CMux and the CMux tree against GGSW selectors on the native plans (include/cntt_cmux.h) on the MI355X.  Bit-exact throughout,
no tolerance anywhere but in the one functional test: call 1 against the sequence of public calls the header states on all ten kinds;
the size classes of the external product; the host path; the tree against the leaf stage from public calls and one glwe_cmux_batch per
stage; the leaf stage against call 1 on trivial ciphertexts; a walk that makes a second, ragged trip; graph capture; the STREAM form at
its first shape; a whole encrypted table lookup through noisy selectors, whose derived noise bound stands in its docstring; the C
example."""
import gc
import os
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_cmux_model import stage_params
from test_gpu_native_pbs import KINDS, STREAM_BYTES, _torch, dev, host, key_planes, per, random_key_words, random_words, seed, wbits
from test_gpu_prime_pack import first_difference, negacyclic_matrix, times_binary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def min_n(kind):
    """the smallest size the plans accept: 32 for the 30-bit residue primes, 16 for the 50-bit ones"""
    return 16 if kind.endswith("plan52") else 32


def sel_polys(k, ell):
    return (k + 1) * ell * (k + 1)


def selectors(torch, plan, rng, k, ell, count=1):
    """the residue planes of `count` random selectors (bits for the binary kinds): the statements are about the words"""
    return key_planes(torch, plan, random_key_words(rng, plan, count * sel_polys(k, ell)))


def selector(plan, kr, i, k, ell):
    sz = sel_polys(k, ell) * plan.ntt_size()
    return [p[i * sz:(i + 1) * sz] for p in kr]


def words_with_zeros(rng, plan, polys):
    """random words with zeros sprinkled over them; from three polynomials on the first is all zero and the second all ones"""
    a = random_words(rng, plan, polys * plan.ntt_size())
    pe = per(plan)
    if polys >= 3:
        a[:pe] = 0
        a[pe:2 * pe] = np.iinfo(plan.word_dtype).max
    a[(2 * pe if polys >= 3 else 0)::7] = 0
    return a


def poison(plan, words):
    return np.full(words * (2 if plan.WORD == 16 else 1), 0x5A5A5A5A5A5A5A5A & np.iinfo(plan.word_dtype).max, dtype=plan.word_dtype)


def subw(plan, a, b):
    """a - b mod 2^w on word arrays"""
    if plan.WORD != 16:
        with np.errstate(over="ignore"):
            return (a - b).astype(plan.word_dtype)
    lo = a[0::2] - b[0::2]
    out = np.empty_like(a)
    out[0::2] = lo
    out[1::2] = a[1::2] - b[1::2] - (a[0::2] < b[0::2]).astype(np.uint64)
    return out


# -- 1. one node -----------------------------------------------------------------------------------------------------------------------------
def run_cmux(torch, plan, where, c0, c1, kr, k, beta, ell, with_ws=False):
    """call 1 on word arrays (the selector as device residue planes) -> the output array, poisoned before"""
    n = plan.ntt_size()
    batch = c0.size // ((k + 1) * per(plan))
    out = poison(plan, batch * (k + 1) * n)
    nws = plan.glwe_cmux_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.glwe_cmux_batch(out, c0, c1, [host(p, plan.res_dtype).copy() for p in kr], k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.glwe_cmux_batch(out_t, dev(torch, c0), dev(torch, c1), kr, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def compose_cmux(torch, plan, c0, c1, kr, k, beta, ell):
    """The header's sequence of public calls: the copy of c0, the wrapping difference on the host, gadget_decompose_batch(plain) and
    external_product_batch(accumulate=True)."""
    out_t = dev(torch, c0.copy())
    d = dev(torch, subw(plan, c1, c0))
    terms = torch.zeros(d.numel() * ell, dtype=d.dtype, device="cuda")
    plan.gadget_decompose_batch(terms, d, beta, ell, mode="plain")
    plan.external_product_batch(out_t, terms, kr, (k + 1) * ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def gadgets(w):
    """(base_log, levels): base_log * levels = w; s > 0; and on the wider words a digit of more than 31 bits"""
    return [(w // 2, 2), (7, 3)] + ([(40, 1)] if w == 64 else [(45, 2)] if w == 128 else [])


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_cmux_equals_the_public_calls_for_every_kind(kind):
    """the smallest size of the kind, k = 0, 1, 2, batch 3, with and without a caller workspace; zeros, all-ones words and c1 == c0"""
    torch = _torch()
    plan = KINDS[kind].try_new(min_n(kind))
    n, pe = plan.ntt_size(), per(plan)
    rng = np.random.default_rng(seed("cmux", kind))
    for k in (0, 1, 2):
        for beta, ell in gadgets(wbits(plan)):
            assert (k + 1) * ell <= plan.max_terms()
            kr = selectors(torch, plan, rng, k, ell)
            c0, c1 = (words_with_zeros(rng, plan, 3 * (k + 1)) for _ in range(2))
            c1[2 * pe:2 * pe + pe // 2] = c0[2 * pe:2 * pe + pe // 2]         # equal words: a zero difference, all digits zero
            c1[-(k + 1) * pe:] = c0[-(k + 1) * pe:]                              # a whole ciphertext with c1 == c0
            want = compose_cmux(torch, plan, c0, c1, kr, k, beta, ell)
            for with_ws in (False, True):
                got = run_cmux(torch, plan, "device", c0, c1, kr, k, beta, ell, with_ws)
                assert got.any() and np.array_equal(got, want), (kind, n, k, beta, ell, with_ws, first_difference(got, want))


@pytest.mark.parametrize("kind,n,k", [("native64_plan32", 32, 1), ("native32_plan32", 32, 2), ("native64_plan32", 4096, 1), ("native32_plan32", 4096, 1),
                                      ("native64_plan32", 8192, 1), ("native32_plan32", 8192, 2), ("native64_plan52", 1024, 1)])
def test_cmux_size_classes(kind, n, k):
    """n = 32 and n = 4096, the last fused size; n = 8192 and the Plan52 kind: the composed external product"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("cmux-large", kind, n))
    beta, ell, batch = 7, 2, 2
    kr = selectors(torch, plan, rng, k, ell)
    c0, c1 = (words_with_zeros(rng, plan, batch * (k + 1)) for _ in range(2))
    want = compose_cmux(torch, plan, c0, c1, kr, k, beta, ell)
    for with_ws in (False, True):
        got = run_cmux(torch, plan, "device", c0, c1, kr, k, beta, ell, with_ws)
        assert got.any() and np.array_equal(got, want), (kind, n, with_ws, first_difference(got, want))


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32"])
def test_cmux_on_the_host_path(kind):
    torch = _torch()
    beta, ell, batch = 6, 3, 3
    plan = KINDS[kind].try_new(64)
    rng = np.random.default_rng(seed("cmux-host", kind))
    for k in (1, 0):
        kr = selectors(torch, plan, rng, k, ell)
        c0, c1 = (words_with_zeros(rng, plan, batch * (k + 1)) for _ in range(2))
        want = run_cmux(torch, plan, "device", c0, c1, kr, k, beta, ell)
        for with_ws in (True, False):
            got = run_cmux(torch, plan, "host", c0, c1, kr, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, want), (kind, k, with_ws, first_difference(got, want))


# -- 2. the tree -----------------------------------------------------------------------------------------------------------------------------
def run_tree(torch, plan, where, lut, kr, m, k, beta, ell, batch, with_ws=False):
    n = plan.ntt_size()
    out = poison(plan, batch * (k + 1) * n)
    nws = plan.cmux_tree_workspace_bytes(m, k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws and nws else None   # one entry needs none
        plan.cmux_tree_batch(out, lut, None if kr is None else [host(p, plan.res_dtype).copy() for p in kr], m, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.cmux_tree_batch(out_t, dev(torch, lut), kr, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def compose_leaf(torch, plan, f0, f1, sel, k, beta, ell):
    """stage 1 as the header defines it, from public calls: zero masks, the body f0, the `levels` digit polynomials of f1 - f0, and
    external_product_batch(nterms = levels, accumulate=True) against the selector's body rows.  f0, f1: (count, per) word arrays."""
    n, pe = plan.ntt_size(), per(plan)
    count = f0.shape[0]
    out = np.zeros((count, k + 1, pe), dtype=plan.word_dtype)
    out[:, k] = f0
    out_t = dev(torch, out.reshape(-1))
    d = dev(torch, subw(plan, f1.reshape(-1), f0.reshape(-1)))
    terms = torch.zeros(count * ell * pe, dtype=d.dtype, device="cuda")
    plan.gadget_decompose_batch(terms, d, beta, ell, mode="plain")
    plan.external_product_batch(out_t, terms, [p[k * ell * (k + 1) * n:] for p in sel], ell, k + 1, accumulate=True)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def compose_tree(torch, plan, lut, kr, m, k, beta, ell, batch):
    """the header's sequence: the leaf stage from public calls, then one glwe_cmux_batch per stage on the batch * h pairs of that stage"""
    pe = per(plan)
    if m == 1:
        out = np.zeros((batch, k + 1, pe), dtype=plan.word_dtype)
        out[:, k] = lut.reshape(batch, pe)
        return out.reshape(-1)
    cur = lut.reshape(batch, m, pe)
    for s, (h, i) in enumerate(stage_params(m), 1):
        sel = selector(plan, kr, i, k, ell)
        lo, hi = np.ascontiguousarray(cur[:, :h]), np.ascontiguousarray(cur[:, h:])
        if s == 1:
            cur = compose_leaf(torch, plan, lo.reshape(batch * h, pe), hi.reshape(batch * h, pe), sel, k, beta, ell)
        else:
            cur = run_cmux(torch, plan, "device", lo.reshape(-1), hi.reshape(-1), sel, k, beta, ell)
        cur = cur.reshape(batch, h, (k + 1) * pe)
    return cur.reshape(-1)


@pytest.mark.parametrize("kind,n,k,batch", [("native64_plan32", 32, 1, 1), ("native32_plan32", 32, 2, 3), ("native128_plan32", 32, 0, 3),
                                            ("native_binary64_plan32", 32, 1, 3), ("native64_plan32", 32, 0, 1), ("native32_plan32", 32, 1, 3),
                                            ("native64_plan32", 32, 2, 3), ("native64_plan32", 1024, 1, 3)])
def test_tree_equals_the_leaf_stage_and_one_cmux_per_stage(kind, n, k, batch):
    """n = 32 with M in {1, 2, 4, 8}, the case at n = 1024 with M = 8; both workspace modes; the host path at M = 1 and 4"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("tree", kind, n, k))
    beta, ell = 5, 2
    for m in (1, 2, 4, 8) if n == 32 else (8,):
        depth = m.bit_length() - 1
        kr = selectors(torch, plan, rng, k, ell, depth) if depth else None
        lut = words_with_zeros(rng, plan, batch * m)
        want = compose_tree(torch, plan, lut, kr, m, k, beta, ell, batch)
        for with_ws in (False, True):
            got = run_tree(torch, plan, "device", lut, kr, m, k, beta, ell, batch, with_ws)
            assert got.any() and np.array_equal(got, want), (kind, n, k, m, with_ws, first_difference(got, want))
        if n == 32 and m in (1, 4):
            assert np.array_equal(run_tree(torch, plan, "host", lut, kr, m, k, beta, ell, batch, with_ws=True), want), (kind, k, m, "host")
            assert np.array_equal(run_tree(torch, plan, "host", lut, kr, m, k, beta, ell, batch, with_ws=False), want), (kind, k, m, "host, no workspace")


@pytest.mark.parametrize("kind,k", [("native64_plan32", 1), ("native32_plan32", 2), ("native128_plan32", 0), ("native_binary32_plan52", 1)])
def test_leaf_stage_equals_cmux_on_trivial_ciphertexts(kind, k):
    """M = 2 is the leaf stage alone.  It has the words of glwe_cmux_batch on host-built trivial ciphertexts, whose zero masks call 1
    does decompose: the torus arithmetic is exact, for every kind."""
    torch = _torch()
    for n in (min_n(kind), 1024):
        plan = KINDS[kind].try_new(n)
        pe = per(plan)
        rng = np.random.default_rng(seed("leaf", kind, k, n))
        beta, ell, batch = 6, 2, 3
        kr = selectors(torch, plan, rng, k, ell)
        lut = words_with_zeros(rng, plan, batch * 2)
        triv = np.zeros((batch, 2, k + 1, pe), dtype=plan.word_dtype)
        triv[:, :, k] = lut.reshape(batch, 2, pe)
        want = run_cmux(torch, plan, "device", np.ascontiguousarray(triv[:, 0]).reshape(-1), np.ascontiguousarray(triv[:, 1]).reshape(-1), kr, k, beta, ell)
        got = run_tree(torch, plan, "device", lut, kr, 2, k, beta, ell, batch, with_ws=True)
        assert got.any() and np.array_equal(got, want), (kind, k, n, first_difference(got, want))


# -- 3. a second, ragged trip of the walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["native64_plan32", "native32_plan32"])
def test_walk_makes_a_second_trip_with_a_ragged_tail(kind):
    """the grid rule caps the workgroups; cap / (k + 1) + 3 output ciphertexts leave 3 (k + 1) polynomials for a second trip that most
    workgroups do not make -- in call 1 and in the leaf stage of a tree with M = 2"""
    torch = _torch()
    n, k, beta, ell = 32, 1, 5, 2
    plan = KINDS[kind].try_new(n)
    cap = cntt.lib().cntt_native_cmux_grid(1 << 30, 5, plan.WORD)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_native_cmux_grid(batch * (k + 1), 5, plan.WORD) == cap < batch * (k + 1) < 2 * cap
    rng = np.random.default_rng(seed("cmux-ragged", kind))
    kr = selectors(torch, plan, rng, k, ell)
    c0, c1 = (random_words(rng, plan, batch * (k + 1) * n) for _ in range(2))
    got = run_cmux(torch, plan, "device", c0, c1, kr, k, beta, ell)
    want = compose_cmux(torch, plan, c0, c1, kr, k, beta, ell)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], c0[tail]) and not np.array_equal(got[tail], poison(plan, 3 * (k + 1) * n))
    lut = random_words(rng, plan, batch * 2 * n)
    got = run_tree(torch, plan, "device", lut, kr, 2, k, beta, ell, batch)
    want = compose_tree(torch, plan, lut, kr, 2, k, beta, ell, batch)
    assert np.array_equal(got, want), first_difference(got, want)
    triv = np.zeros((3, k + 1, n), dtype=plan.word_dtype)
    triv[:, k] = lut.reshape(batch, 2, n)[-3:, 0]
    assert got[tail].any() and not np.array_equal(got[tail], triv.reshape(-1)) and not np.array_equal(got[tail], poison(plan, 3 * (k + 1) * n))


# -- 4. graph capture ------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_the_tree_with_a_caller_workspace():
    """native64 Plan32, n = 1024, M = 16: captured once, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    n, k, beta, ell, batch, m = 1024, 1, 8, 3, 2, 16
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(25)
    kr = selectors(torch, plan, rng, k, ell, 4)
    lut = dev(torch, random_words(rng, plan, batch * m * n))
    ws = torch.zeros(plan.cmux_tree_workspace_bytes(m, k, ell, batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(plan, batch * (k + 1) * n))
    plan.cmux_tree_batch(out, lut, kr, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.cmux_tree_batch(out, lut, kr, m, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, plan, batch * m * n))
        eager = torch.zeros_like(out)
        plan.cmux_tree_batch(eager, fresh, kr, m, k, beta, ell)
        lut.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 5. the STREAM form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,beta", [("native64_plan32", 4), ("native32_plan32", 2)])
def test_cmux_and_leaf_stage_of_a_streaming_batch(kind, beta):
    """native_cmux_diff_kernel<W, true, LEAF>: the first batch whose digits pass STREAM_BYTES (host_native_cmux.inc compares
    nct * (k + 1) * levels * n * word for ciphertext sources and nct * levels * n * word for table leaves), at n = 1024, k = 1 and 15
    levels, with a caller workspace of exactly the workspace formula.  Every word against the call over two halves of the batch, which
    do not stream; the first and the last element against the public calls."""
    torch = _torch()
    n, k, ell = 1024, 1, 15
    plan = KINDS[kind].try_new(n)
    w = plan.WORD
    rng = np.random.default_rng(seed("cmux-stream", kind))
    kr = selectors(torch, plan, rng, k, ell)
    tt, lo_, hi_ = (torch.int32, -2 ** 31, 2 ** 31 - 1) if w == 4 else (torch.int64, -2 ** 63, 2 ** 63 - 1)
    gen = torch.Generator(device="cuda").manual_seed(seed("cmux-stream", kind))
    for leaf in (False, True):
        unit = (1 if leaf else k + 1) * ell * n * w
        batch = STREAM_BYTES // unit + 1
        assert batch * unit > STREAM_BYTES >= (batch - 1) * unit and (batch - batch // 2) * unit <= STREAM_BYTES
        per_in, per_out = (2 * n if leaf else (k + 1) * n), (k + 1) * n
        a = torch.randint(lo_, hi_, (batch * per_in,), dtype=tt, device="cuda", generator=gen)
        b = None if leaf else torch.randint(lo_, hi_, (batch * per_in,), dtype=tt, device="cuda", generator=gen)
        out = torch.full((batch * per_out,), 0x5A5A5A5A, dtype=tt, device="cuda")
        nws = plan.cmux_tree_workspace_bytes(2, k, ell, batch) if leaf else plan.glwe_cmux_workspace_bytes(k, ell, batch)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda")

        def call(dst, lo, hi, workspace=None):
            if leaf:
                plan.cmux_tree_batch(dst, a[lo * per_in:hi * per_in], kr, 2, k, beta, ell, workspace=workspace)
            else:
                plan.glwe_cmux_batch(dst, a[lo * per_in:hi * per_in], b[lo * per_in:hi * per_in], kr, k, beta, ell, workspace=workspace)

        call(out, 0, batch, ws)
        half = batch // 2
        small = torch.empty((batch - half) * per_out, dtype=tt, device="cuda")
        for lo, hi in ((0, half), (half, batch)):
            part = small[:(hi - lo) * per_out]
            part.fill_(0x5A5A5A5A)
            call(part, lo, hi)
            assert torch.equal(part, out[lo * per_out:hi * per_out]), (kind, leaf, lo, hi)
        for e in (0, batch - 1):
            got = host(out[e * per_out:(e + 1) * per_out], plan.word_dtype)
            src = host(a[e * per_in:(e + 1) * per_in], plan.word_dtype)
            if leaf:
                want = compose_leaf(torch, plan, src[None, :n], src[None, n:], kr, k, beta, ell)
            else:
                want = compose_cmux(torch, plan, src, host(b[e * per_in:(e + 1) * per_in], plan.word_dtype), kr, k, beta, ell)
            assert got.any() and np.array_equal(got, want), (kind, leaf, e, first_difference(got, want))
        del a, b, out, ws, small
        gc.collect()
        torch.cuda.empty_cache()


# -- 6. an encrypted table lookup ------------------------------------------------------------------------------------------------------------
def noisy_ggsw(rng, S_mat, bit, n, beta, ell):
    """GGSW(bit) under the binary key S (k = 1) mod 2^64, coefficient domain: row (q, l) = (A, A (*) S + e) with |e| < 2^10 and
    bit * 2^(64 - beta l) added to polynomial q"""
    rows = 2 * ell
    A = rng.integers(0, 2 ** 64, size=(rows, n), dtype=np.uint64).astype(object)
    body = times_binary(A, S_mat) + rng.integers(-2 ** 10 + 1, 2 ** 10, size=(rows, n)).astype(object)
    for q in range(2):
        for l in range(1, ell + 1):
            (A if q == 0 else body)[q * ell + l - 1, 0] += bit << (64 - beta * l)
    return np.stack([(A % 2 ** 64).astype(np.uint64), (body % 2 ** 64).astype(np.uint64)], axis=1).reshape(-1)


def test_every_address_of_an_encrypted_lookup_decodes():
    """native64 Plan32, n = 64, k = 1, binary key, base_log 16, levels 4 (base_log * levels = 64: no rounding): a random table of
    M * n = 4 * 64 3-bit entries at steps of 2^61, log2 M + log2 n = 8 address bits as noisy GGSWs (|e| < 2^10).  cmux_tree_batch over
    the top 2 bits, blind_rotate_batch with rot_t[i] = 2n - 2^i over the low 6, sample_extract_batch(index 0): EVERY one of the 256
    addresses decodes to its entry.
    Error bound: the table is noise-free.  A CMux adds sum over its (k + 1) levels term polynomials of digit (*) row noise, each
    coefficient a sum of n products of a digit (at most B / 2 = 2^15 in size) and a noise word (below 2^10): at most
    (k + 1) n levels (B / 2) 2^10 = 2 * 2^6 * 2^2 * 2^15 * 2^10 = 2^34, and it passes on the noise of the input it selects, exactly,
    because nothing is rounded.  The log2 M = 2 tree stages and the log2 n = 6 rotations are one CMux each.  So the error is below
    (log2 M + log2 n) * 2^34 = 2^37, asserted; half a message step is 2^60."""
    torch = _torch()
    n, k, beta, ell, m = 64, 1, 16, 4, 4
    logn, depth = 6, 2
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(seed("native-cmux-lookup", m))
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    # GGSW(0) and GGSW(1) of every address bit as residue planes: bit i of the address uses G[i][its value]
    G = [[key_planes(torch, plan, noisy_ggsw(rng, NS, bit, n, beta, ell)) for bit in (0, 1)] for _ in range(logn + depth)]
    entries = rng.integers(0, 8, size=(m, n))
    table = dev(torch, (entries.astype(np.uint64) << np.uint64(61)).reshape(-1))
    rot_t = dev(torch, np.array([2 * n - (1 << i) for i in range(logn)] + [0], dtype=np.uint32))
    accs = torch.zeros(m * n * (k + 1) * n, dtype=torch.int64, device="cuda")
    ws_tree = torch.zeros(plan.cmux_tree_workspace_bytes(m, k, ell, 1), dtype=torch.uint8, device="cuda")
    ws_rot = torch.zeros(plan.pbs_workspace_bytes(logn, k, ell, 1), dtype=torch.uint8, device="cuda")
    glwe = torch.zeros((k + 1) * n, dtype=torch.int64, device="cuda")

    def planes(bits, first):
        return [torch.cat([G[first + i][b][j] for i, b in enumerate(bits)]) for j in range(plan.NPRIMES)]

    low = [planes([(a >> i) & 1 for i in range(logn)], 0) for a in range(n)]
    for hi in range(m):
        plan.cmux_tree_batch(glwe, table, planes([(hi >> i) & 1 for i in range(depth)], logn), m, k, beta, ell, workspace=ws_tree)
        for lo in range(n):
            a = hi * n + lo
            plan.blind_rotate_batch(accs[a * (k + 1) * n:(a + 1) * (k + 1) * n], glwe, rot_t, low[lo], logn, k, beta, ell, workspace=ws_rot,
                                    lut_per_element=True)
    lwe = torch.zeros(m * n * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.sample_extract_batch(lwe, accs, k, 0)
    torch.cuda.synchronize()
    rows = host(lwe, np.uint64).reshape(m * n, n + 1)
    with np.errstate(over="ignore"):
        phase = rows[:, n] - (rows[:, :n] * S.astype(np.uint64)).sum(axis=1, dtype=np.uint64)          # uint64 arithmetic wraps: mod 2^64
    dec = [int(((int(x) >> 60) + 1) >> 1) & 7 for x in phase]
    want = entries.reshape(-1).tolist()
    assert len(set(want)) == 8 and dec == want, [i for i, (x, y) in enumerate(zip(dec, want)) if x != y][:8]
    err = [(int(x) - (y << 61)) % 2 ** 64 for x, y in zip(phase, want)]
    worst = max(min(e, 2 ** 64 - e) for e in err)
    bound = (depth + logn) * (k + 1) * n * ell * (1 << (beta - 1)) * (1 << 10)
    assert bound == 1 << 37
    print("lookup M = %d: worst error 2^%.2f over %d addresses, derived bound 2^37" % (m, np.log2(max(worst, 1)), m * n))
    assert worst < bound


# -- 7. the C example ------------------------------------------------------------------------------------------------------------------------
def test_lookup_native_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "lookup_native"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "lookup_native")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "every looked-up entry decoded" in r.stdout, r.stdout
