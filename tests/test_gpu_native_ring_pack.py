"""Ring packing of LWE ciphertexts through automorphisms on the native plans (include/cntt_ring_pack.h) on the MI355X.  Bit-exact
throughout, no tolerance anywhere but in the one decoding test: the embedding against the plain-int model and through
sample_extract_batch(index = 0) back to its input; a merge node against the sequence of public calls the header defines it by, for the
five non-binary kinds, at the staging edge of each word type under both settings of the "autom_lds" switch, on the host path and on a
stream; the pack against embed + merges + trace; the LWE-leaf stage against embedding then merging; a second grid trip; graph capture; the
closed form on noise-free keys; encrypted messages under noisy keys, whose derived noise bound stands in the test's docstring; the C
example.

The plans start at n = 32 (30-bit residue primes) and n = 16 (50-bit ones), so those are the smallest shapes any call here can see."""
import os
import random
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_automorphism_model import autom_gather, phase, trace_exponents, trace_keys
from native_ring_pack_model import decode, embed, encode, lwe_phase, stages
from test_gpu_native_automorphism import NON_BINARY, addw, ak_planes, min_n, negw, poison, run_trace, sigma
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, per, random_words, seed, to_array, to_ints, wbits
from test_gpu_prime_pack import first_difference, negacyclic_matrix, times_binary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORD_KINDS = ["native32_plan32", "native64_plan32", "native128_plan32"]


def cw(plan):
    """array elements per word"""
    return 2 if plan.WORD == 16 else 1


def row_len(plan, k):
    """array elements of one LWE row"""
    return (k * plan.ntt_size() + 1) * cw(plan)


def rot_np(plan, a, shift):
    """X^shift on a word array of whole polynomials, numpy: the gather form of CNTT_SRC_ROTATE"""
    n = plan.ntt_size()
    r = (np.arange(n, dtype=np.int64) - shift) % (2 * n)
    x = np.ascontiguousarray(a.reshape(-1, n, cw(plan))[:, r % n, :])
    neg = negw(plan, x.reshape(-1)).reshape(x.shape)
    return np.where((r >= n)[None, :, None], neg, x).reshape(-1)


def quarters(plan, a):
    """the first quarter of the first polynomial 0, the second quarter all-ones words"""
    pe = per(plan)
    a[:pe // 4] = 0
    a[pe // 4:pe // 2] = np.iinfo(plan.word_dtype).max
    return a


def key_slice(kr, r, per_key):
    return [p[r * per_key:(r + 1) * per_key] for p in kr]


# -- 1. the embedding ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["native32_plan52", "native64_plan52", "native32_plan32", "native64_plan32", "native128_plan32", "native_binary64_plan32"])
def test_embed_matches_the_model_and_inverts_sample_extraction(kind):
    """the three word types and one binary kind at their smallest size, k = 0, 1, 2, batch 3, device and host path"""
    torch = _torch()
    plan = KINDS[kind].try_new(min_n(kind))
    n, w, batch = plan.ntt_size(), wbits(plan), 3
    rng = np.random.default_rng(seed("ring-embed", kind))
    for k in (0, 1, 2):
        rl = row_len(plan, k)
        lwe = random_words(rng, plan, batch * (k * n + 1))
        lwe[:rl // 4] = 0
        lwe[rl // 4:rl // 2] = np.iinfo(plan.word_dtype).max
        want = to_array(plan, [v for b in range(batch) for v in embed(to_ints(plan, lwe[b * rl:(b + 1) * rl]), w, k, n)])
        out_t = dev(torch, poison(plan, batch * (k + 1) * n))
        plan.glwe_embed_batch(out_t, dev(torch, lwe), k)
        torch.cuda.synchronize()
        got = host(out_t, plan.word_dtype)
        assert np.array_equal(got, want), (kind, k, first_difference(got, want))
        out_h = poison(plan, batch * (k + 1) * n)
        plan.glwe_embed_batch(out_h, lwe, k)
        assert np.array_equal(out_h, want), (kind, k, "host")
        back = dev(torch, poison(plan, batch * (k * n + 1)))
        plan.sample_extract_batch(back, out_t, k, 0)
        torch.cuda.synchronize()
        assert np.array_equal(host(back, plan.word_dtype), lwe), (kind, k, "sample_extract")


# -- 2. one merge node ---------------------------------------------------------------------------------------------------------------------
def run_merge(torch, plan, where, even, odd, kr, shift, t, k, beta, ell, with_ws=False, stream=None):
    n = plan.ntt_size()
    batch = even.size // ((k + 1) * per(plan))
    out = poison(plan, batch * (k + 1) * n)
    nws = plan.glwe_merge_workspace_bytes(k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws and nws else None
        plan.glwe_merge_batch(out, even, odd, [host(p, plan.res_dtype).copy() for p in kr] if k else None, shift, t, k, beta, ell, workspace=ws)
        return out
    out_t, e_t, o_t = dev(torch, out), dev(torch, even), dev(torch, odd)
    ws = torch.zeros(max(nws, 16), dtype=torch.uint8, device="cuda") if with_ws else None
    if stream is None:
        plan.glwe_merge_batch(out_t, e_t, o_t, kr if k else None, shift, t, k, beta, ell, workspace=ws)
    else:
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            plan.glwe_merge_batch(out_t, e_t, o_t, kr if k else None, shift, t, k, beta, ell, workspace=ws)
        stream.synchronize()
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def compose_merge(torch, plan, even, odd, kr, shift, t, k, beta, ell):
    """The header's sequence of public calls: rotate / add / subtract and the prefill on the host in numpy, automorphism_batch on the k
    mask polynomials of d, gadget_decompose_batch(plain), every digit negated mod 2^w, external_product_batch(accumulate=True)."""
    pe = per(plan)
    batch = even.size // ((k + 1) * pe)
    ro = rot_np(plan, odd, shift)
    a = addw(plan, even, ro).reshape(batch, k + 1, pe)
    d = addw(plan, even, negw(plan, ro)).reshape(batch, k + 1, pe)
    out = a.copy()
    out[:, k] = addw(plan, np.ascontiguousarray(a[:, k]).reshape(-1), sigma(plan, np.ascontiguousarray(d[:, k]).reshape(-1), t)).reshape(batch, pe)
    out_t = dev(torch, out.reshape(-1))
    if k:
        masks = dev(torch, np.ascontiguousarray(d[:, :k]).reshape(-1))
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


@pytest.mark.parametrize("kind", NON_BINARY)
def test_merge_equals_the_public_calls_for_every_kind(kind):
    """the smallest size of the kind, k = 0, 1, 2, batch 3, shift in {0, 1, n - 1, n, 2n - 1}, t in {3, n + 1, 2n - 1}, full-word and
    rounded digits, with a caller workspace and with NULL"""
    torch = _torch()
    plan = KINDS[kind].try_new(min_n(kind))
    n, w, batch = plan.ntt_size(), wbits(plan), 3
    rng = np.random.default_rng(seed("ring-merge", kind))
    for k in (0, 1, 2):
        for beta, ell in ((w // 4, 4), (7, 3)):
            kr = ak_planes(torch, plan, rng, k, ell)
            even = quarters(plan, random_words(rng, plan, batch * (k + 1) * n))
            odd = quarters(plan, random_words(rng, plan, batch * (k + 1) * n))
            for i, shift in enumerate((0, 1, n - 1, n, 2 * n - 1)):
                for t in (3, n + 1, 2 * n - 1):
                    want = compose_merge(torch, plan, even, odd, kr, shift, t, k, beta, ell)
                    got = run_merge(torch, plan, "device", even, odd, kr, shift, t, k, beta, ell, with_ws=bool(i % 2))
                    assert got.any() and np.array_equal(got, want), (kind, k, beta, ell, shift, t, first_difference(got, want))


@pytest.mark.parametrize("kind,n", [("native128_plan32", 2048), ("native128_plan32", 4096), ("native64_plan32", 4096), ("native64_plan32", 8192),
                                    ("native32_plan32", 8192), ("native32_plan32", 16384)])
def test_merge_at_the_staging_edge(kind, n):
    """the last size of each word type whose two source polynomials are staged through LDS (64 KiB together) and the first that is
    not: k = 1, one level, batch 1; both settings of the switch give identical words, those of the public calls"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("ring-edge", kind, n))
    k, beta, ell = 1, 9, 1
    kr = ak_planes(torch, plan, rng, k, ell)
    even, odd = random_words(rng, plan, (k + 1) * n), random_words(rng, plan, (k + 1) * n)
    shift, t = int(rng.integers(2 * n)), 2 * int(rng.integers(n)) + 1
    got = []
    for lds in (1, 0):
        with cntt.debug_switches(autom_lds=lds):
            got.append(run_merge(torch, plan, "device", even, odd, kr, shift, t, k, beta, ell, with_ws=True))
    assert got[0].any() and np.array_equal(got[0], got[1]), (kind, n, first_difference(got[0], got[1]))
    want = compose_merge(torch, plan, even, odd, kr, shift, t, k, beta, ell)
    assert np.array_equal(got[0], want), (kind, n, first_difference(got[0], want))


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32"])
def test_merge_on_the_host_path_and_on_a_stream(kind):
    torch = _torch()
    beta, ell, batch, n = 6, 3, 3, 64
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("ring-merge-host", kind))
    for k in (1, 0):
        kr = ak_planes(torch, plan, rng, k, ell)
        even, odd = random_words(rng, plan, batch * (k + 1) * n), random_words(rng, plan, batch * (k + 1) * n)
        want = compose_merge(torch, plan, even, odd, kr, 5, n + 1, k, beta, ell)
        for with_ws in (True, False):
            got = run_merge(torch, plan, "host", even, odd, kr, 5, n + 1, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, want), (kind, k, with_ws, first_difference(got, want))
    k = 1
    kr = ak_planes(torch, plan, rng, k, ell)
    even, odd = random_words(rng, plan, batch * (k + 1) * n), random_words(rng, plan, batch * (k + 1) * n)
    want = compose_merge(torch, plan, even, odd, kr, n + 3, 5, k, beta, ell)
    got = run_merge(torch, plan, "device", even, odd, kr, n + 3, 5, k, beta, ell, True, stream=torch.cuda.Stream())
    assert got.any() and np.array_equal(got, want), (kind, "stream", first_difference(got, want))


# -- 3. the pack ---------------------------------------------------------------------------------------------------------------------------
def run_pack(torch, plan, where, lwe, kr, m, k, beta, ell, with_ws):
    n = plan.ntt_size()
    batch = lwe.size // (m * row_len(plan, k))
    out = poison(plan, batch * (k + 1) * n)
    nws = plan.ring_pack_workspace_bytes(m, k, ell, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.ring_pack_batch(out, lwe, [host(p, plan.res_dtype).copy() for p in kr] if k else None, m, k, beta, ell, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.ring_pack_batch(out_t, dev(torch, lwe), kr if k else None, m, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def embed_rows(torch, plan, lwe, k):
    rows = lwe.size // row_len(plan, k)
    out_t = dev(torch, poison(plan, rows * (k + 1) * plan.ntt_size()))
    plan.glwe_embed_batch(out_t, dev(torch, lwe), k)
    torch.cuda.synchronize()
    return host(out_t, plan.word_dtype)


def sequence_pack(torch, plan, lwe, kr, m, k, beta, ell):
    """call 1 on all rows, call 2 once per stage on the batch * h pairs of that stage, then glwe_trace_batch"""
    n, ct = plan.ntt_size(), (k + 1) * per(plan)
    batch = lwe.size // (m * row_len(plan, k))
    per_key = k * ell * (k + 1) * n
    cur = embed_rows(torch, plan, lwe, k).reshape(batch, m, ct)
    tree, steps = stages(n, m)
    for _, h, shift, t, r in tree:
        even, odd = np.ascontiguousarray(cur[:, :h]).reshape(-1), np.ascontiguousarray(cur[:, h:2 * h]).reshape(-1)
        cur = run_merge(torch, plan, "device", even, odd, key_slice(kr, r, per_key), shift, t, k, beta, ell).reshape(batch, h, ct)
    return run_trace(torch, plan, cur.reshape(-1), kr, steps, k, beta, ell, True)


@pytest.mark.parametrize("kind,n,k,batch", [("native64_plan52", 16, 1, 1), ("native32_plan52", 16, 1, 1), ("native64_plan32", 32, 2, 3),
                                            ("native128_plan32", 32, 2, 3), ("native32_plan32", 32, 0, 2)])
def test_pack_equals_embed_merges_and_trace(kind, n, k, batch):
    """M in {1, 2, n / 2, n}: the embed-only path, the leaf-only stage, the trace after a tree and the last merge writing glwe_out, and
    both parities of the buffers; with a caller workspace and with NULL, and the host path once"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    logn, beta, ell = n.bit_length() - 1, 6, 2
    rng = np.random.default_rng(seed("ring-pack", kind, n, k))
    kr = ak_planes(torch, plan, rng, k, ell, logn)
    for m in (1, 2, n // 2, n):
        lwe = random_words(rng, plan, batch * m * (k * n + 1))
        lwe[:row_len(plan, k) // 4] = 0
        want = sequence_pack(torch, plan, lwe, kr, m, k, beta, ell)
        for with_ws in (True, False):
            got = run_pack(torch, plan, "device", lwe, kr, m, k, beta, ell, with_ws)
            assert got.any() and np.array_equal(got, want), (kind, n, k, m, with_ws, first_difference(got, want))
        if m in (2, n):
            got = run_pack(torch, plan, "host", lwe, kr, m, k, beta, ell, m == 2)
            assert np.array_equal(got, want), (kind, n, k, m, "host", first_difference(got, want))


@pytest.mark.parametrize("kind", WORD_KINDS)
def test_leaf_stage_equals_embedding_then_merging(kind):
    """M = 2: the pack's first stage reads the LWE rows through the embed rule; its words are those of the PUBLIC merge on the embedded
    ciphertexts followed by the trace -- the leaf form of the kernel against its ciphertext form.  Rows of k n + 1 words start at odd
    word offsets: batch 3, k = 1, both settings of the switch."""
    torch = _torch()
    n, k, beta, ell, batch, m = 64, 1, 8, 2, 3, 2
    plan = KINDS[kind].try_new(n)
    logn = n.bit_length() - 1
    rng = np.random.default_rng(seed("ring-leaf", kind))
    kr = ak_planes(torch, plan, rng, k, ell, logn)
    per_key = k * ell * (k + 1) * n
    lwe = random_words(rng, plan, batch * m * (k * n + 1))
    emb = embed_rows(torch, plan, lwe, k).reshape(batch, m, (k + 1) * per(plan))
    merged = run_merge(torch, plan, "device", np.ascontiguousarray(emb[:, 0]).reshape(-1), np.ascontiguousarray(emb[:, 1]).reshape(-1),
                       key_slice(kr, logn - 1, per_key), n // 2, 3, k, beta, ell)
    want = run_trace(torch, plan, merged, kr, logn - 1, k, beta, ell, True)
    for lds in (1, 0):
        with cntt.debug_switches(autom_lds=lds):
            got = run_pack(torch, plan, "device", lwe, kr, m, k, beta, ell, True)
        assert got.any() and np.array_equal(got, want), (kind, lds, first_difference(got, want))


@pytest.mark.parametrize("kind,n", [("native64_plan32", 32), ("native32_plan32", 64)])
def test_merge_and_embed_make_a_second_grid_trip(kind, n):
    """more output polynomials than cntt_native_ring_pack_grid returns, with a ragged tail"""
    torch = _torch()
    k, beta, ell = 1, 5, 2
    plan = KINDS[kind].try_new(n)
    logn = n.bit_length() - 1
    cap = cntt.lib().cntt_native_ring_pack_grid(1 << 30, logn, plan.WORD)
    batch = cap // (k + 1) + 3
    assert cntt.lib().cntt_native_ring_pack_grid(batch * (k + 1), logn, plan.WORD) == cap < batch * (k + 1) < 2 * cap
    rng = np.random.default_rng(seed("ring-ragged", kind))
    kr = ak_planes(torch, plan, rng, k, ell)
    even, odd = random_words(rng, plan, batch * (k + 1) * n), random_words(rng, plan, batch * (k + 1) * n)
    got = run_merge(torch, plan, "device", even, odd, kr, n + 1, 2 * n - 1, k, beta, ell)
    want = compose_merge(torch, plan, even, odd, kr, n + 1, 2 * n - 1, k, beta, ell)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * (k + 1) * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], poison(plan, 3 * (k + 1) * n))
    lwe = random_words(rng, plan, batch * (k * n + 1))
    emb = embed_rows(torch, plan, lwe, k)
    back = dev(torch, poison(plan, batch * (k * n + 1)))
    plan.sample_extract_batch(back, dev(torch, emb), k, 0)
    torch.cuda.synchronize()
    assert np.array_equal(host(back, plan.word_dtype), lwe)


def test_graph_capture_of_the_pack_with_a_caller_workspace():
    """native64 Plan32, n = 1024, k = 1, M = 8: three stages and seven trace rounds captured once as a linear chain and replayed twice
    on fresh inputs"""
    torch = _torch()
    n, k, beta, ell, batch, m = 1024, 1, 8, 3, 2, 8
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(28)
    kr = ak_planes(torch, plan, rng, k, ell, 10)
    lwe = dev(torch, random_words(rng, plan, batch * m * (k * n + 1)))
    ws = torch.zeros(plan.ring_pack_workspace_bytes(m, k, ell, batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(plan, batch * (k + 1) * n))
    plan.ring_pack_batch(out, lwe, kr, m, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.ring_pack_batch(out, lwe, kr, m, k, beta, ell, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, plan, batch * m * (k * n + 1)))
        eager = torch.zeros_like(out)
        plan.ring_pack_batch(eager, fresh, kr, m, k, beta, ell)
        lwe.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


# -- 4. what the pack means ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,n", [(64, 32), (32, 32), (128, 32)])
def test_pack_on_noise_free_keys_is_the_closed_form(w, n):
    """base_log * levels = w, k = 1, binary key: coefficient j n / M of the phase is n * phase_j mod 2^w and every other coefficient 0"""
    torch = _torch()
    plan = KINDS["native%d_plan32" % w].try_new(n)
    logn, k, beta, ell = n.bit_length() - 1, 1, w // 4, 4
    rnd = random.Random("native-ring-closed/%d" % w)
    S = [[rnd.randrange(2) for _ in range(n)]]
    kr = key_planes(torch, plan, to_array(plan, trace_keys(rnd, w, S, logn, n, beta, ell)))
    for m in (1, 2, 4, n):
        rows = [[rnd.randrange(1 << w) for _ in range(k * n + 1)] for _ in range(m)]
        got = run_pack(torch, plan, "device", to_array(plan, [v for row in rows for v in row]), kr, m, k, beta, ell, True)
        want = [0] * n
        for j, row in enumerate(rows):
            want[j * n // m] = n * lwe_phase(row, S, w) % (1 << w)
        assert phase(to_ints(plan, got), S, w) == want, (w, n, m)


def test_pack_decodes_every_message_under_noisy_keys():
    """native64 Plan32, n = 1024, k = 1, M = 16, binary key, base_log 16, levels 4 (base_log * levels = w: no rounding).  Sixteen LWE
    ciphertexts carry the 3-bit messages j mod 8 at bit 64 - 10 - 3 = 51 -- ten bits of headroom below the message, as the header asks --
    with encryption noise below E0 = 2^10; the ten trace keys have noise below E = 2^10 per coefficient.  After the pack coefficient
    j n / M = 64 j of the phase is 2^10 (2^51 m_j + e_j) + error = 2^61 m_j + error, decoded from the top three bits, correct for EVERY
    message, and every other coefficient holds error only.
    Error bound, derived from the header's growth rule.  The input noise grows by n: at most n E0 = 2^20.  One keyswitch (a stage or a
    trace round alike: k * levels term polynomials, each coefficient a sum of n products of a digit of size at most B / 2 = 2^15 and a
    noise word below E) adds at most KS = k levels n (B / 2) E = 4 * 2^10 * 2^15 * 2^10 = 2^37, and the noise of step i of the
    log2 n = 10 steps grows by 2^(9 - i): together at most n E0 + (2^10 - 1) KS < 2^20 + 2^47, asserted below half a message step,
    2^60, before the GPU call.  The measured worst error is printed next to the bound."""
    torch = _torch()
    n, k, beta, ell, w, m, bits = 1024, 1, 16, 4, 64, 16, 3
    logn = 10
    E0 = E = 1 << 10
    bound = n * E0 + ((1 << logn) - 1) * k * ell * n * (1 << (beta - 1)) * E
    assert bound == (1 << 20) + 1023 * (1 << 37) and bound < 1 << (w - bits - 1)
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(seed("native-ring-noisy"))
    S = rng.integers(0, 2, size=n).astype(np.int64)
    NS = negacyclic_matrix(S)
    key = []
    for t in trace_exponents(n, logn):
        rot = np.array(autom_gather([int(s) for s in S], t, w), dtype=object)          # sigma_t(S) mod 2^64: words 0, 1 and 2^64 - 1
        A = rng.integers(0, 2 ** 64, size=(ell, n), dtype=np.uint64).astype(object)
        body = times_binary(A, NS) + rng.integers(-E + 1, E, size=(ell, n)).astype(object)
        for l in range(1, ell + 1):
            body[l - 1] += rot * (1 << (w - beta * l))
        key.append(np.stack([(A % 2 ** 64).astype(np.uint64), (body % 2 ** 64).astype(np.uint64)], axis=1).reshape(-1))
    kr = key_planes(torch, plan, np.concatenate(key))
    msgs = [j % 8 for j in range(m)]
    a = rng.integers(0, 2 ** 64, size=(m, n), dtype=np.uint64)
    b = (a.astype(object) * S.astype(object)).sum(axis=1) + np.array([encode(x, bits, w, n) for x in msgs], dtype=object) \
        + rng.integers(-E0 + 1, E0, size=m).astype(object)
    lwe = np.concatenate([a, (b % 2 ** 64).astype(np.uint64)[:, None]], axis=1).reshape(-1)
    got = run_pack(torch, plan, "device", lwe, kr, m, k, beta, ell, True).reshape(2, n)
    ph = [int(x) for x in ((got[1].astype(object) - times_binary(got[0][None, :], NS)[0]) % 2 ** 64)]
    dec = [decode(ph[j * n // m], bits, w) for j in range(m)]
    assert dec == msgs, dec
    want = [0] * n
    for j, x in enumerate(msgs):
        want[j * n // m] = x << (w - bits)
    err = [(x - y) % 2 ** 64 for x, y in zip(ph, want)]
    worst = max(min(e, 2 ** 64 - e) for e in err)
    print("native ring pack n = %d, M = %d: worst error 2^%.2f over %d coefficients, derived bound 2^%.2f" % (n, m, np.log2(max(worst, 1)), n, np.log2(bound)))
    assert worst < bound


# -- 5. the C example ----------------------------------------------------------------------------------------------------------------------
def test_ring_pack_native_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "ring_pack_native"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "ring_pack_native")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
