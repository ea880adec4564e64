"""The multi-bit bootstrap of the native plans (include/cntt_multibit.h) on the MI355X.  Bit-exact: the accumulate kernel against the
per-prime model (tests/native_multibit_model.py, checked on the CPU) on every Plan32 kind, on both sides of the four-product fold, with
all-(P - 1) operands and over a second trip of the grid; the blind rotation against the composition of public calls (PLAIN decompose ->
cntt_native_external_product_batch per pattern -> rotate -> sum) and against the ring model; the bootstrap against its three steps,
with and without a caller workspace, through the host path and graph-captured after one eager call."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_multibit_model import PRIMES32, fast_accumulate_plane, mb_offset, model_multibit_rotate, rotate, subset_exponents
from test_gpu_native_pbs import (KINDS, _torch, dev, host, key_planes, per, random_key_words, random_words, seed, to_array, to_ints, wbits)

pytestmark = pytest.mark.gpu

PLAN32 = ["native32_plan32", "native64_plan32", "native128_plan32", "native_binary32_plan32", "native_binary64_plan32",
          "native_binary128_plan32"]


def psis_of(torch, plan):
    """psi_i = fwd(X)[0] on every residue plane"""
    n = plan.ntt_size()
    x = to_array(plan, [0, 1] + [0] * (n - 2))
    res = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(dev(torch, x), res)
    torch.cuda.synchronize()
    return [int(host(r, np.uint32)[0]) for r in res]


def planes(torch, arrays):
    return [dev(torch, a) for a in arrays]


def run_accumulate(torch, plan, psis, T, K, rows, nterms, nout, g, batch):
    n = plan.ntt_size()
    out = [dev(torch, np.full(batch * nout * n, 0xFFFFFFFF, dtype=np.uint32)) for _ in range(plan.NPRIMES)]
    plan.multibit_accumulate_batch(out, planes(torch, T), dev(torch, rows), planes(torch, K), nterms, nout, g)
    torch.cuda.synchronize()
    for i in range(plan.NPRIMES):
        want = fast_accumulate_plane(T[i], K[i], rows, psis[i], n, PRIMES32[i], nterms, nout, g, batch)
        got = host(out[i], np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (i, nterms, nout, g, batch, "first bad word", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


# -- 1. the accumulate kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 64])
@pytest.mark.parametrize("kind", PLAN32)
def test_accumulate_matches_model(kind, n):
    """every kind (so every nprimes), g = 1 ... 4, nout = 1 ... 3, nterms on both sides of the fold (1, 3, 4, 5, 8, 9), random canonical
    residues and all-(P - 1) operands, the exponents 0, n, 2n - 1 in every group, batch 3 (odd)"""
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    psis = psis_of(torch, plan)
    rng = np.random.default_rng(seed("nmb/acc", kind, n))
    batch = 3
    for case, (g, nout, nterms) in enumerate([(1, 1, 1), (2, 2, 3), (3, 3, 4), (4, 1, 5), (2, 3, 8), (3, 2, 9), (4, 2, 4), (1, 3, 9)]):
        rows = rng.integers(0, 2 * n, size=g * batch, dtype=np.uint32)
        rows[:3] = [0, n, 2 * n - 1][:len(rows[:3])]
        worst = case % 2 == 1
        T, K = [], []
        for i in range(plan.NPRIMES):
            p = PRIMES32[i]
            if worst:
                T.append(np.full(batch * nterms * n, p - 1, dtype=np.uint32))
                K.append(np.full((nterms * nout << g) * n, p - 1, dtype=np.uint32))
            else:
                T.append(rng.integers(0, p, size=batch * nterms * n, dtype=np.uint32))
                K.append(rng.integers(0, p, size=(nterms * nout << g) * n, dtype=np.uint32))
        run_accumulate(torch, plan, psis, T, K, rows, nterms, nout, g, batch)


def test_accumulate_over_a_second_grid_trip():
    """a batch one plane's grid cannot cover in one trip, derived from cntt_native_multibit_grid; exponents taken mod 2n on the device"""
    torch = _torch()
    n, g, nout, nterms = 32, 2, 1, 5
    plan = KINDS["native32_plan32"].try_new(n)
    cap = cntt.lib().cntt_native_multibit_grid(1 << 40)
    batch = cap * 256 // (n // 4) + 3
    assert cntt.lib().cntt_native_multibit_grid(batch * nout * n // 4) == cap and batch * nout * n // 4 > cap * 256
    rng = np.random.default_rng(seed("nmb/trip"))
    rows = rng.integers(0, 1 << 32, size=g * batch, dtype=np.uint32)
    T = [rng.integers(0, PRIMES32[i], size=batch * nterms * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
    K = [rng.integers(0, PRIMES32[i], size=(nterms * nout << g) * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
    run_accumulate(torch, plan, psis_of(torch, plan), T, K, rows, nterms, nout, g, batch)


def test_accumulate_empty_sums_and_host_path():
    torch = _torch()
    n, g, nout, batch = 32, 2, 2, 2
    plan = KINDS["native64_plan32"].try_new(n)
    psis = psis_of(torch, plan)
    rows = np.array([0, n, 2 * n - 1, 5], dtype=np.uint32)
    out = [dev(torch, np.full(batch * nout * n, 7, dtype=np.uint32)) for _ in range(plan.NPRIMES)]
    empty = [dev(torch, np.zeros(0, dtype=np.uint32)) for _ in range(plan.NPRIMES)]
    plan.multibit_accumulate_batch(out, empty, dev(torch, rows), empty, 0, nout, g)
    torch.cuda.synchronize()
    assert all(int(host(o, np.uint32).sum()) == 0 for o in out)
    rng = np.random.default_rng(seed("nmb/acc/host"))
    nterms = 6
    T = [rng.integers(0, PRIMES32[i], size=batch * nterms * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
    K = [rng.integers(0, PRIMES32[i], size=(nterms * nout << g) * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
    hout = [np.zeros(batch * nout * n, dtype=np.uint32) for _ in range(plan.NPRIMES)]
    plan.multibit_accumulate_batch(hout, T, rows, K, nterms, nout, g)
    for i in range(plan.NPRIMES):
        assert np.array_equal(hout[i], fast_accumulate_plane(T[i], K[i], rows, psis[i], n, PRIMES32[i], nterms, nout, g, batch))
    bad = rows.copy()
    bad[2] = 2 * n
    with pytest.raises(cntt.Panic, match="rot_rows"):
        plan.multibit_accumulate_batch(hout, T, bad, K, nterms, nout, g)


# -- 2. the blind rotation -----------------------------------------------------------------------------------------------------------------
def composed_rotate(torch, plan, lut, rot_t, kp, L, k, beta, ell, g, batch):
    """the public calls the rotation replaces: set-up by rotating lut on the host, then per group PLAIN decompose ->
    external_product_batch per pattern -> rotate by e_t -> sum mod 2^w"""
    n, w = plan.ntt_size(), wbits(plan)
    M, J, P = 1 << w, (k + 1) * ell, per(plan)
    li = to_ints(plan, lut)
    acc = []
    for b in range(batch):
        for q in range(k + 1):
            acc += rotate(li[q * n:(q + 1) * n], int(rot_t[L * batch + b]), M)
    for r in range(L // g):
        d_acc = dev(torch, to_array(plan, acc))
        digits = torch.zeros(batch * J * P, dtype=d_acc.dtype, device="cuda")
        plan.gadget_decompose_batch(digits, d_acc, beta, ell)
        total = [0] * len(acc)
        for t in range(1 << g):
            lo, hi = mb_offset(r, t, 0, 0, g, J, k) * n, mb_offset(r, t + 1, 0, 0, g, J, k) * n
            tmp = torch.zeros(batch * (k + 1) * P, dtype=d_acc.dtype, device="cuda")
            plan.external_product_batch(tmp, digits, [x[lo:hi] for x in kp], J, k + 1)
            torch.cuda.synchronize()
            prod = to_ints(plan, host(tmp, plan.word_dtype))
            for b in range(batch):
                e = subset_exponents([int(rot_t[(r * g + i) * batch + b]) for i in range(g)], n)[t]
                for q in range(k + 1):
                    s = (b * (k + 1) + q) * n
                    rot = rotate(prod[s:s + n], e, M)
                    total[s:s + n] = [(x + y) % M for x, y in zip(total[s:s + n], rot)]
        acc = total
    return acc


def rotation_case(torch, kind, n, k, g, L, batch, beta, ell, tag, where="device", with_ws=False):
    """where = "host": the call on host slices (a host-side workspace is checked and then ignored); with_ws: the figure of
    multibit_pbs_workspace_bytes, which covers what the rotation alone needs"""
    plan = KINDS[kind].try_new(n)
    J = (k + 1) * ell
    rng = np.random.default_rng(seed("nmb/rot", kind, n, k, g, L, tag))
    lut = random_words(rng, plan, (k + 1) * n)
    rot_t = rng.integers(0, 2 * n, size=(L + 1) * batch, dtype=np.uint32)
    if L >= 2:
        rot_t[0], rot_t[batch] = 2 * n - 1, n                        # a subset sum that wraps 2n (g >= 2)
    key_words = random_key_words(rng, plan, ((L // g) * J * (k + 1)) << g)
    # (no mask words: no key, and nothing for fwd_batch to transform)
    kp = key_planes(torch, plan, key_words) if L else [torch.zeros(0, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    nws = plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch)
    if where == "host":
        h_acc = to_array(plan, [1] * (batch * (k + 1) * n))
        plan.multibit_blind_rotate_batch(h_acc, lut, rot_t, [host(x, np.uint32).copy() for x in kp], L, k, beta, ell, g,
                                         workspace=np.zeros(nws, dtype=np.uint8) if with_ws else None)
        return plan, lut, rot_t, key_words, kp, to_ints(plan, h_acc)
    acc = dev(torch, to_array(plan, [1] * (batch * (k + 1) * n)))
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.multibit_blind_rotate_batch(acc, dev(torch, lut), dev(torch, rot_t), kp, L, k, beta, ell, g, workspace=ws)
    torch.cuda.synchronize()
    return plan, lut, rot_t, key_words, kp, to_ints(plan, host(acc, plan.word_dtype))


@pytest.mark.parametrize("g", [1, 2, 3, 4])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("kind", ["native32_plan32", "native64_plan32", "native128_plan32", "native_binary64_plan32"])
def test_blind_rotate_equals_the_public_calls_and_the_model(kind, k, g):
    torch = _torch()
    n, L, batch, ell = 32, 2 * g, 2, 2
    beta = wbits(KINDS[kind]) // 4 - 1
    plan, lut, rot_t, key_words, kp, got = rotation_case(torch, kind, n, k, g, L, batch, beta, ell, "a")
    assert got == composed_rotate(torch, plan, lut, rot_t, kp, L, k, beta, ell, g, batch), (kind, k, g)
    if k == 1:
        want = model_multibit_rotate(to_ints(plan, lut), rot_t, to_ints(plan, key_words), wbits(plan), n, L, k, beta, ell, g, batch)
        assert got == want, (kind, g)


def test_blind_rotate_at_4096_and_without_mask_words():
    torch = _torch()
    plan, lut, rot_t, _, kp, got = rotation_case(torch, "native64_plan32", 4096, 1, 2, 2, 1, 15, 2, "big")
    assert got == composed_rotate(torch, plan, lut, rot_t, kp, 2, 1, 15, 2, 2, 1)
    plan, lut, rot_t, _, kp, got = rotation_case(torch, "native32_plan32", 32, 1, 3, 0, 2, 7, 2, "zero")
    assert got == composed_rotate(torch, plan, lut, rot_t, kp, 0, 1, 7, 2, 3, 2)
    # one group and no group, with a caller workspace on the device and through the host path with and without one: the same words
    for L in (2, 0):
        plan, lut, rot_t, _, kp, got = rotation_case(torch, "native32_plan32", 32, 1, 2, L, 2, 7, 2, "frames")
        assert got == composed_rotate(torch, plan, lut, rot_t, kp, L, 1, 7, 2, 2, 2), L
        for where, with_ws in (("device", True), ("host", False), ("host", True)):
            assert rotation_case(torch, "native32_plan32", 32, 1, 2, L, 2, 7, 2, "frames", where, with_ws)[5] == got, (L, where, with_ws)


# -- 3. the bootstrap ---------------------------------------------------------------------------------------------------------------------
def bootstrap_case(torch, kind, n, k, g, L, batch, ell, tag):
    plan = KINDS[kind].try_new(n)
    J = (k + 1) * ell
    rng = np.random.default_rng(seed("nmb/pbs", kind, n, k, g, L, tag))
    lut = random_words(rng, plan, (k + 1) * n)
    lwe = random_words(rng, plan, batch * (L + 1))
    key_words = random_key_words(rng, plan, ((L // g) * J * (k + 1)) << g)
    return plan, lut, lwe, key_words


def three_steps(torch, plan, lut, lwe, kp, L, k, beta, ell, g, batch):
    n = plan.ntt_size()
    rot_t = torch.zeros((L + 1) * batch, dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_batch(rot_t, dev(torch, lwe), L)
    acc = dev(torch, to_array(plan, [0] * (batch * (k + 1) * n)))
    plan.multibit_blind_rotate_batch(acc, dev(torch, lut), rot_t, kp, L, k, beta, ell, g)
    out = dev(torch, to_array(plan, [0] * (batch * (k * n + 1))))
    plan.sample_extract_batch(out, acc, k)
    torch.cuda.synchronize()
    return host(out, plan.word_dtype)


@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("kind", ["native32_plan32", "native64_plan32", "native128_plan32", "native_binary32_plan32"])
def test_bootstrap_equals_its_three_steps(kind, g):
    """with and without a caller workspace, through the host path, and replayed from a graph captured after the eager calls"""
    torch = _torch()
    n, k, L, batch, ell = 64, 1, 2 * g, 3, 2
    beta = wbits(KINDS[kind]) // 4
    plan, lut, lwe, key_words = bootstrap_case(torch, kind, n, k, g, L, batch, ell, "steps")
    kp = key_planes(torch, plan, key_words)
    want = three_steps(torch, plan, lut, lwe, kp, L, k, beta, ell, g, batch)
    d_lut, d_lwe = dev(torch, lut), dev(torch, lwe)
    out = dev(torch, to_array(plan, [1] * (batch * (k * n + 1))))
    plan.multibit_bootstrap_batch(out, d_lwe, d_lut, kp, L, k, beta, ell, g)
    torch.cuda.synchronize()
    assert np.array_equal(host(out, plan.word_dtype), want)
    ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch), dtype=torch.uint8, device="cuda")
    out2 = dev(torch, to_array(plan, [2] * (batch * (k * n + 1))))
    plan.multibit_bootstrap_batch(out2, d_lwe, d_lut, kp, L, k, beta, ell, g, workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(host(out2, plan.word_dtype), want)
    hout = to_array(plan, [3] * (batch * (k * n + 1)))
    plan.multibit_bootstrap_batch(hout, lwe, lut, [host(x, np.uint32) for x in kp], L, k, beta, ell, g)
    assert np.array_equal(hout, want)
    # graph capture: the tables exist (eager calls above), a caller workspace, so a linear chain of kernels
    out3 = dev(torch, to_array(plan, [4] * (batch * (k * n + 1))))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.multibit_bootstrap_batch(out3, d_lwe, d_lut, kp, L, k, beta, ell, g, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(out3, plan.word_dtype), want)


def test_bootstrap_without_mask_words_equals_its_three_steps():
    """lwe_dim = 0: no group, no key; device without and with a caller workspace, and the host path"""
    torch = _torch()
    kind, n, k, g, L, batch, ell, beta = "native32_plan32", 64, 1, 2, 0, 2, 2, 8
    plan, lut, lwe, _ = bootstrap_case(torch, kind, n, k, g, L, batch, ell, "zero")
    kp = [torch.zeros(0, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    want = three_steps(torch, plan, lut, lwe, kp, L, k, beta, ell, g, batch)
    assert want.any()
    for ws in (None, torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch), dtype=torch.uint8, device="cuda")):
        out = dev(torch, to_array(plan, [1] * (batch * (k * n + 1))))
        plan.multibit_bootstrap_batch(out, dev(torch, lwe), dev(torch, lut), kp, L, k, beta, ell, g, workspace=ws)
        torch.cuda.synchronize()
        assert np.array_equal(host(out, plan.word_dtype), want), ws is None
    hout = to_array(plan, [3] * (batch * (k * n + 1)))
    plan.multibit_bootstrap_batch(hout, lwe, lut, [host(x, np.uint32) for x in kp], L, k, beta, ell, g)
    assert np.array_equal(hout, want)


def test_device_refusals_leave_the_outputs_untouched():
    torch = _torch()
    n, k, L, batch, ell, beta, g = 32, 1, 4, 2, 2, 8, 2
    plan, lut, lwe, key_words = bootstrap_case(torch, "native64_plan32", n, k, g, L, batch, ell, "refuse")
    kp = key_planes(torch, plan, key_words)
    out = dev(torch, to_array(plan, [9] * (batch * (k * n + 1))))
    d_lut, d_lwe = dev(torch, lut), dev(torch, lwe)
    small = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch) - 1, dtype=torch.uint8, device="cuda")
    for kwargs, args, text in (({}, (L, k, beta, ell, 5), "grouping = 5"), ({}, (L, k, beta, ell, 3), "multiple of grouping"),
                               ({}, (L, k, 33, ell, g), "word width"), ({"workspace": small}, (L, k, beta, ell, g), "workspace_bytes")):
        with pytest.raises(cntt.Panic, match=text):
            plan.multibit_bootstrap_batch(out, d_lwe, d_lut, kp, *args, **kwargs)
    with pytest.raises(cntt.Panic, match="overlaps"):
        plan.multibit_bootstrap_batch(out, out[:batch * (L + 1)], d_lut, kp, L, k, beta, ell, g)
    p52 = KINDS["native64_plan52"].try_new(n)
    k52 = [torch.zeros(kp[0].numel(), dtype=torch.int64, device="cuda") for _ in range(p52.NPRIMES)]
    with pytest.raises(cntt.Panic, match="Plan52"):
        p52.multibit_bootstrap_batch(out, d_lwe, d_lut, k52, L, k, beta, ell, g)
    torch.cuda.synchronize()
    assert to_ints(plan, host(out, plan.word_dtype)) == [9] * (batch * (k * n + 1))
