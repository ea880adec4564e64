"""The circuit bootstrap of the native plans (include/cntt_cbs.h) on the MI355X.  Bit-exact, no tolerance: the call against the sequence of
public calls of its convention (Lc bootstraps, (k + 1) Lc packing keyswitches at lwe_count = 1 on (u, 0), fwd) on the five non-binary
kinds; its keyswitch half against the plain-int model with every digit forced to -B / 2 and key words of all ones; a ragged E-tile, three
slabs with a ragged last one and a second trip of the grid; the host path; a non-default stream; L = 0; graph capture.  The one functional
test -- circuit-bootstrapped address bits drive a whole table lookup -- derives its bound in its docstring."""
import os
import random
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_cbs_model import H, bsk, fpksk, lwe_encrypt, model_keyswitch_rows, selector_from_rows, shape
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, per, random_words, seed, to_array, to_ints, wbits
from test_gpu_prime_pack import first_difference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONBINARY = ["native32_plan32", "native64_plan32", "native128_plan32", "native32_plan52", "native64_plan52"]


def sizes(k, n, Lk, Lc):
    """(Lin, R, polynomials of one selector, polynomials of fpksk)"""
    lin = k * n
    return lin, (lin + 1) * Lk, (k + 1) * Lc * (k + 1), (k + 1) * (lin + 1) * Lk * (k + 1)


def res_t(torch, plan):
    return torch.int64 if plan.RES == 8 else torch.int32


def run_cbs(torch, plan, where, lwe, bsk_planes, fk, L, k, gad, with_ws=False, stream=None):
    """the call on word arrays (the bootstrapping key as device planes) -> the NPRIMES output planes as arrays, poisoned before"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // ((L + 1) * (2 if plan.WORD == 16 else 1))
    count = batch * sizes(k, n, kl, cl)[2] * n
    nws = plan.circuit_bootstrap_workspace_bytes(L, k, pl, kl, cl, batch)
    if where == "host":
        outs = [np.full(count, 0x5A5A5A5A, dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.circuit_bootstrap_batch(outs, lwe, None if bsk_planes is None else [host(p, plan.res_dtype).copy() for p in bsk_planes], fk, L, k, pb, pl,
                                     kb, kl, cb, cl, workspace=ws)
        return outs
    outs = [torch.full((count,), 0x5A5A5A5A, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    lwe_t, fk_t = dev(torch, lwe), dev(torch, fk)
    torch.cuda.synchronize()
    if stream is None:
        plan.circuit_bootstrap_batch(outs, lwe_t, bsk_planes, fk_t, L, k, pb, pl, kb, kl, cb, cl, workspace=ws)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            plan.circuit_bootstrap_batch(outs, lwe_t, bsk_planes, fk_t, L, k, pb, pl, kb, kl, cb, cl, workspace=ws)
        stream.synchronize()
    return [host(o, plan.res_dtype) for o in outs]


def public_u(torch, plan, lwe, bsk_planes, L, k, gad):
    """steps 1 and 2 from public calls: u[l - 1] = batch lists of Lin + 1 ints for l = 1 .. Lc"""
    pb, pl, kb, kl, cb, cl = gad
    n, w = plan.ntt_size(), wbits(plan)
    M = 1 << w
    x = to_ints(plan, lwe)
    batch = len(x) // (L + 1)
    for b in range(batch):
        x[b * (L + 1) + L] = (x[b * (L + 1) + L] + (1 << (w - 2))) % M
    lwe1 = dev(torch, to_array(plan, x))
    bsk_arg = bsk_planes if L else [torch.empty(0, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
    us = []
    for l in range(1, cl + 1):
        h = H(w, cb, l)
        lut = to_array(plan, [0] * (k * n) + [M - h] * n)
        u_t = dev(torch, to_array(plan, [0] * (batch * (k * n + 1))))
        plan.bootstrap_batch(u_t, lwe1, dev(torch, lut), bsk_arg, L, k, pb, pl)
        torch.cuda.synchronize()
        u = to_ints(plan, host(u_t, plan.word_dtype))
        rows = [u[b * (k * n + 1):(b + 1) * (k * n + 1)] for b in range(batch)]
        for r in rows:
            r[k * n] = (r[k * n] + h) % M
        us.append(rows)
    return us


def fwd_planes(torch, plan, words):
    """cntt_native_fwd_batch over word ints -> NPRIMES arrays"""
    return [host(p, plan.res_dtype) for p in key_planes(torch, plan, to_array(plan, words))]


def compose_cbs(torch, plan, lwe, bsk_planes, fk, L, k, gad):
    """the header's sequence of public calls, step 3 as pack_keyswitch_batch on (u, 0) with lwe_count = 1, step 4 as fwd_batch"""
    pb, pl, kb, kl, cb, cl = gad
    n, pe = plan.ntt_size(), per(plan)
    lin, R, selp, _ = sizes(k, n, kl, cl)
    us = public_u(torch, plan, lwe, bsk_planes, L, k, gad)
    batch = len(us[0])
    fq = [key_planes(torch, plan, fk[q * R * (k + 1) * pe:(q + 1) * R * (k + 1) * pe]) for q in range(k + 1)]
    out = [np.zeros((batch, (k + 1) * cl, (k + 1) * n), dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
    for l, rows in enumerate(us):
        ct = dev(torch, to_array(plan, [x for r in rows for x in r + [0]]))            # the whole of u is the mask, the body word is 0
        for q in range(k + 1):
            g = dev(torch, to_array(plan, [0] * (batch * (k + 1) * n)))
            plan.pack_keyswitch_batch(g, ct, fq[q], lin + 1, 1, k, kb, kl)
            planes = [torch.empty(batch * (k + 1) * n, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
            plan.fwd_batch(g, planes)
            torch.cuda.synchronize()
            for i, p in enumerate(planes):
                out[i][:, q * cl + l] = host(p, plan.res_dtype).reshape(batch, (k + 1) * n)
    return [o.reshape(-1) for o in out]


def random_case(torch, plan, rng, L, k, gad, batch):
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    lwe = random_words(rng, plan, batch * (L + 1))
    bsk_planes = key_planes(torch, plan, random_words(rng, plan, L * (k + 1) * pl * (k + 1) * n)) if L else None
    fk = random_words(rng, plan, sizes(k, n, kl, cl)[3] * n)
    return lwe, bsk_planes, fk


def gadgets(w, Lk, Lc):
    """(pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels): the keyswitch gadget is as wide as it may be; the PBS
    gadget keeps all bits of the constants -H_l; cbs_base_log * Lc = w - 1 for Lc = 1, the edge of its rule"""
    return (w // 4, 4, min(31, w // Lk), Lk, w - 1 if Lc == 1 else 5, Lc)


def same(got, want):
    return all(np.array_equal(g, x) for g, x in zip(got, want))


def diff(got, want):
    return [first_difference(g, x) for g, x in zip(got, want) if not np.array_equal(g, x)][:1]


# -- 1. against the public calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", NONBINARY)
def test_equals_the_public_call_sequence(kind):
    """n = 32, k in {1, 2}, L = 4, batch in {1, 3, 5}, Lc in {1, 2}, Lk in {1, 3}; with and without a caller workspace; the Plan52 kinds
    also at n = 16, where the external product is the composed pipeline"""
    torch = _torch()
    rng = np.random.default_rng(seed("ncbs", kind))
    cases = [(32, 1, 4, 1, 1, 1), (32, 2, 4, 3, 2, 3), (32, 1, 4, 5, 2, 1)] + ([(16, 1, 4, 3, 2, 3)] if kind.endswith("plan52") else [])
    for n, k, L, batch, Lc, Lk in cases:
        plan = KINDS[kind].try_new(n)
        gad = gadgets(wbits(plan), Lk, Lc)
        assert (k + 1) * gad[1] <= plan.max_terms()
        lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
        want = compose_cbs(torch, plan, lwe, bsk_planes, fk, L, k, gad)
        for with_ws in (False, True):
            got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, with_ws)
            assert all(g.any() for g in got) and same(got, want), (kind, n, k, L, batch, gad, with_ws, diff(got, want))


# -- 2. the keyswitch half against the model, digits at the extreme -----------------------------------------------------------------------
@pytest.mark.parametrize("kind,k,Lk", [("native32_plan32", 1, 1), ("native64_plan32", 0, 1), ("native64_plan32", 2, 1), ("native128_plan32", 0, 1),
                                       ("native128_plan32", 1, 3), ("native128_plan32", 2, 3), ("native64_plan52", 1, 1)])
def test_keyswitch_half_with_every_digit_at_minus_half_the_base_and_key_words_of_all_ones(kind, k, Lk):
    """ks_base_log = 31 (Lk = 3 needs 93 bits: native128).  Every word of u is x = -sum_j 2^30 2^(w - 31 j), whose digits are -B / 2 on every
    level, and every key word is 2^w - 1: the subtraction runs a borrow through every limb of the accumulator.  u is forced through the
    inputs: L = 1, the body of lwe_in is 3 * 2^(w - 2), so the body of lwe' is 0 and the set-up accumulator is the constant -H_1 without a
    rotation; lwe_in[0] = 2^(w - 1) has ms = n, so the CMux difference is -2 acc = the constant polynomial G_1, one digit 1 in every
    coefficient under the PBS gadget (cbs_base_log, 1); the bootstrapping key row (body, level 1) is -x X on the masks and x on the
    body, and (1 + X + ... + X^(n - 1)) (-x X) = (x, -x, ..., -x), which the sample extraction turns into x everywhere."""
    torch = _torch()
    n, L, batch, cb = 32, 1, 11, 4
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    M = 1 << w
    gad = (cb, 1, 31, Lk, cb, 1)
    lin, R, selp, fkp = sizes(k, n, Lk, 1)
    x = (-sum(1 << (30 + w - 31 * j) for j in range(1, Lk + 1))) % M
    lwe = to_array(plan, [1 << (w - 1), 3 << (w - 2)] * batch)
    key = [0] * ((k + 1) * (k + 1) * n)                                  # rows (q, 1) x o
    for o in range(k + 1):
        base = (k * (k + 1) + o) * n
        if o < k:
            key[base + 1] = (-x) % M
        else:
            key[base] = x
    bsk_planes = key_planes(torch, plan, to_array(plan, key))
    us = public_u(torch, plan, lwe, bsk_planes, L, k, gad)
    assert all(r == [x] * (lin + 1) for r in us[0]), "the inputs do not force u"
    fk_ints = [M - 1] * (fkp * n)
    rows = model_keyswitch_rows(us[0][0], fk_ints, w, k, n, 31, Lk)
    assert rows[0][0] == (-(lin + 1) * Lk << 30) % M                     # -sum d (-1) = sum d
    want = fwd_planes(torch, plan, selector_from_rows([rows], k, n) * batch)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, to_array(plan, fk_ints), L, k, gad)
    assert all(g.any() for g in got) and same(got, want), (kind, k, Lk, diff(got, want))


@pytest.mark.parametrize("kind,k,Lk", [("native64_plan32", 1, 2), ("native128_plan32", 2, 3), ("native32_plan32", 0, 1)])
def test_keyswitch_half_equals_the_model_on_random_words(kind, k, Lk):
    """u from the public bootstrap, step 3 from the plain-int model, step 4 from fwd_batch"""
    torch = _torch()
    n, L, batch = 32, 4, 3
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    gad = gadgets(w, Lk, 2)
    rng = np.random.default_rng(seed("ncbs-model", kind))
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    us = public_u(torch, plan, lwe, bsk_planes, L, k, gad)
    fk_ints = to_ints(plan, fk)
    sel = []
    for b in range(batch):
        sel += selector_from_rows([model_keyswitch_rows(u[b], fk_ints, w, k, n, gad[2], gad[3]) for u in us], k, n)
    want = fwd_planes(torch, plan, sel)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
    assert all(g.any() for g in got) and same(got, want), (kind, diff(got, want))


# -- 3. ragged tile, slabs, a second trip of the grid -------------------------------------------------------------------------------------
def test_three_slabs_with_a_ragged_last_one_and_a_ragged_tile():
    """n = 64, k = 1, Lk = 3: R = 195 rows are four slabs of 49 rows, the last one of 48; 11 elements are one full tile and one of 3"""
    torch = _torch()
    kind, n, k, L, batch, Lk, Lc = "native64_plan32", 64, 1, 4, 11, 3, 1
    plan = KINDS[kind].try_new(n)
    gad = gadgets(64, Lk, Lc)
    cols, tiles, rows, slabs = shape(n, 8, k, sizes(k, n, Lk, Lc)[1], batch)
    assert slabs >= 3 and rows * slabs > sizes(k, n, Lk, Lc)[1] and batch % 8 and tiles == 2
    rng = np.random.default_rng(seed("ncbs-slabs"))
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    want = compose_cbs(torch, plan, lwe, bsk_planes, fk, L, k, gad)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
    assert same(got, want), diff(got, want)


@pytest.mark.parametrize("kind", ["native64_plan32", "native32_plan32"])
def test_ragged_tile_and_a_second_trip_of_the_grid(kind):
    """8195 elements are 1024 full tiles and one of 3; with one column block, k + 1 = 2 keys and one slab that is 2050 work items for a
    grid capped at 2048: two workgroups make a second trip.  L = 1 keeps it in seconds and still fills the masks of u; the reference
    is the model on the u of the public bootstrap for the first and the last elements, and the call on two halves for every word."""
    torch = _torch()
    n, k, L, batch = 32, 1, 1, 8195
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    gad = (w // 4, 4, 31, 1, 5, 1)
    lin, R, selp, fkp = sizes(k, n, 1, 1)
    cols, tiles, rows, slabs = shape(n, plan.WORD, k, R, batch)
    items = (k + 1) * cols * tiles * slabs
    cap = cntt.lib().cntt_native_cbs_grid(1 << 30, 5, plan.WORD)
    assert cntt.lib().cntt_native_cbs_grid(items, 5, plan.WORD) == cap < items < 2 * cap and batch % 8 == 3 and slabs == 1
    rng = np.random.default_rng(seed("ncbs-ragged", kind))
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
    half = 4096
    for lo, hi in ((0, half), (half, batch)):
        part = run_cbs(torch, plan, "device", lwe[lo * (L + 1):hi * (L + 1)], bsk_planes, fk, L, k, gad)
        assert same([g[lo * selp * n:hi * selp * n] for g in got], part), (kind, lo, hi)
    ends = np.concatenate([lwe[:2 * (L + 1)], lwe[-3 * (L + 1):]])
    us = public_u(torch, plan, ends, bsk_planes, L, k, gad)
    fk_ints = to_ints(plan, fk)
    sel = []
    for b in range(5):
        sel += selector_from_rows([model_keyswitch_rows(us[0][b], fk_ints, w, k, n, gad[2], gad[3])], k, n)
    want = fwd_planes(torch, plan, sel)
    for g, x in zip(got, want):
        assert np.array_equal(np.concatenate([g[:2 * selp * n], g[-3 * selp * n:]]), x), kind
        assert g[-3 * selp * n:].any()


# -- 4. host path, stream, L = 0, graph capture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32", "native32_plan52"])
def test_host_path_equals_device_path_and_lwe_dim_zero(kind):
    torch = _torch()
    n, k, batch = 32, 1, 3
    plan = KINDS[kind].try_new(n)
    rng = np.random.default_rng(seed("ncbs-host", kind))
    for L, Lk, Lc in ((4, 3, 2), (0, 1, 2)):                             # lwe_dim == 0: the set-up alone, no bootstrapping key
        gad = gadgets(wbits(plan), Lk, Lc)
        lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
        want = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
        if L == 0:
            assert same(want, compose_cbs(torch, plan, lwe, None, fk, L, k, gad)), kind
        for with_ws in (True, False):
            got = run_cbs(torch, plan, "host", lwe, bsk_planes, fk, L, k, gad, with_ws)
            assert all(g.any() for g in got) and same(got, want), (kind, L, with_ws, diff(got, want))


def test_non_default_stream():
    torch = _torch()
    kind, n, k, L, batch = "native32_plan32", 32, 2, 4, 3
    plan = KINDS[kind].try_new(n)
    gad = gadgets(32, 3, 2)
    rng = np.random.default_rng(31)
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    want = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, stream=torch.cuda.Stream())
    assert same(got, want), diff(got, want)


def test_graph_capture_with_a_caller_workspace_after_one_eager_call():
    """native64 Plan32 at n = 1024, a shape the header declares capturable: captured once, replayed twice on fresh inputs"""
    torch = _torch()
    n, k, L, batch = 1024, 1, 4, 3
    gad = (8, 3, 22, 2, 8, 2)
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(29)
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    lwe_t, fk_t = dev(torch, lwe), dev(torch, fk)
    ws = torch.zeros(plan.circuit_bootstrap_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch), dtype=torch.uint8, device="cuda")
    count = batch * sizes(k, n, gad[3], gad[5])[2] * n
    outs = [torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.circuit_bootstrap_batch(outs, lwe_t, bsk_planes, fk_t, L, k, *gad, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.circuit_bootstrap_batch(outs, lwe_t, bsk_planes, fk_t, L, k, *gad, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, plan, batch * (L + 1)))
        eager = [torch.zeros_like(o) for o in outs]
        plan.circuit_bootstrap_batch(eager, fresh, bsk_planes, fk_t, L, k, *gad)
        lwe_t.copy_(fresh)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(e.any() and torch.equal(o, e) for o, e in zip(outs, eager))


# -- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def test_circuit_bootstrapped_address_bits_look_up_every_entry():
    """native64 Plan32, n = 32, k = 1, L = 4, binary keys, NOISE-FREE keys and inputs; PBS gadget (16, 4) (nothing rounded), keyswitch
    gadget (22, 2) (s = 20), selector gadget (8, 3) (s' = 40).  The two values of a bit are circuit-bootstrapped in one call; a table of
    M n = 4 * 32 3-bit entries at steps of 2^61 is looked up at every one of its 128 addresses: cmux_tree_batch over the top 2 bits,
    blind_rotate_batch with rot_t[i] = 2n - 2^i over the low 5, sample_extract_batch(index 0).
    Bound, from the headers.  Step 2 is exact (cntt_cbs.h).  The keyswitch rounding leaves every coefficient of a selector row's phase
    off by less than n (Lin + 1) 2^(s - 1) = 32 * 33 * 2^19 < 2^30 (cntt_cbs.h, the rounding bound for a binary S).  A CMux against such a
    selector adds at most (k + 1) n Lc (B / 2) 2^30 = 2 * 32 * 3 * 2^7 * 2^30 < 2^45 and the rounding of its difference to a multiple of
    2^s', (1 + k n) 2^(s' - 1) = 33 * 2^39 < 2^45 (cntt_cmux.h); it passes the error of the input it selects on unchanged.  The 2 tree
    stages and the 5 rotations are one CMux each: 7 * 2^46 < 2^49, asserted, against half a step of 2^60."""
    torch = _torch()
    w, n, k, L, m = 64, 32, 1, 4, 4
    logn, depth = 5, 2
    gad = (16, 4, 22, 2, 8, 3)
    pb, pl, kb, kl, cb, cl = gad
    plan = KINDS["native64_plan32"].try_new(n)
    rng = random.Random(seed("ncbs-e2e"))
    S = [[rng.randrange(2) for _ in range(n)]]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    bsk_planes = key_planes(torch, plan, np.array(bsk(rng, w, s_lwe, S, n, pb, pl), dtype=np.uint64))
    fk_t = dev(torch, np.array(fpksk(rng, w, S, n, kb, kl), dtype=np.uint64))
    lwe = np.array([x for bit in (0, 1) for x in lwe_encrypt(rng, w, s_lwe, bit << 63)], dtype=np.uint64)
    selp = sizes(k, n, kl, cl)[2] * n
    sels = [torch.zeros(2 * selp, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.circuit_bootstrap_batch(sels, dev(torch, lwe), bsk_planes, fk_t, L, k, *gad)

    def planes(bits):
        return [torch.cat([p[b * selp:(b + 1) * selp] for b in bits]) for p in sels]

    nrng = np.random.default_rng(seed("ncbs-e2e-table"))
    entries = nrng.integers(0, 8, size=(m, n))
    table = dev(torch, (entries.astype(np.uint64) << np.uint64(61)).reshape(-1))
    rot_t = dev(torch, np.array([2 * n - (1 << i) for i in range(logn)] + [0], dtype=np.uint32))
    accs = torch.zeros(m * n * (k + 1) * n, dtype=torch.int64, device="cuda")
    glwe = torch.zeros((k + 1) * n, dtype=torch.int64, device="cuda")
    low = [planes([(a >> i) & 1 for i in range(logn)]) for a in range(n)]
    for hi in range(m):
        plan.cmux_tree_batch(glwe, table, planes([(hi >> i) & 1 for i in range(depth)]), m, k, cb, cl)
        for lo in range(n):
            a = hi * n + lo
            plan.blind_rotate_batch(accs[a * (k + 1) * n:(a + 1) * (k + 1) * n], glwe, rot_t, low[lo], logn, k, cb, cl, lut_per_element=True)
    out = torch.zeros(m * n * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.sample_extract_batch(out, accs, k, 0)
    torch.cuda.synchronize()
    rows = host(out, np.uint64).reshape(m * n, n + 1)
    with np.errstate(over="ignore"):
        phase = rows[:, n] - (rows[:, :n] * np.array(S[0], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    dec = [int(((int(x) >> 60) + 1) >> 1) & 7 for x in phase]
    want = entries.reshape(-1).tolist()
    err = [(int(x) - (y << 61)) % 2 ** 64 for x, y in zip(phase, want)]
    worst = max(min(e, 2 ** 64 - e) for e in err)
    bound = (depth + logn) * ((k + 1) * n * cl * (1 << (cb - 1)) * (n * (k * n + 1) << 19) + ((1 + k * n) << 39))
    assert bound < 1 << 49
    print("circuit bootstrap + lookup M = %d: worst error 2^%.2f over %d addresses, derived bound 2^%.2f" % (m, np.log2(max(worst, 1)), m * n, np.log2(bound)))
    assert dec == want, [i for i, (x, y) in enumerate(zip(dec, want)) if x != y][:8]
    assert worst < bound


# -- 6. the C example -----------------------------------------------------------------------------------------------------------------------
def test_cbs_lookup_native_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "cbs_lookup_native"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "cbs_lookup_native")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "every looked-up entry decoded" in r.stdout, r.stdout
