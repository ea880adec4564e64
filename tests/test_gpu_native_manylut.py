"""The many-LUT bootstrap and the one-rotation circuit bootstrap of the native plans (include/cntt_manylut.h) on the MI355X.  Bit-exact, no
tolerance: the coarse modulus switch and the extraction of several indices against the plain-int model and against single
sample_extract_batch calls; bootstrap_manylut_batch against its three public steps on all ten kinds and against bootstrap_batch at
t = 0; circuit_bootstrap_manylut_batch against the sequence of public calls of its convention on the five non-binary kinds, against
circuit_bootstrap_batch at t = 0, Lc = 1, past one trip of the product grid, at lwe_dim = 0, on the host path, on a non-default stream
and graph-captured; four tables on every 3-bit message in one bootstrap, and a whole table lookup whose selectors the new call produced."""
import os
import random
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from native_cbs_model import H, bsk, fpksk, lwe_encrypt, shape
from native_manylut_model import cbs_table, interleave, model_extract_many, model_modswitch_coarse
from test_gpu_native_cbs import NONBINARY, diff, random_case, res_t, same, sizes
from test_gpu_native_pbs import (KINDS, STREAM_BYTES, WORDS, _torch, dev, host, key_planes, per, random_key_words, random_words, seed, to_array,
                                 to_ints, wbits)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- 1. the coarse modulus switch ---------------------------------------------------------------------------------------------------------
def coarse_words(rng, w, logn, t, count):
    """zeros, all-ones words, the exact ties of the coarse grid and the word below each, and random words in between"""
    s = w - (logn - t) - 1                                    # one coarse step
    two_np = 2 << (logn - t)
    ws = [0, (1 << w) - 1, (1 << w) - (1 << (s - 1)), (1 << w) - (1 << (s - 1)) - 1]
    for j in sorted({0, 1, two_np // 2 - 1, two_np // 2, two_np - 1}):
        ws += [(j << s) + (1 << (s - 1)), (j << s) + (1 << (s - 1)) - 1]
    return [ws[i // 2 % len(ws)] if i % 2 == 0 else int.from_bytes(rng.bytes(w // 8), "little") for i in range(count)]


def small_plan(w, n):
    """the native plans start at n = 32 (Plan32) and n = 16 (Plan52, 32- and 64-bit words): the smallest rings there are"""
    return (WORDS[w] if n >= 32 else KINDS["native%d_plan52" % w]).try_new(n)


SMALL = [(32, 16), (64, 16), (32, 32), (64, 32), (128, 32)]


@pytest.mark.parametrize("w,n", SMALL)
def test_coarse_modswitch_matches_model(w, n):
    """L + 1 = 34 words and 33 elements: both edges of the 32 x 32 transpose tile are ragged, four tiles"""
    torch = _torch()
    plan = small_plan(w, n)
    logn, L, batch = n.bit_length() - 1, 33, 33
    rng = np.random.default_rng(seed("nml-ms", w, n))
    for t in sorted({0, 1, logn - 1, logn}):
        lwe = coarse_words(rng, w, logn, t, batch * (L + 1))
        want = np.array(model_modswitch_coarse(lwe, L, batch, w, logn, t), dtype=np.uint32)
        assert (want % (1 << t) == 0).all() and want.max() < 2 * n
        la = to_array(plan, lwe)
        rot = dev(torch, np.full_like(want, 0xFFFFFFFF))
        plan.lwe_modswitch_manylut_batch(rot, dev(torch, la), L, t)
        torch.cuda.synchronize()
        got = host(rot, np.uint32)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (w, n, t, "first bad exponent", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))
        hgot = np.full_like(want, 0xFFFFFFFF)
        plan.lwe_modswitch_manylut_batch(hgot, la, L, t)
        assert np.array_equal(hgot, want), (w, n, t, "host")
        if t == 0:
            plan.lwe_modswitch_batch(rot, dev(torch, la), L)
            torch.cuda.synchronize()
            assert np.array_equal(host(rot, np.uint32), want)


# -- 2. the extraction of several indices ----------------------------------------------------------------------------------------------------
def offset_by_one_word(torch, plan, a):
    """a copy of the array on the device that starts one word past a 16-byte boundary (32- and 64-bit words)"""
    t = dev(torch, np.concatenate([np.zeros(1, dtype=a.dtype), a]))
    assert t.data_ptr() % 16 == 0
    return t[1:]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("w,n", SMALL)
def test_sample_extract_many_matches_model_and_single_extractions(w, n, k, where):
    """n = 16 (Plan52) and n = 32, batch 3; count 1, 7, 8, 9, 16: one chunk of rows, a ragged one, a full one, two chunks.  On 32- and
    64-bit words both buffers of the device path start one word past a 16-byte boundary."""
    torch = _torch()
    batch = 3
    plan = small_plan(w, n)
    rng = np.random.default_rng(seed("nml-ext", w, n, k))
    ga = random_words(rng, plan, batch * (k + 1) * n)
    gi = to_ints(plan, ga)
    row = k * n + 1
    for count in (1, 7, 8, 9, 16):
        want = []
        for b in range(batch):
            elem = [gi[(b * (k + 1) + p) * n:(b * (k + 1) + p + 1) * n] for p in range(k + 1)]
            want += model_extract_many(elem, count, w)
        want = to_array(plan, want)
        if where == "host":
            got = np.full_like(want, 0x5A)
            plan.sample_extract_many_batch(got, ga, k, count)
            assert np.array_equal(got, want), (w, k, count)
            continue
        if w == 128:
            g_t, out_t = dev(torch, ga), dev(torch, np.full_like(want, 0x5A))
        else:
            g_t, out_t = offset_by_one_word(torch, plan, ga), offset_by_one_word(torch, plan, np.full_like(want, 0x5A))
            assert g_t.data_ptr() % 16 == w // 8 and out_t.data_ptr() % 16 == w // 8
        plan.sample_extract_many_batch(out_t, g_t, k, count)
        torch.cuda.synchronize()
        got = host(out_t, want.dtype)
        assert np.array_equal(got, want), (w, k, count)
        # against `count` single extractions of the public call
        pw = 2 if w == 128 else 1
        one = dev(torch, np.zeros(batch * row * pw, dtype=want.dtype))
        g0 = dev(torch, ga)
        for h in range(count):
            plan.sample_extract_batch(one, g0, k, h)
            torch.cuda.synchronize()
            single = host(one, want.dtype).reshape(batch, row * pw)
            assert np.array_equal(got.reshape(batch, count, row * pw)[:, h], single), (w, k, count, h)


def test_sample_extract_many_streaming_variant():
    """native64 Plan52 at n = 16, k = 1, count = 16: the first batch whose output passes the streaming threshold (non-temporal stores), against
    the same call on two halves, which do not stream, and against the model on the first and the last element"""
    torch = _torch()
    w, n, k, count = 64, 16, 1, 16
    plan = small_plan(w, n)
    row = k * n + 1
    batch = STREAM_BYTES // (count * row * 8) + 1
    assert batch * count * row * 8 > STREAM_BYTES >= (batch - 1) * count * row * 8
    rng = np.random.default_rng(seed("nml-stream"))
    ga = random_words(rng, plan, batch * (k + 1) * n)
    g_t = dev(torch, ga)
    out = torch.full((batch * count * row,), 0x5A, dtype=torch.int64, device="cuda")
    plan.sample_extract_many_batch(out, g_t, k, count)
    half = batch // 2
    parts = torch.full((batch * count * row,), 0x3C, dtype=torch.int64, device="cuda")
    plan.sample_extract_many_batch(parts[:half * count * row], g_t[:half * (k + 1) * n], k, count)
    plan.sample_extract_many_batch(parts[half * count * row:], g_t[half * (k + 1) * n:], k, count)
    torch.cuda.synchronize()
    assert torch.equal(out, parts)
    gi = to_ints(plan, ga)
    for b in (0, batch - 1):
        elem = [gi[(b * (k + 1) + p) * n:(b * (k + 1) + p + 1) * n] for p in range(k + 1)]
        want = np.array(model_extract_many(elem, count, w), dtype=np.uint64)
        assert np.array_equal(host(out[b * count * row:(b + 1) * count * row], np.uint64), want), b


# -- 3. the many-LUT bootstrap --------------------------------------------------------------------------------------------------------------
def run_boot(torch, plan, lwe_t, lut_t, kr, L, k, gad, t, count, batch, with_ws=False, per_element=None):
    n, pw = plan.ntt_size(), 2 if plan.WORD == 16 else 1
    out = torch.full((batch * count * (k * n + 1) * pw,), 0x5A, dtype=lwe_t.dtype, device="cuda")
    ws = torch.zeros(plan.pbs_workspace_bytes(L, k, gad[1], batch), dtype=torch.uint8, device="cuda") if with_ws else None
    plan.bootstrap_manylut_batch(out, lwe_t, lut_t, kr, L, k, gad[0], gad[1], t, count, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    return out


def three_steps(torch, plan, lwe_t, lut_t, kr, L, k, gad, t, count, batch, per_element):
    n, pw = plan.ntt_size(), 2 if plan.WORD == 16 else 1
    rot = torch.zeros(batch * (L + 1), dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_manylut_batch(rot, lwe_t, L, t)
    acc = torch.zeros(batch * (k + 1) * n * pw, dtype=lwe_t.dtype, device="cuda")
    plan.blind_rotate_batch(acc, lut_t, rot, kr, L, k, gad[0], gad[1], lut_per_element=per_element)
    out = torch.zeros(batch * count * (k * n + 1) * pw, dtype=lwe_t.dtype, device="cuda")
    plan.sample_extract_many_batch(out, acc, k, count)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bootstrap_manylut_equals_its_three_steps_and_bootstrap_batch_at_t_zero(kind):
    """n = 32, k = 1, L = 3, batch 3, t = 2, lut_count 1, 3, 4, shared and per-element tables, with and without a caller workspace; the
    host path once; at t = 0, lut_count = 1 the call is bootstrap_batch"""
    torch = _torch()
    assert len(KINDS) == 10
    n, k, L, batch, t = 32, 1, 3, 3, 2
    plan = KINDS[kind].try_new(n)
    gad = (wbits(plan) // 4, 2)
    pw = 2 if plan.WORD == 16 else 1
    rng = np.random.default_rng(seed("nml-boot", kind))
    lwe = random_words(rng, plan, batch * (L + 1))
    key = random_key_words(rng, plan, L * (k + 1) * gad[1] * (k + 1))
    kr = key_planes(torch, plan, key)
    lwe_t = dev(torch, lwe)
    for per_element in (False, True):
        lut = random_words(rng, plan, (batch if per_element else 1) * (k + 1) * n)
        lut_t = dev(torch, lut)
        for count in (1, 3, 4):
            want = three_steps(torch, plan, lwe_t, lut_t, kr, L, k, gad, t, count, batch, per_element)
            for with_ws in (False, True):
                got = run_boot(torch, plan, lwe_t, lut_t, kr, L, k, gad, t, count, batch, with_ws, per_element)
                assert want.any() and torch.equal(got, want), (kind, per_element, count, with_ws)
        hout = np.full(batch * 3 * (k * n + 1) * pw, 0x5A, dtype=plan.word_dtype)
        plan.bootstrap_manylut_batch(hout, lwe, lut, [host(p, plan.res_dtype).copy() for p in kr], L, k, gad[0], gad[1], t, 3,
                                     lut_per_element=per_element)
        want = three_steps(torch, plan, lwe_t, lut_t, kr, L, k, gad, t, 3, batch, per_element)
        assert np.array_equal(hout, host(want, plan.word_dtype)), (kind, per_element, "host")
        ref = torch.zeros(batch * (k * n + 1) * pw, dtype=lwe_t.dtype, device="cuda")
        plan.bootstrap_batch(ref, lwe_t, lut_t, kr, L, k, gad[0], gad[1], lut_per_element=per_element)
        torch.cuda.synchronize()
        assert torch.equal(run_boot(torch, plan, lwe_t, lut_t, kr, L, k, gad, 0, 1, batch, False, per_element), ref), (kind, per_element)


# -- 4. the one-rotation circuit bootstrap ---------------------------------------------------------------------------------------------------
def run_cbs(torch, plan, where, lwe, bsk_planes, fk, L, k, gad, t, with_ws=False, stream=None):
    """the call on word arrays (the bootstrapping key as device planes) -> the NPRIMES output planes as arrays, poisoned before"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // ((L + 1) * (2 if plan.WORD == 16 else 1))
    count = batch * sizes(k, n, kl, cl)[2] * n
    nws = plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pl, kl, cl, batch)
    if where == "host":
        outs = [np.full(count, 0x5A5A5A5A, dtype=plan.res_dtype) for _ in range(plan.NPRIMES)]
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.circuit_bootstrap_manylut_batch(outs, lwe, None if bsk_planes is None else [host(p, plan.res_dtype).copy() for p in bsk_planes], fk,
                                             L, k, pb, pl, kb, kl, cb, cl, t, workspace=ws)
        return outs
    outs = [torch.full((count,), 0x5A5A5A5A, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    lwe_t, fk_t = dev(torch, lwe), dev(torch, fk)
    torch.cuda.synchronize()
    if stream is None:
        plan.circuit_bootstrap_manylut_batch(outs, lwe_t, bsk_planes, fk_t, L, k, pb, pl, kb, kl, cb, cl, t, workspace=ws)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            plan.circuit_bootstrap_manylut_batch(outs, lwe_t, bsk_planes, fk_t, L, k, pb, pl, kb, kl, cb, cl, t, workspace=ws)
        stream.synchronize()
    return [host(o, plan.res_dtype) for o in outs]


def public_u(torch, plan, lwe, bsk_planes, L, k, gad, t):
    """steps 1 and 2 from public calls -- the coarse switch of lwe', blind_rotate_batch with the shared table, sample_extract_batch at
    l - 1, + H_l on the body: u[l - 1] = batch lists of Lin + 1 ints for l = 1 .. Lc"""
    pb, pl, kb, kl, cb, cl = gad
    n, w = plan.ntt_size(), wbits(plan)
    M, pw = 1 << w, 2 if plan.WORD == 16 else 1
    x = to_ints(plan, lwe)
    batch = len(x) // (L + 1)
    for b in range(batch):
        x[b * (L + 1) + L] = (x[b * (L + 1) + L] + (1 << (w - 2))) % M
    lwe1 = dev(torch, to_array(plan, x))
    rot = torch.zeros(batch * (L + 1), dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_manylut_batch(rot, lwe1, L, t)
    table = dev(torch, to_array(plan, [c for poly in cbs_table(w, k, n, cb, cl, t) for c in poly]))
    acc = torch.zeros(batch * (k + 1) * n * pw, dtype=lwe1.dtype, device="cuda")
    bsk_arg = bsk_planes if L else [torch.empty(0, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
    plan.blind_rotate_batch(acc, table, rot, bsk_arg, L, k, pb, pl, lut_per_element=False)
    us = []
    for l in range(1, cl + 1):
        u_t = torch.zeros(batch * (k * n + 1) * pw, dtype=lwe1.dtype, device="cuda")
        plan.sample_extract_batch(u_t, acc, k, l - 1)
        torch.cuda.synchronize()
        u = to_ints(plan, host(u_t, plan.word_dtype))
        rows = [u[b * (k * n + 1):(b + 1) * (k * n + 1)] for b in range(batch)]
        for r in rows:
            r[k * n] = (r[k * n] + H(w, cb, l)) % M
        us.append(rows)
    return us


def compose_cbs(torch, plan, lwe, bsk_planes, fk, L, k, gad, t):
    """the header's sequence of public calls, step 3 as pack_keyswitch_batch on (u, 0) with lwe_count = 1, step 4 as fwd_batch"""
    pb, pl, kb, kl, cb, cl = gad
    n, pe = plan.ntt_size(), per(plan)
    lin, R, selp, _ = sizes(k, n, kl, cl)
    us = public_u(torch, plan, lwe, bsk_planes, L, k, gad, t)
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


def gadgets(w):
    """(8, 3, 22, 2, 8, 3); on 32-bit words the keyswitch gadget (22, 2) would pass the word, there it is (11, 2)"""
    return (8, 3, 22 if w >= 64 else 11, 2, 8, 3)


@pytest.mark.parametrize("kind", NONBINARY)
def test_circuit_bootstrap_manylut_equals_the_public_call_sequence(kind):
    """n = 32, k = 1, L = 3, batch 3, t = 2, Lc = 3; k = 0 and k = 2 once each; with and without a caller workspace"""
    torch = _torch()
    n, L, batch, t = 32, 3, 3, 2
    plan = KINDS[kind].try_new(n)
    gad = gadgets(wbits(plan))
    rng = np.random.default_rng(seed("nml-cbs", kind))
    for k in (1,) + ((0, 2) if kind == "native64_plan32" else (0,) if kind == "native32_plan32" else (2,) if kind == "native128_plan32" else ()):
        assert (k + 1) * gad[1] <= plan.max_terms()
        lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
        want = compose_cbs(torch, plan, lwe, bsk_planes, fk, L, k, gad, t)
        for with_ws in (False, True):
            got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t, with_ws)
            assert all(g.any() for g in got) and same(got, want), (kind, k, with_ws, diff(got, want))


@pytest.mark.parametrize("kind", NONBINARY)
def test_circuit_bootstrap_manylut_at_t_zero_is_circuit_bootstrap_batch(kind):
    torch = _torch()
    n, k, L, batch = 32, 1, 3, 3
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    gad = (w // 4, 4, 11, 2, w - 1, 1)                                   # the PBS gadget keeps all bits of the constant -H_1 = -1
    rng = np.random.default_rng(seed("nml-t0", kind))
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    count = batch * sizes(k, n, gad[3], 1)[2] * n
    want = [torch.zeros(count, dtype=res_t(torch, plan), device="cuda") for _ in range(plan.NPRIMES)]
    plan.circuit_bootstrap_batch(want, dev(torch, lwe), bsk_planes, dev(torch, fk), L, k, *gad)
    torch.cuda.synchronize()
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, 0)
    assert all(g.any() for g in got) and same(got, [host(x, plan.res_dtype) for x in want]), kind


@pytest.mark.parametrize("kind", ["native64_plan32", "native32_plan32"])
def test_ragged_tile_and_a_second_trip_of_the_product_grid(kind):
    """Lc = 2, t = 1, batch 4098: E = 8196 elements are 1024 full tiles of 8 and one of 4; with one column block, k + 1 = 2 keys and one
    slab that is 2050 work items for a grid capped at 2048.  L = 1 keeps it in seconds.  The reference is the call on two halves for
    every word and the public-call sequence for the first and the last elements."""
    torch = _torch()
    n, k, L, batch, t = 32, 1, 1, 4098, 1
    plan = KINDS[kind].try_new(n)
    gad = (8, 3, 31, 1, 5, 2)
    lin, R, selp, fkp = sizes(k, n, 1, 2)
    cols, tiles, rows, slabs = shape(n, plan.WORD, k, R, batch * 2)
    items = (k + 1) * cols * tiles * slabs
    cap = cntt.lib().cntt_native_cbs_grid(1 << 30, 5, plan.WORD)
    assert cntt.lib().cntt_native_cbs_grid(items, 5, plan.WORD) == cap < items < 2 * cap and (batch * 2) % 8 == 4 and slabs == 1
    rng = np.random.default_rng(seed("nml-ragged", kind))
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t)
    half = 2048
    for lo, hi in ((0, half), (half, batch)):
        part = run_cbs(torch, plan, "device", lwe[lo * (L + 1):hi * (L + 1)], bsk_planes, fk, L, k, gad, t)
        assert same([g[lo * selp * n:hi * selp * n] for g in got], part), (kind, lo, hi)
    ends = np.concatenate([lwe[:2 * (L + 1)], lwe[-2 * (L + 1):]])
    want = compose_cbs(torch, plan, ends, bsk_planes, fk, L, k, gad, t)
    for g, x in zip(got, want):
        assert np.array_equal(np.concatenate([g[:2 * selp * n], g[-2 * selp * n:]]), x), kind
        assert g[-2 * selp * n:].any()


@pytest.mark.parametrize("kind", ["native64_plan32", "native128_plan32", "native32_plan52"])
def test_host_path_equals_device_path_and_lwe_dim_zero(kind):
    torch = _torch()
    n, k, batch, t = 32, 1, 3, 2
    plan = KINDS[kind].try_new(n)
    gad = gadgets(wbits(plan))
    rng = np.random.default_rng(seed("nml-host", kind))
    for L in (3, 0):                                                     # lwe_dim == 0: the set-up alone, no bootstrapping key
        lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
        want = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t)
        if L == 0:
            assert same(want, compose_cbs(torch, plan, lwe, None, fk, L, k, gad, t)), kind
        for with_ws in (True, False):
            got = run_cbs(torch, plan, "host", lwe, bsk_planes, fk, L, k, gad, t, with_ws)
            assert all(g.any() for g in got) and same(got, want), (kind, L, with_ws, diff(got, want))


def test_non_default_stream():
    torch = _torch()
    kind, n, k, L, batch, t = "native32_plan32", 32, 2, 3, 3, 2
    plan = KINDS[kind].try_new(n)
    gad = gadgets(32)
    rng = np.random.default_rng(30)
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    want = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t)
    got = run_cbs(torch, plan, "device", lwe, bsk_planes, fk, L, k, gad, t, stream=torch.cuda.Stream())
    assert same(got, want), diff(got, want)


def test_graph_capture_with_a_caller_workspace_after_one_eager_call():
    """native64 Plan32 at n = 1024, L = 4, batch 3, a shape the header declares capturable: one stream, a linear chain of kernels,
    captured once after one eager call and replayed twice on fresh inputs"""
    torch = _torch()
    n, k, L, batch, t = 1024, 1, 4, 3, 1
    gad = (8, 3, 22, 2, 8, 2)
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(30)
    lwe, bsk_planes, fk = random_case(torch, plan, rng, L, k, gad, batch)
    lwe_t, fk_t = dev(torch, lwe), dev(torch, fk)
    ws = torch.zeros(plan.circuit_bootstrap_manylut_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch), dtype=torch.uint8, device="cuda")
    count = batch * sizes(k, n, gad[3], gad[5])[2] * n
    outs = [torch.full((count,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.circuit_bootstrap_manylut_batch(outs, lwe_t, bsk_planes, fk_t, L, k, *gad, t, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.circuit_bootstrap_manylut_batch(outs, lwe_t, bsk_planes, fk_t, L, k, *gad, t, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, plan, batch * (L + 1)))
        eager = [torch.zeros_like(o) for o in outs]
        plan.circuit_bootstrap_manylut_batch(eager, fresh, bsk_planes, fk_t, L, k, *gad, t)
        lwe_t.copy_(fresh)
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(e.any() and torch.equal(o, e) for o, e in zip(outs, eager))


# -- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def many_f(h, m):
    """function h of a 3-bit message"""
    return (m * (2 * h + 1) + h) & 7


def test_many_lut_bootstrap_evaluates_every_table_on_every_message():
    """native64 Plan32, n = 128, k = 1, L = 2, t = 2, PBS gadget (16, 4) (nothing rounded), NOISE-FREE keys; a message m of 3 bits under
    one padding bit is encoded as m 2^60 and owns a box of n' / 8 = 4 coarse steps, the table shifted by half a box.  cntt_manylut.h: the
    exponent is off by at most D = (L + 1) / 2 + |e| 2n' / 2^w coarse steps; with every key bit set and an input noise |e| <= 2^50,
    D = 1.5 + 2^50 * 64 / 2^64 < 2 = half a box (checked below in plain ints), so every one of the 4 tables decodes on every message.
    With noise-free keys and a gadget that fills the word the outputs carry no error at all."""
    torch = _torch()
    w, n, k, L, t, pbs, in_noise = 64, 128, 1, 2, 2, (16, 4), 1 << 50
    M, nprime = 1 << w, n >> t
    box = nprime // 8
    assert box % 2 == 0 and 2 * ((L + 1) * M + 2 * in_noise * 2 * nprime) < 2 * box * M          # D < box / 2, times 2 * 2^w
    plan = KINDS["native64_plan32"].try_new(n)
    rng = random.Random(seed("nml-many"))
    S = [[rng.randrange(2) for _ in range(n)]]
    s_lwe = [1] * L                                                      # every switched word enters: the worst drift
    kr = key_planes(torch, plan, np.array(bsk(rng, w, s_lwe, S, n, *pbs), dtype=np.uint64))
    fs = []
    for h in range(1 << t):
        f = []
        for c in range(nprime):
            s = c + box // 2
            v = many_f(h, (s % nprime) // box) << (w - 4)
            f.append(v if s < nprime else (-v) % M)
        fs.append(f)
    lut = dev(torch, np.array([0] * (k * n) + interleave(fs, n, t), dtype=np.uint64))
    lwe = np.array([x for m in range(8) for x in lwe_encrypt(rng, w, s_lwe, m << (w - 4), noise=in_noise)], dtype=np.uint64)
    out = torch.zeros(8 * (1 << t) * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.bootstrap_manylut_batch(out, dev(torch, lwe), lut, kr, L, k, *pbs, t, 1 << t)
    torch.cuda.synchronize()
    rows = host(out, np.uint64).reshape(8 * (1 << t), n + 1)
    with np.errstate(over="ignore"):
        phase = rows[:, n] - (rows[:, :n] * np.array(S[0], dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    dec = [int(((int(x) >> (w - 5)) + 1) >> 1) & 15 for x in phase]
    want = [many_f(h, m) for m in range(8) for h in range(1 << t)]
    assert dec == want, [i for i, (x, y) in enumerate(zip(dec, want)) if x != y][:8]
    assert [int(x) for x in phase] == [v << (w - 4) for v in want]


def test_one_rotation_circuit_bootstrapped_address_bits_look_up_every_entry():
    """The lookup of tests/test_gpu_native_cbs.py::test_circuit_bootstrapped_address_bits_look_up_every_entry with its selectors produced
    by circuit_bootstrap_manylut_batch at t = 2: native64 Plan32, n = 32, k = 1, L = 4, noise-free keys and inputs, gadgets (16, 4),
    (22, 2), (8, 3).  The margin of cntt_manylut.h holds: D = (L + 1) / 2 = 2.5 < n / 2^(t + 1) = 4 coarse steps, so u[b][l] has the same
    exact phase 0 / G_l as there, and the bound derived there does not depend on t: 7 CMuxes of at most
    (k + 1) n Lc (B / 2) n (Lin + 1) 2^(s - 1) + (1 + k n) 2^(s' - 1) each, below 2^49 against half a step of 2^60."""
    torch = _torch()
    w, n, k, L, m, t = 64, 32, 1, 4, 4, 2
    logn, depth = 5, 2
    gad = (16, 4, 22, 2, 8, 3)
    pb, pl, kb, kl, cb, cl = gad
    assert 2 * (L + 1) < 4 * (n >> (t + 1)) and cl <= 1 << t <= n // 2
    plan = KINDS["native64_plan32"].try_new(n)
    rng = random.Random(seed("nml-e2e"))
    S = [[rng.randrange(2) for _ in range(n)]]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    bsk_planes = key_planes(torch, plan, np.array(bsk(rng, w, s_lwe, S, n, pb, pl), dtype=np.uint64))
    fk_t = dev(torch, np.array(fpksk(rng, w, S, n, kb, kl), dtype=np.uint64))
    lwe = np.array([x for bit in (0, 1) for x in lwe_encrypt(rng, w, s_lwe, bit << 63)], dtype=np.uint64)
    selp = sizes(k, n, kl, cl)[2] * n
    sels = [torch.zeros(2 * selp, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.circuit_bootstrap_manylut_batch(sels, dev(torch, lwe), bsk_planes, fk_t, L, k, *gad, t)

    def planes(bits):
        return [torch.cat([p[b * selp:(b + 1) * selp] for b in bits]) for p in sels]

    nrng = np.random.default_rng(seed("nml-e2e-table"))
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
    print("one-rotation circuit bootstrap + lookup M = %d: worst error 2^%.2f over %d addresses, derived bound 2^%.2f"
          % (m, np.log2(max(worst, 1)), m * n, np.log2(bound)))
    assert dec == want, [i for i, (x, y) in enumerate(zip(dec, want)) if x != y][:8]
    assert worst < bound


# -- 6. the C example -----------------------------------------------------------------------------------------------------------------------
def test_pbs_manylut_native_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pbs_manylut_native"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pbs_manylut_native")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
