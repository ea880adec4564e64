"""The many-LUT bootstrap and the one-rotation circuit bootstrap of the prime plans (include/cntt_prime_manylut.h) on the MI355X.
Bit-exact, no tolerance: the coarse modulus switch and the extraction of several indices against the plain-int model
(tests/prime_manylut_model.py) and the extraction against single sample_extract_batch calls; bootstrap_manylut_batch against its three
steps, against the model, and at t = 0 against bootstrap_batch; circuit_bootstrap_manylut_batch against the sequence of public calls of
its convention, its keyswitch half against the model for strict-range primes too, and at t = 0, Lc = 1 against circuit_bootstrap_batch;
the host path, both workspace modes, a non-default stream, graph capture.  The two functional tests decode under noisy keys and assert the
bounds derived in the header."""
import os
import random
import subprocess

import numpy as np
import pytest

import test_gpu_prime_cbs as tcb
from prime_cbs_model import H, Q4, bsk, flatten, fpksk, lwe_encrypt, lwe_phase
from prime_cmux_model import phase
from prime_manylut_model import model_bootstrap_manylut, model_extract_many, model_modswitch_coarse
from test_gpu_prime_pack import first_difference
from test_gpu_prime_pbs import ALL, _torch, dev, dt, host, key_ntt, make_plan, min_n, random_words, seed, zeros
from test_prime_manylut_model import MANY, many_bound, many_enc, many_f, many_table
from test_prime_pbs_model import P30, P32, P62, PM64, modswitch_words, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
poison = tcb.poison
COUNTS = (1, 2, 7, 8, 9)          # the edges of the 8-row chunk; n itself is added per case


# -- 1. the coarse modulus switch and the extraction of several indices against the model ----------------------------------------------------
@pytest.mark.parametrize("p", ALL)
def test_coarse_modswitch_matches_model(p):
    """every t at n = min_n(p) and 64, L in {0, 5}, batch in {1, 3, 9} and 33 x 33 words beyond one tile; words on both sides of the
    boundaries of the grid"""
    torch = _torch()
    for n in (min_n(p), 64):
        logn = n.bit_length() - 1
        plan = make_plan(p, n)
        rng = np.random.default_rng(seed("ml-ms", p, n))
        for t in range(logn + 1):
            special = modswitch_words(p, logn - t, rng) if t < logn else [0, 1, p - 1, (p + 1) // 2, (p - 1) // 2, p // 4, p // 4 + 1]
            for L, batch in ((0, 1), (5, 3), (5, 9), (32, 33)) if t in (0, 2, logn) else ((5, 3),):
                count = batch * (L + 1)
                words = [special[(i // 2 + L) % len(special)] if i % 2 == 0 else int(rng.integers(0, p, dtype=np.uint64)) for i in range(count)]
                rot_t = torch.full((count,), -1, dtype=torch.int32, device="cuda")
                plan.lwe_modswitch_manylut_batch(rot_t, dev(torch, np.array(words, dtype=dt(p))), L, t)
                torch.cuda.synchronize()
                assert [int(x) for x in host(rot_t, np.uint32)] == model_modswitch_coarse(words, L, batch, p, logn, t), (p, n, t, L, batch)


def single_extractions(torch, plan, p, glwe_t, k, count, batch):
    """count calls of sample_extract_batch, interleaved into the layout batch x count x (k n + 1)"""
    n = plan.ntt_size()
    out = np.zeros((batch, count, k * n + 1), dtype=dt(p))
    for h in range(count):
        one = zeros(torch, p, batch * (k * n + 1))
        plan.sample_extract_batch(one, glwe_t, k, h)
        torch.cuda.synchronize()
        out[:, h] = host(one, dt(p)).reshape(batch, k * n + 1)
    return out.reshape(-1)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", ALL)
def test_sample_extract_many_matches_model_and_single_extractions(p, where):
    """count in {1, 2, 7, 8, 9, n}: one row, a ragged chunk, a full chunk, a second chunk, and the wrap in every row; k in {0, 1, 2}"""
    torch = _torch()
    rng = np.random.default_rng(seed("ml-ext", p, where))
    for n, k, batch in ((min_n(p), 1, 3), (64, 2, 1), (min_n(p), 0, 9), (64, 1, 9)):
        plan = make_plan(p, n)
        glwe = random_words(rng, p, batch * (k + 1) * n)
        glwe[0], glwe[n - 1], glwe[1] = 0, p - 1, 1
        g = [int(x) for x in glwe]
        for count in COUNTS + (n,):
            if where == "host":
                out = poison(p, batch * count * (k * n + 1))
                plan.sample_extract_many_batch(out, glwe.copy(), k, count)
                got = out
            else:
                out = dev(torch, poison(p, batch * count * (k * n + 1)))
                plan.sample_extract_many_batch(out, dev(torch, glwe), k, count)
                torch.cuda.synchronize()
                got = host(out, dt(p))
            want = []
            for b in range(batch):
                base = b * (k + 1) * n
                want += model_extract_many([g[base + q * n:base + (q + 1) * n] for q in range(k + 1)], count, p)
            assert [int(x) for x in got] == want, (p, n, k, batch, count, where)
            if where == "device" and count in (9, n):
                assert np.array_equal(got, single_extractions(torch, plan, p, dev(torch, glwe), k, count, batch)), (p, n, k, count)


@pytest.mark.parametrize("p", [P62, P30])
def test_sample_extract_many_wide_window(p):
    """n = 2048 once: 512 (64-bit words) or 1024 (32-bit words) windows per row, count = 9 and n, against single extractions"""
    torch = _torch()
    n, k, batch = 2048, 1, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ml-wide", p))
    glwe_t = dev(torch, random_words(rng, p, batch * (k + 1) * n))
    for count in (9, n):
        out = dev(torch, poison(p, batch * count * (k * n + 1)))
        plan.sample_extract_many_batch(out, glwe_t, k, count)
        torch.cuda.synchronize()
        got, want = host(out, dt(p)), single_extractions(torch, plan, p, glwe_t, k, count, batch) if count == 9 else None
        if count == 9:
            assert np.array_equal(got, want), first_difference(got, want)
        else:                                                                    # every row h against the single extraction, 64 sampled rows
            rows = got.reshape(batch, count, k * n + 1)
            for h in sorted({0, 1, 7, 8, n - 1} | {int(x) for x in rng.integers(0, n, size=59)}):
                one = zeros(torch, p, batch * (k * n + 1))
                plan.sample_extract_batch(one, glwe_t, k, h)
                torch.cuda.synchronize()
                assert np.array_equal(rows[:, h], host(one, dt(p)).reshape(batch, k * n + 1)), (p, h)


# -- 2. the many-LUT bootstrap against its three steps, the model and bootstrap_batch ------------------------------------------------------
def run_boot(torch, plan, p, where, lwe, lut, bsk_t, L, k, gad, t, count, with_ws=False, per_element=None):
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    out = poison(p, batch * count * (k * n + 1))
    nws = plan.pbs_workspace_bytes(L, k, gad[1], batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.bootstrap_manylut_batch(out, lwe, lut, host(bsk_t, dt(p)).copy(), L, k, *gad, t, count, workspace=ws, lut_per_element=per_element)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.bootstrap_manylut_batch(out_t, dev(torch, lwe), dev(torch, lut), bsk_t, L, k, *gad, t, count, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def three_steps(torch, plan, p, lwe, lut, bsk_t, L, k, gad, t, count):
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    rot_t = torch.zeros((L + 1) * batch, dtype=torch.int32, device="cuda")
    acc = zeros(torch, p, batch * (k + 1) * n)
    out = zeros(torch, p, batch * count * (k * n + 1))
    plan.lwe_modswitch_manylut_batch(rot_t, dev(torch, lwe), L, t)
    plan.blind_rotate_batch(acc, dev(torch, lut), rot_t, bsk_t, L, k, *gad)
    plan.sample_extract_many_batch(out, acc, k, count)
    torch.cuda.synchronize()
    return host(out, dt(p))


@pytest.mark.parametrize("p", ALL)
def test_bootstrap_manylut_equals_its_three_steps(p):
    """k in {0, 1, 2}, L in {0, 3, 5}, batch in {1, 3, 9}, a shared and a per-element table, with and without a caller workspace; on the
    primes outside the strict range also against the big-integer model (n <= 32, batch 1 and 3)"""
    torch = _torch()
    rng = np.random.default_rng(seed("ml-boot", p))
    W = wbits(p)
    gad = (W // 4, 4)
    for n, k, L, batch, t, count, per_element in ((min_n(p), 1, 3, 3, 2, 3, False), (64, 2, 5, 9, 3, 8, True), (min_n(p), 0, 3, 1, 1, 2, False),
                                                  (64, 1, 0, 3, 6, 9, False)):
        plan = make_plan(p, n)
        lwe = random_words(rng, p, batch * (L + 1))
        lut = random_words(rng, p, (batch if per_element else 1) * (k + 1) * n)
        key = random_words(rng, p, L * (k + 1) * gad[1] * (k + 1) * n)          # coefficient domain: what the model takes
        bsk_t = key_ntt(torch, plan, key)
        want = three_steps(torch, plan, p, lwe, lut, bsk_t, L, k, gad, t, count)
        for with_ws in (False, True):
            got = run_boot(torch, plan, p, "device", lwe, lut, bsk_t, L, k, gad, t, count, with_ws, per_element)
            assert got.any() and np.array_equal(got, want), (p, n, k, L, batch, t, count, with_ws, first_difference(got, want))
        if p in tcb.NONSTRICT and n <= 32 and not per_element:
            rows = [int(x) for x in key]
            lut_p = [[int(x) for x in lut[q * n:(q + 1) * n]] for q in range(k + 1)]
            for b in range(batch):
                model = model_bootstrap_manylut([int(x) for x in lwe[b * (L + 1):(b + 1) * (L + 1)]], lut_p, rows, p, L, k, n, *gad, t, count)
                per = count * (k * n + 1)
                assert [int(x) for x in want[b * per:(b + 1) * per]] == model, (p, n, k, "element", b)


@pytest.mark.parametrize("p", [P62, PM64, P30, P32])
def test_bootstrap_manylut_at_t_zero_is_bootstrap_batch(p):
    torch = _torch()
    rng = np.random.default_rng(seed("ml-boot0", p))
    n, k, L, batch, gad = 64, 1, 4, 5, (7, 3)
    plan = make_plan(p, n)
    lwe, lut = random_words(rng, p, batch * (L + 1)), random_words(rng, p, (k + 1) * n)
    bsk_t = dev(torch, random_words(rng, p, L * (k + 1) * gad[1] * (k + 1) * n))
    want = zeros(torch, p, batch * (k * n + 1))
    plan.bootstrap_batch(want, dev(torch, lwe), dev(torch, lut), bsk_t, L, k, *gad)
    torch.cuda.synchronize()
    got = run_boot(torch, plan, p, "device", lwe, lut, bsk_t, L, k, gad, 0, 1)
    assert got.any() and np.array_equal(got, host(want, dt(p)))


# -- 3. the one-rotation circuit bootstrap against the public calls ---------------------------------------------------------------------------
def run_cbs(torch, plan, p, where, lwe, bsk_t, fk_t, L, k, gad, t, with_ws=False):
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    out = poison(p, batch * tcb.sizes(k, n, kl, cl)[2] * n)
    nws = plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pl, kl, cl, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.circuit_bootstrap_manylut_batch(out, lwe, None if bsk_t is None else host(bsk_t, dt(p)).copy(), host(fk_t, dt(p)).copy(), L, k, *gad, t,
                                             workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.circuit_bootstrap_manylut_batch(out_t, dev(torch, lwe), bsk_t, fk_t, L, k, *gad, t, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def public_u(torch, plan, p, lwe, bsk_t, L, k, gad, t):
    """steps 1 and 2 from public calls: ONE bootstrap_manylut_batch on the shared table, then + H_l: u[l - 1] = batch x (Lin + 1) words"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    x = lwe.astype(object).reshape(batch, L + 1).copy()
    x[:, L] = (x[:, L] + Q4(p)) % p
    lut = np.zeros((k + 1) * n, dtype=dt(p))
    for c in range(n):
        h = c & ((1 << t) - 1)
        lut[k * n + c] = (p - H(p, cb, h + 1)) % p if h < cl else 0
    empty = zeros(torch, p, 0)
    rows = zeros(torch, p, batch * cl * (k * n + 1))
    plan.bootstrap_manylut_batch(rows, dev(torch, x.astype(dt(p)).reshape(-1)), dev(torch, lut), empty if bsk_t is None else bsk_t, L, k, pb, pl, t, cl)
    torch.cuda.synchronize()
    u = host(rows, dt(p)).astype(object).reshape(batch, cl, k * n + 1)
    us = []
    for l in range(1, cl + 1):
        ul = u[:, l - 1].copy()
        ul[:, k * n] = (ul[:, k * n] + H(p, cb, l)) % p
        us.append(ul.astype(dt(p)))
    return us


def compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad, t):
    """the header's sequence: bootstrap_manylut_batch, + H_l, pack_keyswitch_batch on (u, 0) with lwe_count = 1, fwd_batch, normalize_batch"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    lin, R, selp, _ = tcb.sizes(k, n, kl, cl)
    out = np.zeros((batch, (k + 1) * cl, (k + 1) * n), dtype=dt(p))
    for l, u in enumerate(public_u(torch, plan, p, lwe, bsk_t, L, k, gad, t)):
        ct = np.zeros((batch, lin + 2), dtype=dt(p))
        ct[:, :lin + 1] = u
        ct_t = dev(torch, ct.reshape(-1))
        for q in range(k + 1):
            g = dev(torch, np.zeros(batch * (k + 1) * n, dtype=dt(p)))
            plan.pack_keyswitch_batch(g, ct_t, fk_t[q * R * (k + 1) * n:(q + 1) * R * (k + 1) * n], lin + 1, 1, k, kb, kl)
            plan.fwd_batch(g)
            plan.normalize_batch(g)
            torch.cuda.synchronize()
            out[:, q * cl + l] = host(g, dt(p)).reshape(batch, (k + 1) * n)
    return out.reshape(-1)


def random_case(torch, plan, p, rng, L, k, gad, batch):
    """tcb.random_case; without mask words the phase is the body itself, u is exactly 0 or G_l, and a batch whose bits all read 0 would
    give an all-zero output: the first body is put at p / 2, which reads 1"""
    lwe, bsk_t, fk_t = tcb.random_case(torch, plan, p, rng, L, k, gad, batch)
    if L == 0:
        lwe[0] = p // 2
    return lwe, bsk_t, fk_t


def gadgets(p, Lk, Lc):
    """tcb.gadgets with a selector gadget of Lc levels for every Lc"""
    W = wbits(p)
    return (W // 4, 4, min(31, W // Lk), Lk, min(5, W // Lc), Lc)


@pytest.mark.parametrize("p", tcb.NONSTRICT)
def test_circuit_bootstrap_manylut_equals_the_public_call_sequence(p):
    """nine primes; n in {min_n, 64}, k in {1, 2}, L in {0, 3, 5}, batch in {1, 3, 9}, Lc in {1, 2, 3, 4} with 2^t = Lc rounded up and one
    t above it; with and without a caller workspace (k = 0: against the model, below)"""
    torch = _torch()
    rng = np.random.default_rng(seed("ml-cbs", p))
    for n, k, L, batch, Lc, Lk, t in ((min_n(p), 1, 3, 3, 3, 1, 2), (64, 2, 5, 1, 4, 3, 2), (min_n(p), 1, 3, 9, 2, 3, 3), (64, 1, 0, 3, 1, 1, 0)):
        plan = make_plan(p, n)
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        want = compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad, t)
        for with_ws in (False, True):
            got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t, with_ws)
            assert got.any() and np.array_equal(got, want), (p, n, k, L, batch, gad, t, with_ws, first_difference(got, want))


@pytest.mark.parametrize("p", tcb.STRICT_AND_EDGE)
def test_keyswitch_half_equals_the_model_for_strict_range_primes_too(p):
    """u from the public many-LUT bootstrap (whose words the call has for every prime), step 3 from the plain-int model: exact mod p"""
    torch = _torch()
    rng = np.random.default_rng(seed("ml-cbs-model", p))
    for n, k, L, batch, Lc, Lk, t in ((min_n(p), 1, 3, 3, 3, 3, 2), (64, 2, 3, 1, 2, 1, 1), (min_n(p), 0, 3, 9, 4, 3, 2)):
        plan = make_plan(p, n)
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        us = public_u(torch, plan, p, lwe, bsk_t, L, k, gad, t)
        want = tcb.model_from_u(us, host(fk_t, dt(p)).tolist(), p, k, n, gad[2], gad[3])
        got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t)
        assert got.any() and np.array_equal(got, want), (p, n, k, gad, first_difference(got, want))


@pytest.mark.parametrize("p", [P62, PM64, P30, P32])
def test_circuit_bootstrap_manylut_at_t_zero_is_circuit_bootstrap_batch(p):
    torch = _torch()
    rng = np.random.default_rng(seed("ml-cbs0", p))
    n, k, L, batch = 32, 1, 3, 3
    plan = make_plan(p, n)
    gad = gadgets(p, 3, 1)
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    want = tcb.run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
    got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, 0)
    assert got.any() and np.array_equal(got, want), first_difference(got, want)


@pytest.mark.parametrize("p", [P62, P30])
def test_a_batch_beyond_one_trip_of_the_keyswitch_grid(p):
    """2049 bits x 4 levels are 8196 elements: 1024 full tiles and one of 4, with k + 1 = 2 keys 2050 work items for a grid capped at
    2048; the one-rotation call against circuit_bootstrap_batch's own rotation is not available (other tables), so against the public
    sequence"""
    torch = _torch()
    n, k, L, batch, Lc, t = min_n(p), 1, 3, 2049, 4, 2
    gad = gadgets(p, 1, Lc)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ml-cbs-trip", p))
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    want = compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad, t)
    got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t)
    assert np.array_equal(got, want), first_difference(got, want)
    assert got[-4 * Lc * n:].any()


# -- 4. host path, stream, graph capture -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P32])
def test_host_paths_equal_device_paths(p):
    torch = _torch()
    n, k, batch, t = 32, 1, 3, 2
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("ml-host", p))
    for L, Lk, Lc in ((3, 3, 3), (0, 1, 2)):
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        want = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t)
        lut = random_words(rng, p, (k + 1) * n)
        key = bsk_t if L else zeros(torch, p, 0)
        want_b = run_boot(torch, plan, p, "device", lwe, lut, key, L, k, gad[:2], t, 3)
        for with_ws in (True, False):
            got = run_cbs(torch, plan, p, "host", lwe, bsk_t, fk_t, L, k, gad, t, with_ws)
            assert got.any() and np.array_equal(got, want), (p, L, with_ws, first_difference(got, want))
            got_b = run_boot(torch, plan, p, "host", lwe, lut, key, L, k, gad[:2], t, 3, with_ws)
            assert got_b.any() and np.array_equal(got_b, want_b), (p, L, with_ws)


def test_graph_capture_with_a_caller_workspace_after_one_eager_call():
    """both calls captured into one graph, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    p, n, k, L, batch, t, count = PM64, 1024, 1, 4, 3, 2, 3
    gad = (8, 3, 22, 2, 8, 3)
    plan = make_plan(p, n)
    rng = np.random.default_rng(29)
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    lwe_t, lut_t = dev(torch, lwe), dev(torch, random_words(rng, p, (k + 1) * n))
    ws = torch.zeros(plan.circuit_bootstrap_manylut_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch), dtype=torch.uint8, device="cuda")
    pws = torch.zeros(plan.pbs_workspace_bytes(L, k, gad[1], batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(p, batch * tcb.sizes(k, n, gad[3], gad[5])[2] * n))
    rows = dev(torch, poison(p, batch * count * (k * n + 1)))

    def both(o, r, x, w, pw):
        plan.circuit_bootstrap_manylut_batch(o, x, bsk_t, fk_t, L, k, *gad, t, workspace=w)
        plan.bootstrap_manylut_batch(r, x, lut_t, bsk_t, L, k, gad[0], gad[1], t, count, workspace=pw)

    both(out, rows, lwe_t, ws, pws)                                            # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        both(out, rows, lwe_t, ws, pws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, p, batch * (L + 1)))
        eager, eager_rows = torch.zeros_like(out), torch.zeros_like(rows)
        both(eager, eager_rows, fresh, None, None)
        lwe_t.copy_(fresh)
        out.zero_()
        rows.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager) and eager_rows.any() and torch.equal(rows, eager_rows)


def test_non_default_stream():
    torch = _torch()
    p, n, k, L, batch, t = P30, 64, 2, 3, 3, 2
    gad = gadgets(p, 3, 3)
    plan = make_plan(p, n)
    rng = np.random.default_rng(31)
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    lut = random_words(rng, p, (k + 1) * n)
    want = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, t)
    want_b = run_boot(torch, plan, p, "device", lwe, lut, bsk_t, L, k, gad[:2], t, 4)
    out, rows = dev(torch, poison(p, want.size)), dev(torch, poison(p, want_b.size))
    lwe_t, lut_t = dev(torch, lwe), dev(torch, lut)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.circuit_bootstrap_manylut_batch(out, lwe_t, bsk_t, fk_t, L, k, *gad, t)
        plan.bootstrap_manylut_batch(rows, lwe_t, lut_t, bsk_t, L, k, gad[0], gad[1], t, 4)
    s.synchronize()
    assert np.array_equal(host(out, dt(p)), want) and np.array_equal(host(rows, dt(p)), want_b)


# -- 5. decoding under noisy keys ----------------------------------------------------------------------------------------------------------------
def test_many_lut_bootstrap_evaluates_every_table_on_every_message():
    """The shape tests/test_prime_manylut_model.py decodes on the model alone: 2^64 - 2^32 + 1, n = 128, k = 1, L = 2, PBS gadget (32, 2),
    t = 2: four tables on the eight messages of a 3-bit space under one padding bit, binary keys, every key row with a noise |e| < 2^4,
    input noise below 2^20.  Selection (cntt_prime_manylut.h): the switch drifts by less than (L + 1) / 2 = 1.5 coarse steps and the
    noise and the encoding by less than 2^-30 more, against half a box of n' / 16 = 2.  Error: below L (k + 1) n levels (B / 2) 2^4 = 2^45,
    asserted, against half a step of 2^59.  The worst error seen is printed beside it."""
    torch = _torch()
    p, n, k, L, pbs, t = (MANY[x] for x in ("p", "n", "k", "L", "pbs", "t"))
    plan = make_plan(p, n)
    rng = random.Random(seed("ml-e2e"))
    S = [[rng.randrange(2) for _ in range(n)] for _ in range(k)]
    s_lwe = [1] * L
    bsk_t = key_ntt(torch, plan, np.array(bsk(rng, p, s_lwe, S, n, *pbs, noise=MANY["key_noise"]), dtype=np.uint64))
    lut = np.array([w for poly in many_table(p, k, n, t) for w in poly], dtype=np.uint64)
    lwe = np.array([w for m in range(8) for w in lwe_encrypt(rng, p, s_lwe, many_enc(m, p), noise=MANY["in_noise"])], dtype=np.uint64)
    rows = run_boot(torch, plan, p, "device", lwe, lut, bsk_t, L, k, pbs, t, 1 << t).reshape(8, 1 << t, k * n + 1)
    s_in = flatten(S)
    worst = 0
    for m in range(8):
        for h in range(1 << t):
            ph = lwe_phase(rows[m, h].tolist(), s_in, p)
            assert ((32 * ph + p) // (2 * p)) % 16 == many_f(h, m), (m, h)
            e = (ph - many_enc(many_f(h, m), p)) % p
            worst = max(worst, min(e, p - e))
    print("many-LUT bootstrap, 4 tables x 8 messages: worst error 2^%.2f against the bound 2^45" % np.log2(max(worst, 1)))
    assert worst < many_bound(n, k, L, pbs) == 1 << 45


def test_one_rotation_circuit_bootstrapped_address_bits_select_every_entry():
    """The test of tests/test_gpu_prime_cbs.py through the one-rotation call: PM64, n = 64, k = 1, L = 8, binary keys, every key row with
    a noise |e| < 2^4; PBS gadget (16, 4), keyswitch gadget (22, 2), selector gadget (8, 3), t = 2; the 3 address bits of each of the 8
    addresses are encrypted as bit (p + 1) / 2 + e, |e| < 2^40, circuit-bootstrapped in ONE call of 24 elements (24 rotations, not 72) and
    fed to cmux_tree_batch at M = 8.  Selection (cntt_prime_manylut.h): (L + 1) / 2 + (2^40 + 1) 2n' / p < 4.6 coarse steps against the
    margin n / 2^(t + 1) = 8.  Error: the rotation's algebra does not depend on t, so the bound of cntt_prime_cbs.h holds as derived in
    tests/test_gpu_prime_cbs.py: a selector row is off by less than 2^38 and the tree's output by less than 2^56, asserted, against half
    a step of 2^60.  The worst error seen is printed beside it."""
    torch = _torch()
    p, n, k, L, t = PM64, 64, 1, 8, 2
    gad = (16, 4, 22, 2, 8, 3)
    pb, pl, kb, kl, cb, cl = gad
    plan = make_plan(p, n)
    rng = random.Random(seed("ml-cbs-e2e"))
    S = [[rng.randrange(2) for _ in range(n)]]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    bsk_t = key_ntt(torch, plan, np.array(bsk(rng, p, s_lwe, S, n, pb, pl, noise=15), dtype=np.uint64))
    fk_t = key_ntt(torch, plan, np.array(fpksk(rng, p, S, n, kb, kl, noise=15), dtype=np.uint64))
    lwe = np.array([w for a in range(8) for i in range(3) for w in lwe_encrypt(rng, p, s_lwe, ((a >> i) & 1) * ((p + 1) // 2), noise=1 << 40)],
                   dtype=np.uint64)
    selp = tcb.sizes(k, n, kl, cl)[2] * n
    sels = dev(torch, np.zeros(24 * selp, dtype=np.uint64))
    plan.circuit_bootstrap_manylut_batch(sels, dev(torch, lwe), bsk_t, fk_t, L, k, *gad, t)
    nrng = np.random.default_rng(seed("ml-cbs-e2e-table"))
    entries = nrng.integers(0, 8, size=(8, n))
    table = dev(torch, (entries.astype(object) * (p // 8)).astype(np.uint64).reshape(-1))
    worst = 0
    for a in range(8):
        out = dev(torch, np.zeros((k + 1) * n, dtype=np.uint64))
        plan.cmux_tree_batch(out, table, sels[a * 3 * selp:(a + 1) * 3 * selp], 8, k, cb, cl)
        torch.cuda.synchronize()
        ph = phase(host(out, np.uint64).tolist(), S, p)
        dec = [int((8 * x + p // 2) // p) % 8 for x in ph]
        assert dec == entries[a].tolist(), (a, dec, entries[a].tolist())
        e = [(x - int(y) * (p // 8)) % p for x, y in zip(ph, entries[a])]
        worst = max(worst, max(min(v, p - v) for v in e))
    print("one-rotation circuit bootstrap + tree at M = 8: worst error 2^%.2f against the bound 2^56" % np.log2(max(worst, 1)))
    assert worst < 1 << 56


# -- 6. the C example ---------------------------------------------------------------------------------------------------------------------------
def test_pbs_manylut_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pbs_manylut_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pbs_manylut_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 8 and not any("WRONG" in ln for ln in lines), r.stdout
