"""The circuit bootstrap of the prime plans (include/cntt_prime_cbs.h) on the MI355X.  Bit-exact, no tolerance: the call against the
sequence of public calls of its convention (Lc bootstraps, (k + 1) Lc packing keyswitches at lwe_count = 1, fwd, normalize) for the primes
outside the strict range; its keyswitch half against the plain-int model for strict-range primes too; the wide accumulator at the edge
of its bound; a ragged E-tile and a second trip of the grid; the host path; both workspace modes; graph capture; a non-default stream.
The one functional test -- circuit-bootstrapped address bits drive cmux_tree_batch to every entry -- derives its bound in its docstring."""
import os
import random
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_prime_automorphism as tga
from prime_cbs_model import G, H, Q4, bsk, fpksk, lwe_encrypt, model_keyswitch_rows, selector_from_rows, shape
from prime_cmux_model import phase
from test_gpu_prime_pack import first_difference
from test_gpu_prime_pbs import (P31, PA30, PA62, PG64, PW31, PW63, P51, _torch, dev, dt, host, key_ntt, make_plan, min_n, random_words, seed)
from test_prime_pbs_model import P30, P32, P50, P62, P63, PM64, signed_digits, wbits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

poison = tga.poison
NONSTRICT = [P62, PM64, P50, PG64, P51, PA62, P30, P32, PA30]     # outside 2^62 <= p < 2^63 and 2^30 <= p < 2^31
STRICT_AND_EDGE = [P63, PW63, PA62, P31, PW31, PA30]                # PA62, PA30: just above 2^61 and 2^29


def sizes(k, n, Lk, Lc):
    """(Lin, R, polynomials of one selector, polynomials of fpksk)"""
    lin = k * n
    return lin, (lin + 1) * Lk, (k + 1) * Lc * (k + 1), (k + 1) * (lin + 1) * Lk * (k + 1)


def run_cbs(torch, plan, p, where, lwe, bsk_t, fk_t, L, k, gad, with_ws=False):
    """the call on word arrays (the keys as device tensors) -> the selectors, poisoned before"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    out = poison(p, batch * sizes(k, n, kl, cl)[2] * n)
    nws = plan.circuit_bootstrap_workspace_bytes(L, k, pl, kl, cl, batch)
    if where == "host":
        ws = np.zeros(nws, dtype=np.uint8) if with_ws else None
        plan.circuit_bootstrap_batch(out, lwe, None if bsk_t is None else host(bsk_t, dt(p)).copy(), host(fk_t, dt(p)).copy(), L, k, pb, pl, kb, kl,
                                     cb, cl, workspace=ws)
        return out
    out_t = dev(torch, out)
    ws = torch.zeros(nws, dtype=torch.uint8, device="cuda") if with_ws else None
    plan.circuit_bootstrap_batch(out_t, dev(torch, lwe), bsk_t, fk_t, L, k, pb, pl, kb, kl, cb, cl, workspace=ws)
    torch.cuda.synchronize()
    return host(out_t, dt(p))


def public_u(torch, plan, p, lwe, bsk_t, L, k, gad):
    """steps 1 and 2 from public calls: u[l - 1] = batch x (Lin + 1) words for l = 1 .. Lc"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    x = lwe.astype(object).reshape(batch, L + 1).copy()
    x[:, L] = (x[:, L] + Q4(p)) % p
    lwe1 = dev(torch, x.astype(dt(p)).reshape(-1))
    us = []
    for l in range(1, cl + 1):
        h = H(p, cb, l)
        lut = np.zeros((k + 1) * n, dtype=dt(p))
        lut[k * n:] = (p - h) % p
        u_t = dev(torch, np.zeros(batch * (k * n + 1), dtype=dt(p)))
        plan.bootstrap_batch(u_t, lwe1, dev(torch, lut), bsk_t, L, k, pb, pl)
        torch.cuda.synchronize()
        u = host(u_t, dt(p)).astype(object).reshape(batch, k * n + 1)
        u[:, k * n] = (u[:, k * n] + h) % p
        us.append(u.astype(dt(p)))
    return us


def compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad):
    """the header's sequence of public calls, step 3 as pack_keyswitch_batch on (u, 0) with lwe_count = 1, fwd_batch, normalize_batch"""
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    batch = lwe.size // (L + 1)
    lin, R, selp, _ = sizes(k, n, kl, cl)
    out = np.zeros((batch, (k + 1) * cl, (k + 1) * n), dtype=dt(p))
    for l, u in enumerate(public_u(torch, plan, p, lwe, bsk_t, L, k, gad)):
        ct = np.zeros((batch, lin + 2), dtype=dt(p))
        ct[:, :lin + 1] = u                                            # the whole of u is the mask, the body word is 0
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
    pb, pl, kb, kl, cb, cl = gad
    n = plan.ntt_size()
    lwe = random_words(rng, p, batch * (L + 1))
    bsk_t = key_ntt(torch, plan, random_words(rng, p, L * (k + 1) * pl * (k + 1) * n)) if L else None
    fk_t = dev(torch, random_words(rng, p, sizes(k, n, kl, cl)[3] * n))        # NTT-domain words as they are: equality needs no meaning
    return lwe, bsk_t, fk_t


def gadgets(p, Lk, Lc):
    """(pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels): the keyswitch gadget fills W when it can, and the
    PBS gadget keeps all but W mod 4 bits -- one that rounds the constants -H_l away leaves a CMux difference without digits, a blind
    rotation that never moves and a zero output for every bit 0"""
    W = wbits(p)
    return (W // 4, 4, min(31, W // Lk), Lk, W // 2 if Lc == 2 else 5, Lc)


# -- 1. against the public calls ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", NONSTRICT)
def test_equals_the_public_call_sequence(p):
    """n in {32, 64}, k in {1, 2}, L in {3, 5}, batch in {1, 3}, Lc in {1, 2}, Lk in {1, 3}; (L + 1) / 2 < n / 2, so the drift of the
    modulus switch cannot cross a quadrant; random canonical keys; with and without a caller workspace"""
    torch = _torch()
    rng = np.random.default_rng(seed("cbs", p))
    for n, k, L, batch, Lc, Lk in ((32, 1, 3, 1, 1, 1), (64, 2, 5, 3, 2, 3), (32, 2, 5, 3, 1, 3), (64, 1, 3, 3, 2, 1)):
        plan = make_plan(p, n)
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        want = compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad)
        for with_ws in (False, True):
            got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad, with_ws)
            assert got.any() and np.array_equal(got, want), (p, n, k, L, batch, gad, with_ws, first_difference(got, want))


def model_from_u(us, fk_words, p, k, n, kb, kl):
    """the selectors of the plain-int model from the u of every level: us[l - 1][b] -> batch selectors back to back"""
    batch = us[0].shape[0]
    out = []
    for b in range(batch):
        rows = [model_keyswitch_rows(u[b].tolist(), fk_words, p, k, n, kb, kl) for u in us]
        out += selector_from_rows(rows, k, n)
    return np.array(out, dtype=dt(p))


@pytest.mark.parametrize("p", STRICT_AND_EDGE)
def test_keyswitch_half_equals_the_model_for_strict_range_primes_too(p):
    """u from the public bootstrap (whose words the call has for every prime), step 3 from the plain-int model: exact mod p"""
    torch = _torch()
    rng = np.random.default_rng(seed("cbs-model", p))
    for n, k, L, batch, Lc, Lk in ((min_n(p), 1, 3, 3, 2, 3), (64, 2, 3, 1, 1, 1)):
        plan = make_plan(p, n)
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        us = public_u(torch, plan, p, lwe, bsk_t, L, k, gad)
        want = model_from_u(us, host(fk_t, dt(p)).tolist(), p, k, n, gad[2], gad[3])
        got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
        assert got.any() and np.array_equal(got, want), (p, n, k, gad, first_difference(got, want))


# -- 2. the accumulator at the edge of its bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [PM64, P32])
def test_accumulator_at_the_edge_of_its_bound(p):
    """Every mask word of u is (p - 1) / 2 or (p + 1) / 2, whose digit at ks_base_log = 31, one level, is the largest the prime allows of
    either sign (+-2^30 exactly for 2^64 - 2^32 + 1), and every key word is p - 1; R = 65 rows at n = 64, k = 1 make two slabs of 33 rows,
    the last one short; 11 elements are one full E-tile and a ragged one.  The words of u are forced through the inputs: L = 1 with
    ms(lwe[0]) = n makes the CMux difference of the set-up accumulator -2 acc, whose body is the constant -+G_1; the PBS gadget (W, 1)
    takes it as one digit, and the bootstrapping key row (body, level 1) -> mask is the constant c = (p - 1) / 2 * G_1^-1, so the mask of
    the accumulator is +-(p - 1) / 2."""
    torch = _torch()
    n, k, L, batch = 64, 1, 1, 11
    W = wbits(p)
    gad = (W, 1, 31, 1, 4, 1)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cbs-edge", p))
    lin, R, selp, fkp = sizes(k, n, 1, 1)
    cols, tiles, rows, slabs = shape(n, np.dtype(dt(p)).itemsize, k, R, batch)
    assert slabs == 2 and rows * slabs > R and batch % 8 and tiles == 2
    lwe = random_words(rng, p, batch * (L + 1)).reshape(batch, L + 1)
    lwe[:, 0] = (p + 1) // 2                                            # ms = n
    c = (p - 1) // 2 * pow(G(p, 4, 1), -1, p) % p
    key = np.zeros((4, n), dtype=dt(p))                                 # rows (q, l) x o = (0,1,0), (0,1,1), (1,1,0), (1,1,1)
    key[2, 0] = c
    key[3, 0] = 12345
    bsk_t = key_ntt(torch, plan, key.reshape(-1))
    fk_t = dev(torch, np.full(fkp * n, p - 1, dtype=dt(p)))
    us = public_u(torch, plan, p, lwe.reshape(-1), bsk_t, L, k, gad)
    mask = us[0][:, :lin].astype(object)
    assert set(np.unique(mask).tolist()) == {(p - 1) // 2, (p + 1) // 2}
    top = max(abs(signed_digits(x, p, 31, 1)[0]) for x in ((p - 1) // 2, (p + 1) // 2))
    assert top >= (1 << 30) - (1 << 18) and (p != PM64 or top == 1 << 30)
    assert {signed_digits(int(x), p, 31, 1)[0] for x in mask.reshape(-1)} == {top, -top}
    want = model_from_u(us, [p - 1] * (fkp * n), p, k, n, 31, 1)
    got = run_cbs(torch, plan, p, "device", lwe.reshape(-1), bsk_t, fk_t, L, k, gad)
    assert got.any() and np.array_equal(got, want), (p, first_difference(got, want))


# -- 3. a ragged E-tile and a second trip of the grid ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P30])
def test_ragged_tile_and_a_second_trip_of_the_grid(p):
    """8195 elements are 1024 full tiles and one of 3; with one column block and k + 1 = 2 keys that is 2050 work items for a grid capped
    at 2048: two workgroups make a second trip"""
    torch = _torch()
    n, k, L, batch = min_n(p), 1, 3, 8195
    gad = gadgets(p, 1, 1)
    w = np.dtype(dt(p)).itemsize
    cols, tiles, rows, slabs = shape(n, w, k, sizes(k, n, 1, 1)[1], batch)
    items = (k + 1) * cols * tiles * slabs
    cap = cntt.lib().cntt_prime_cbs_grid(1 << 30, n.bit_length() - 1, w)
    assert cntt.lib().cntt_prime_cbs_grid(items, n.bit_length() - 1, w) == cap < items < 2 * cap and batch % 8 == 3 and slabs == 1
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cbs-ragged", p))
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    want = compose_cbs(torch, plan, p, lwe, bsk_t, fk_t, L, k, gad)
    got = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
    assert np.array_equal(got, want), first_difference(got, want)
    tail = slice((batch - 3) * 4 * n, None)
    assert got[tail].any() and not np.array_equal(got[tail], poison(p, got[tail].size))


# -- 4. host path, workspace, graph capture, stream -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [P62, P32])
def test_host_path_equals_device_path(p):
    torch = _torch()
    n, k, batch = 32, 1, 3
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("cbs-host", p))
    for L, Lk, Lc in ((3, 3, 2), (0, 1, 1)):                             # lwe_dim == 0: the set-up alone, no bootstrapping key
        gad = gadgets(p, Lk, Lc)
        lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
        want = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
        for with_ws in (True, False):
            got = run_cbs(torch, plan, p, "host", lwe, bsk_t, fk_t, L, k, gad, with_ws)
            assert got.any() and np.array_equal(got, want), (p, L, with_ws, first_difference(got, want))


def test_graph_capture_with_a_caller_workspace_after_one_eager_call():
    """captured once, replayed twice on fresh inputs written into the captured buffer"""
    torch = _torch()
    p, n, k, L, batch = PM64, 1024, 1, 4, 3
    gad = (8, 3, 22, 2, 8, 2)
    plan = make_plan(p, n)
    rng = np.random.default_rng(29)
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    lwe_t = dev(torch, lwe)
    ws = torch.zeros(plan.circuit_bootstrap_workspace_bytes(L, k, gad[1], gad[3], gad[5], batch), dtype=torch.uint8, device="cuda")
    out = dev(torch, poison(p, batch * sizes(k, n, gad[3], gad[5])[2] * n))
    plan.circuit_bootstrap_batch(out, lwe_t, bsk_t, fk_t, L, k, *gad, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.circuit_bootstrap_batch(out, lwe_t, bsk_t, fk_t, L, k, *gad, workspace=ws)
    for _ in range(2):
        fresh = dev(torch, random_words(rng, p, batch * (L + 1)))
        eager = torch.zeros_like(out)
        plan.circuit_bootstrap_batch(eager, fresh, bsk_t, fk_t, L, k, *gad)
        lwe_t.copy_(fresh)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert eager.any() and torch.equal(out, eager)


def test_non_default_stream():
    torch = _torch()
    p, n, k, L, batch = P30, 64, 2, 3, 3
    gad = gadgets(p, 3, 2)
    plan = make_plan(p, n)
    rng = np.random.default_rng(31)
    lwe, bsk_t, fk_t = random_case(torch, plan, p, rng, L, k, gad, batch)
    want = run_cbs(torch, plan, p, "device", lwe, bsk_t, fk_t, L, k, gad)
    out = dev(torch, poison(p, want.size))
    lwe_t = dev(torch, lwe)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan.circuit_bootstrap_batch(out, lwe_t, bsk_t, fk_t, L, k, *gad)
    s.synchronize()
    assert np.array_equal(host(out, dt(p)), want)


# -- 5. end to end --------------------------------------------------------------------------------------------------------------------------
def test_circuit_bootstrapped_address_bits_select_every_entry():
    """PM64 (W = 64), n = 64, k = 1, L = 8, binary keys, every key row with a noise |e| < 2^4; PBS gadget (16, 4), keyswitch gadget
    (22, 2), selector gadget (8, 3); the 3 address bits of each of the 8 addresses are encrypted as bit (p + 1) / 2 + e, |e| < 2^40,
    circuit-bootstrapped in ONE call of 24 elements and fed to cmux_tree_batch at M = 8 over a table of 3-bit entries at steps of p / 8.
    Bound on the error of a selector row's phase, from the headers: the blind rotation leaves |err(u)| < L (k + 1) n levels (B / 2) 2^4 =
    8 * 2 * 64 * 4 * 2^15 * 2^4 = 2^31 (cntt_prime_pbs.h, nothing rounded at 16 * 4 = W); a row is M_q times that, M_q = -S_q binary:
    < n 2^31 = 2^37; the keyswitch rounding, s = 64 - 44 = 20, adds < n (Lin + 1) 2^19 < 2^32 and the key noise < R 2^21 2^4 < 2^33
    (cntt_prime_cbs.h).  Together a row is off by less than 2^38.  A CMux of the tree adds at most (k + 1) n levels (B / 2) 2^38 =
    2 * 64 * 3 * 2^7 * 2^38 < 2^54 and its own rounding (s = 40) n 2^39 = 2^45; three stages: below 2^56, asserted, against half a
    step of 2^60.  The worst error seen is printed beside it."""
    torch = _torch()
    p, n, k, L = PM64, 64, 1, 8
    gad = (16, 4, 22, 2, 8, 3)
    pb, pl, kb, kl, cb, cl = gad
    plan = make_plan(p, n)
    rng = random.Random(seed("cbs-e2e"))
    S = [[rng.randrange(2) for _ in range(n)]]
    s_lwe = [rng.randrange(2) for _ in range(L)]
    bsk_t = key_ntt(torch, plan, np.array(bsk(rng, p, s_lwe, S, n, pb, pl, noise=15), dtype=np.uint64))
    fk_t = key_ntt(torch, plan, np.array(fpksk(rng, p, S, n, kb, kl, noise=15), dtype=np.uint64))
    lwe = np.array([w for a in range(8) for i in range(3) for w in lwe_encrypt(rng, p, s_lwe, ((a >> i) & 1) * ((p + 1) // 2), noise=1 << 40)],
                   dtype=np.uint64)
    selp = sizes(k, n, kl, cl)[2] * n
    sels = dev(torch, np.zeros(24 * selp, dtype=np.uint64))
    plan.circuit_bootstrap_batch(sels, dev(torch, lwe), bsk_t, fk_t, L, k, *gad)
    nrng = np.random.default_rng(seed("cbs-e2e-table"))
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
        err = [(x - int(y) * (p // 8)) % p for x, y in zip(ph, entries[a])]
        worst = max(worst, max(min(e, p - e) for e in err))
    print("circuit bootstrap + tree at M = 8: worst error 2^%.2f against the bound 2^56" % np.log2(max(worst, 1)))
    assert worst < 1 << 56


# -- 6. the C example -----------------------------------------------------------------------------------------------------------------------
def test_cbs_lookup_prime_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "cbs_lookup_prime"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "cbs_lookup_prime")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "every looked-up entry decoded" in r.stdout, r.stdout
