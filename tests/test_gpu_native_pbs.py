"""The programmable bootstrap of the native plans (include/cntt_pbs.h) on the MI355X.  Bit-exact: the modulus switch and the sample
extraction against a plain-int model; cntt_native_blind_rotate_batch against the per-iteration public calls it replaces (decompose +
external product accumulating in place, and the two-buffer external_product_decomposed_batch loop) and against the big-integer model
with the oracle's negacyclic_polymul; cntt_native_bootstrap_batch against its three steps; graph capture; the C example.  The one
check with a tolerance is the functional test, whose bound is derived in its docstring."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import (native32, native64, native128, native_binary32, native_binary64, native_binary128)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"native32_plan32": native32.Plan32, "native64_plan32": native64.Plan32, "native128_plan32": native128.Plan32,
         "native_binary32_plan32": native_binary32.Plan32, "native_binary64_plan32": native_binary64.Plan32,
         "native_binary128_plan32": native_binary128.Plan32, "native32_plan52": native32.Plan52,
         "native64_plan52": native64.Plan52, "native_binary32_plan52": native_binary32.Plan52,
         "native_binary64_plan52": native_binary64.Plan52}
FUSED = ["native32_plan32", "native64_plan32", "native_binary32_plan32", "native_binary64_plan32"]
WORDS = {32: native32.Plan32, 64: native64.Plan32, 128: native128.Plan32}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# -- the model: plain Python ints (source / digits / model_terms as in tests/test_gpu_native_gadget.py) ---------------------------------
def source(f, a, w, mode):
    n, M = len(f), 1 << w
    if mode == "plain":
        return list(f)
    g = [0] * n
    for i in range(n):
        t = (i - a) % (2 * n)
        g[i] = f[t % n] if t < n else (-f[t % n]) % M
    if mode == "cmux":
        g = [(x - y) % M for x, y in zip(g, f)]
    return g


def digits(x, w, beta, ell):
    s = w - beta * ell
    state = x if s == 0 else ((x + (1 << (s - 1))) % (1 << w)) >> s
    B, out = 1 << beta, []
    for _ in range(ell):
        d = state % B
        state >>= beta
        if d >= B // 2:
            d -= B
            state += 1
        out.append(d)
    return out[::-1]


def model_terms_element(elem, a, w, beta, ell):
    """elem = npolys lists of n ints -> the npolys * ell term polynomials of the CMux difference."""
    row = []
    for f in elem:
        ds = [digits(x, w, beta, ell) for x in source(f, a, w, "cmux")]
        row.extend([[d[l] % (1 << w) for d in ds] for l in range(ell)])
    return row


def ms(x, w, logn):
    return (((x >> (w - logn - 2)) + 1) >> 1) % (2 << logn)


def model_modswitch(lwe, L, batch, w, logn):
    """lwe: batch * (L + 1) ints -> (L + 1) * batch exponents, transposed, the body negated."""
    two_n = 2 << logn
    out = [0] * ((L + 1) * batch)
    for b in range(batch):
        for i in range(L + 1):
            m = ms(lwe[b * (L + 1) + i], w, logn)
            out[i * batch + b] = (two_n - m) % two_n if i == L else m
    return out


def model_extract(glwe, h, w):
    """glwe: k + 1 lists of n ints -> k n + 1 ints."""
    n, M, k = len(glwe[0]), 1 << w, len(glwe) - 1
    out = []
    for p in range(k):
        out += [glwe[p][h - j] if j <= h else (-glwe[p][h - j + n]) % M for j in range(n)]
    return out + [glwe[k][h]]


# -- words <-> arrays ---------------------------------------------------------------------------------------------------------------
def wbits(plan):
    return 8 * plan.WORD


def per(plan):
    """array elements per polynomial"""
    return plan.ntt_size() * (2 if plan.WORD == 16 else 1)


def to_array(plan, ints):
    if plan.WORD == 16:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=plan.word_dtype)


def to_ints(plan, a):
    if plan.WORD == 16:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[0::2], a[1::2])]
    return [int(x) for x in a]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def random_words(rng, plan, count):
    """count random words as an array of the plan's word dtype"""
    return rng.integers(0, np.iinfo(plan.word_dtype).max, size=count * (2 if plan.WORD == 16 else 1), dtype=plan.word_dtype, endpoint=True)


def random_key_words(rng, plan, npoly):
    n = plan.ntt_size()
    if not plan.BINARY:
        return random_words(rng, plan, npoly * n)
    bits = rng.integers(0, 2, size=npoly * n).astype(plan.word_dtype)
    if plan.WORD == 16:
        a = np.zeros(2 * npoly * n, dtype=np.uint64)
        a[0::2] = bits
        return a
    return bits


def key_planes(torch, plan, key_words):
    res_t = torch.int64 if plan.RES == 8 else torch.int32
    kr = [torch.empty(len(key_words) // per(plan) * plan.ntt_size(), dtype=res_t, device="cuda") for _ in range(plan.NPRIMES)]
    if len(key_words):   # (no key at all: lwe_dim = 0)
        plan.fwd_batch(dev(torch, key_words), kr, binary=plan.BINARY)
    return kr


def workspace(torch, plan, L, k, levels, batch):
    return torch.zeros(plan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")


# -- 1. modulus switch ----------------------------------------------------------------------------------------------------------------
def modswitch_words(rng, w, logn, count):
    s = w - logn - 1   # one exponent step
    two_n = 2 << logn
    ws = [0, (1 << w) - 1, (1 << w) - (1 << (s - 1)), (1 << w) - (1 << (s - 1)) - 1]          # ... the last ones round up to 2n / just not
    for k in (0, 1, 2, two_n // 2 - 1, two_n // 2, two_n - 2, two_n - 1):
        ws += [(k << s) + (1 << (s - 1)), (k << s) + (1 << (s - 1)) - 1]                       # the ties and the word below each
    return [ws[i // 2 % len(ws)] if i % 2 == 0 else int.from_bytes(rng.bytes(w // 8), "little") for i in range(count)]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n", [32, 1024, 32768])
@pytest.mark.parametrize("w", [32, 64, 128])
def test_modswitch_matches_model(w, n, where):
    torch = _torch()
    plan = WORDS[w].try_new(n)
    logn = n.bit_length() - 1
    rng = np.random.default_rng(seed(w, n, where))
    for L in (0, 1, 3, 17):
        for batch in (1, 3, 37, 70):   # 37 and 70: not multiples of the 32-wide transpose tile, 70 with several tiles per row
            lwe = modswitch_words(rng, w, logn, batch * (L + 1))
            want = np.array(model_modswitch(lwe, L, batch, w, logn), dtype=np.uint32)
            la = to_array(plan, lwe)
            if where == "host":
                got = np.full_like(want, 0xFFFFFFFF)
                plan.lwe_modswitch_batch(got, la, L)
            else:
                t = dev(torch, np.full_like(want, 0xFFFFFFFF))
                plan.lwe_modswitch_batch(t, dev(torch, la), L)
                torch.cuda.synchronize()
                got = host(t, np.uint32)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (w, n, L, batch, "first bad exponent", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]))


# -- 2. sample extraction -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("w", [32, 64, 128])
def test_sample_extract_matches_model(w, k, where):
    torch = _torch()
    for n in (32, 256):
        plan = WORDS[w].try_new(n)
        rng = np.random.default_rng(seed(w, k, n))
        batch = 3
        ga = random_words(rng, plan, batch * (k + 1) * n)
        gi = to_ints(plan, ga)
        for index in (0, 1, n - 1):
            want = []
            for b in range(batch):
                elem = [gi[(b * (k + 1) + p) * n:(b * (k + 1) + p + 1) * n] for p in range(k + 1)]
                want += model_extract(elem, index, w)
            want = to_array(plan, want)
            if where == "host":
                got = np.zeros_like(want)
                plan.sample_extract_batch(got, ga, k, index)
            else:
                t = dev(torch, np.zeros_like(want))
                plan.sample_extract_batch(t, dev(torch, ga), k, index)
                torch.cuda.synchronize()
                got = host(t, want.dtype)
            assert np.array_equal(got, want), (w, k, n, index)


# -- 3. blind rotation against the per-iteration public calls -----------------------------------------------------------------------------
def rot_rows(rng, n, L, batch):
    """(L + 1) x batch exponents below 2n; 0, n and 2n - 1 appear in every row."""
    rows = []
    for i in range(L + 1):
        fixed = [0, n, 2 * n - 1, 1, n - 1, n + 1]
        row = [fixed[(b + i) % len(fixed)] if b < 3 else int(rng.integers(0, 2 * n)) for b in range(batch)]
        rows += row
    return np.array(rows, dtype=np.uint32)


def per_iteration_references(torch, plan, lut_t, per_element, rot_t, kr, L, k, beta, ell, batch):
    """(accumulate in place, two-buffer ping-pong) through the calls of cntt_gadget.h / cntt_ext.h"""
    n, npolys, w = plan.ntt_size(), k + 1, wbits(plan)
    tiled = lut_t if per_element else lut_t.repeat(batch)
    # X^a f = the one full-width digit of the rotate mode
    acc = torch.zeros_like(tiled)
    plan.gadget_decompose_batch(acc, tiled, w, 1, rot=rot_t[L * batch:], mode="rotate")
    pp = [acc.clone(), torch.zeros_like(acc)]
    terms = torch.zeros(acc.numel() * ell, dtype=acc.dtype, device="cuda")
    slice_ = npolys * ell * npolys * n
    for i in range(L):
        ri = rot_t[i * batch:(i + 1) * batch]
        ki = [p[i * slice_:(i + 1) * slice_] for p in kr]
        plan.gadget_decompose_batch(terms, acc, beta, ell, rot=ri, mode="cmux")
        plan.external_product_batch(acc, terms, ki, npolys * ell, npolys, accumulate=True)
        plan.external_product_decomposed_batch(pp[1], pp[0], ki, beta, ell, npolys, rot=ri, mode="cmux", addend=pp[0])
        pp.reverse()
    torch.cuda.synchronize()
    return acc, pp[0]


def check_blind_rotate(torch, kind, n, k, per_element, with_ws, L=5, beta=6, where="device"):
    """where = "host": the call on host slices (a host-side workspace is checked and then ignored), the references on the device"""
    plan = KINDS[kind].try_new(n)
    assert plan is not None
    ell = min(3, plan.max_terms() // (k + 1))
    assert ell >= 1
    batch = 4 if n <= 1024 else 3
    rng = np.random.default_rng(seed(kind, n, k, per_element, with_ws))
    lut_t = dev(torch, random_words(rng, plan, (batch if per_element else 1) * (k + 1) * n))
    rot_t = dev(torch, rot_rows(rng, n, L, batch))
    kr = key_planes(torch, plan, random_key_words(rng, plan, L * (k + 1) * ell * (k + 1)))
    acc = dev(torch, random_words(rng, plan, batch * (k + 1) * n))   # written only: the prior content must not matter
    if where == "host":
        acc_h = host(acc, plan.word_dtype).copy()
        ws = np.zeros(plan.pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8) if with_ws else None
        plan.blind_rotate_batch(acc_h, host(lut_t, plan.word_dtype).copy(), host(rot_t, np.uint32).copy(),
                                [host(p, plan.res_dtype).copy() for p in kr], L, k, beta, ell, workspace=ws, lut_per_element=per_element)
        acc = dev(torch, acc_h)
    else:
        ws = workspace(torch, plan, L, k, ell, batch) if with_ws else None
        plan.blind_rotate_batch(acc, lut_t, rot_t, kr, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    inplace, pingpong = per_iteration_references(torch, plan, lut_t, per_element, rot_t, kr, L, k, beta, ell, batch)
    assert torch.equal(inplace, pingpong), (kind, n, k, "the two per-iteration references differ")
    assert torch.equal(acc, inplace), (kind, n, k, per_element, with_ws, L, where, "blind_rotate_batch differs from the per-iteration calls")


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_blind_rotate_equals_per_iteration_calls_n256(kind):
    torch = _torch()
    for k, per_element, with_ws in ((1, False, False), (1, True, True), (2, False, True), (2, True, False)):
        check_blind_rotate(torch, kind, 256, k, per_element, with_ws)
    # the host path with and without a workspace, and on all three paths lwe_dim = 0: the set-up alone, no digits, no key, and a
    # workspace the call does not touch (the device path allocates none)
    for per_element, with_ws, L, where in ((False, True, 2, "host"), (True, False, 2, "host"), (False, True, 0, "device"),
                                           (True, False, 0, "device"), (False, False, 0, "host")):
        check_blind_rotate(torch, kind, 256, 1, per_element, with_ws, L=L, where=where)


@pytest.mark.parametrize("n", [1024, 4096])
@pytest.mark.parametrize("kind", FUSED)
def test_blind_rotate_equals_per_iteration_calls_fused_sizes(kind, n):
    torch = _torch()
    for k, per_element, with_ws in ((1, False, True), (2, True, False)):
        check_blind_rotate(torch, kind, n, k, per_element, with_ws)


def test_blind_rotate_equals_per_iteration_calls_composed_n8192():
    torch = _torch()
    for k, per_element, with_ws in ((1, True, True), (2, False, False)):
        check_blind_rotate(torch, "native64_plan32", 8192, k, per_element, with_ws)


STREAM_BYTES = 384 << 20   # the library's streaming threshold (host_common.hpp)


@pytest.mark.parametrize("w,per_element", [(32, True), (64, False), (128, False)])
def test_blind_rotate_set_up_of_a_streaming_batch(w, per_element):
    """native_pbs_init_kernel<W, true> on the three word widths: blind_rotate_batch with lwe_dim = 0 is the set-up alone (acc = X^rot
    lut: no digits, no key); the first batch whose accumulator passes the streaming threshold (non-temporal stores) at n = 1024, k = 1,
    against the same call made in two halves, which do not stream, on every word, and against the model on the first, the last and 32
    sampled elements."""
    torch = _torch()
    n, k = 1024, 1
    plan = WORDS[w].try_new(n)
    pe = (k + 1) * per(plan)          # array elements per batch element
    batch = STREAM_BYTES // ((k + 1) * n * plan.WORD) + 1
    tt, lo, hi = (torch.int32, -2 ** 31, 2 ** 31 - 1) if w == 32 else (torch.int64, -2 ** 63, 2 ** 63 - 1)
    g = torch.Generator(device="cuda").manual_seed(w)
    lut = torch.randint(lo, hi, ((batch if per_element else 1) * pe,), dtype=tt, device="cuda", generator=g)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=g)
    nokey = [torch.empty(0, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    acc = torch.empty(batch * pe, dtype=tt, device="cuda")
    plan.blind_rotate_batch(acc, lut, rot, nokey, 0, k, 7, 3, lut_per_element=per_element)
    half = batch // 2
    small = torch.empty((batch - half) * pe, dtype=tt, device="cuda")
    plan.blind_rotate_batch(small[:half * pe], lut[:half * pe] if per_element else lut, rot[:half], nokey, 0, k, 7, 3, lut_per_element=per_element)
    assert torch.equal(small[:half * pe], acc[:half * pe])
    plan.blind_rotate_batch(small, lut[half * pe:] if per_element else lut, rot[half:], nokey, 0, k, 7, 3, lut_per_element=per_element)
    assert torch.equal(small, acc[half * pe:])
    rot_h = rot.cpu().tolist()
    rng = np.random.default_rng(seed("stream-init", w))
    for b in sorted({0, batch - 1} | {int(x) for x in rng.integers(0, batch, size=32)}):
        f = to_ints(plan, host(lut[b * pe:(b + 1) * pe] if per_element else lut, plan.word_dtype))
        want = [x for q in range(k + 1) for x in source(f[q * n:(q + 1) * n], rot_h[b], w, "rotate")]
        assert to_ints(plan, host(acc[b * pe:(b + 1) * pe], plan.word_dtype)) == want, (w, "element", b)


# -- 4. blind rotation against the big-integer model and the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["native64_plan32", "native_binary32_plan32"])
def test_blind_rotate_matches_model_and_oracle(oracle, kind):
    torch = _torch()
    n, k, beta, ell, L, batch = 256, 1, 6, 3, 3, 3
    npolys = k + 1
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    rng = np.random.default_rng(seed(kind, "pbs-model"))
    lut_a = random_words(rng, plan, npolys * n)
    rot = rot_rows(rng, n, L, batch)
    key_a = random_key_words(rng, plan, L * npolys * ell * npolys)
    kr = key_planes(torch, plan, key_a)
    acc_t = dev(torch, np.zeros(batch * npolys * n, dtype=plan.word_dtype))
    plan.blind_rotate_batch(acc_t, dev(torch, lut_a), dev(torch, rot), kr, L, k, beta, ell)
    torch.cuda.synchronize()
    got = to_ints(plan, host(acc_t, plan.word_dtype))
    ref = oracle.Native(kind, n)
    lut_i, key_i = to_ints(plan, lut_a), to_ints(plan, key_a)
    keyp = [key_i[j * n:(j + 1) * n] for j in range(len(key_i) // n)]
    for b in range(batch):
        acc = [source(lut_i[p * n:(p + 1) * n], int(rot[L * batch + b]), w, "rotate") for p in range(npolys)]
        for i in range(L):
            terms = model_terms_element(acc, int(rot[i * batch + b]), w, beta, ell)
            base = i * npolys * ell * npolys
            for o in range(npolys):
                add = [0] * n
                for j, t in enumerate(terms):
                    prod = np.zeros(n, dtype=plan.word_dtype)
                    ref.negacyclic_polymul(prod, to_array(plan, t), to_array(plan, keyp[base + j * npolys + o]))
                    add = [(x + int(y)) % (1 << w) for x, y in zip(add, prod)]
                acc[o] = [(x + y) % (1 << w) for x, y in zip(acc[o], add)]   # every term reads the accumulator BEFORE this iteration
        want = [x for p in acc for x in p]
        assert got[b * npolys * n:(b + 1) * npolys * n] == want, (kind, "element", b)


# -- 5. bootstrap == its three steps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,where,with_ws", [("native64_plan32", 1024, "device", True), ("native64_plan32", 1024, "device", False),
                                                  ("native128_plan32", 256, "device", True), ("native_binary32_plan52", 256, "device", False),
                                                  ("native32_plan32", 256, "host", False), ("native64_plan32", 1024, "host", True)])
def test_bootstrap_equals_its_three_steps(kind, n, where, with_ws):
    check_bootstrap_steps(kind, n, where, with_ws, L=4, batch=5)


@pytest.mark.parametrize("where,with_ws", [("device", True), ("device", False), ("host", True)])
def test_bootstrap_without_mask_words_equals_its_three_steps(where, with_ws):
    """lwe_dim = 0: the body alone -- no iteration, no key, and of the workspace only rot_t and the accumulator"""
    check_bootstrap_steps("native64_plan32", 256, where, with_ws, L=0, batch=2)


def check_bootstrap_steps(kind, n, where, with_ws, L, batch):
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    k, beta = 1, 7
    ell = min(3, plan.max_terms() // (k + 1))
    rng = np.random.default_rng(seed(kind, n, where))
    lwe_a = random_words(rng, plan, batch * (L + 1))
    lut_a = random_words(rng, plan, (k + 1) * n)
    key_a = random_key_words(rng, plan, L * (k + 1) * ell * (k + 1))
    kr = key_planes(torch, plan, key_a)
    out_words = batch * (k * n + 1) * (2 if plan.WORD == 16 else 1)
    if where == "host":
        to, fro = (lambda a: a.copy()), (lambda a, dt: a)
        kr = [host(p, plan.res_dtype).copy() for p in kr]
        ws = np.zeros(plan.pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8) if with_ws else None
    else:
        to, fro = (lambda a: dev(torch, a)), host
        ws = workspace(torch, plan, L, k, ell, batch) if with_ws else None
    lwe_t, lut_t = to(lwe_a), to(lut_a)
    one = to(np.zeros(out_words, dtype=plan.word_dtype))
    plan.bootstrap_batch(one, lwe_t, lut_t, kr, L, k, beta, ell, workspace=ws)
    rot_t = to(np.zeros((L + 1) * batch, dtype=np.uint32))
    acc = to(np.zeros(batch * (k + 1) * per(plan), dtype=plan.word_dtype))
    steps = to(np.zeros(out_words, dtype=plan.word_dtype))
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    plan.blind_rotate_batch(acc, lut_t, rot_t, kr, L, k, beta, ell)
    plan.sample_extract_batch(steps, acc, k, 0)
    if where == "device":
        torch.cuda.synchronize()
    assert np.array_equal(fro(one, plan.word_dtype), fro(steps, plan.word_dtype)), (kind, n, where, with_ws)
    assert fro(one, plan.word_dtype).any()
    if L == 0:   # and the model: coefficient 0 of X^(-ms(body)) lut
        w, logn, lut_i, lwe_i = wbits(plan), n.bit_length() - 1, to_ints(plan, lut_a), to_ints(plan, lwe_a)
        want = []
        for b in range(batch):
            a = (2 * n - ms(lwe_i[b], w, logn)) % (2 * n)
            want += model_extract([source(lut_i[q * n:(q + 1) * n], a, w, "rotate") for q in range(k + 1)], 0, w)
        assert to_ints(plan, fro(one, plan.word_dtype)) == want, (kind, where, with_ws, "lwe_dim = 0 against the model")


# -- 6. the bootstrap bootstraps ------------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


def test_bootstrap_evaluates_the_table_on_encrypted_messages():
    """native64 Plan32, n = 1024, k = 1, base_log 8, levels 4, L = 32; binary LWE / GLWE keys, a noiseless bootstrapping key (row (p, l)
    = a fresh GLWE encryption of 0 with s_i 2^(w - base_log l) added to polynomial p, coefficient 0; the products A S from
    negacyclic_polymul_batch), 4 messages under one padding bit, boxes of n / 4 coefficients shifted by half a box, input noise
    below 2^40.  Phase convention: body - sum A_p S_p; coefficient 0 of X^(-m) v is v[m].
    The bound, derived and not measured: with a noiseless key the only error is the gadget rounding, at most 2^(s-1) per coefficient
    with s = w - base_log levels, which enters the phase through the body and through k products with a binary key polynomial (n
    coefficients each), once per iteration: |phase - f(m) 2^(w-3)| <= L (1 + k n) 2^(w - base_log levels - 1).  Box selection is safe:
    the modulus switch errs by at most (L + 1) / 2 = 16.5 exponents (plus 2^40 / 2^53 of the noise), below half a box = 128."""
    torch = _torch()
    n, k, beta, ell, L, w, reps = 1024, 1, 8, 4, 32, 64, 8
    plan = native64.Plan32.try_new(n)
    g = torch.Generator(device="cuda").manual_seed(2024)

    def rand64(*shape):
        return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device="cuda", generator=g)

    s = torch.randint(0, 2, (L,), dtype=torch.int64, device="cuda", generator=g)
    S = torch.randint(0, 2, (k, n), dtype=torch.int64, device="cuda", generator=g)
    rows = (k + 1) * ell
    # key[i][j][o]: mask polynomials uniform, body = sum_q A_q S_q
    key = torch.zeros((L, rows, k + 1, n), dtype=torch.int64, device="cuda")
    key[:, :, :k, :] = rand64(L, rows, k, n)
    A = key[:, :, :k, :].contiguous()
    prod = torch.zeros_like(A)
    plan.negacyclic_polymul_batch(prod.view(-1), A.view(-1), S.expand(L, rows, k, n).contiguous().view(-1))
    key[:, :, k, :] = prod.sum(dim=2)
    for p in range(k + 1):
        for l in range(1, ell + 1):
            key[:, p * ell + l - 1, p, 0] += s << (w - beta * l)
    kr = [torch.empty(key.numel(), dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(key.view(-1), kr)
    # the table: trivial GLWE, body X^(-n/8) v0 with v0[j] = f(j / (n/4)) 2^61
    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = pbs_f((t % n) // (n // 4)) << 61
        lut[k * n + j] = v if t < n else (-v) % (1 << 64)
    msgs = torch.arange(4, dtype=torch.int64, device="cuda").repeat(reps)
    batch = msgs.numel()
    a = rand64(batch, L)
    noise = torch.randint(-2 ** 40 + 1, 2 ** 40, (batch,), dtype=torch.int64, device="cuda", generator=g)
    body = (a * s).sum(dim=1) + (msgs << 61) + noise
    lwe_in = torch.cat([a, body[:, None]], dim=1).contiguous().view(-1)
    lwe_out = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.bootstrap_batch(lwe_out, lwe_in, dev(torch, lut), kr, L, k, beta, ell)
    torch.cuda.synchronize()
    ct = lwe_out.view(batch, k * n + 1)
    phase = ct[:, k * n] - (ct[:, :k * n] * S.view(-1)).sum(dim=1)            # int64 arithmetic wraps: mod 2^64
    want = torch.tensor([pbs_f(int(m)) << 61 for m in msgs.cpu()], dtype=torch.int64, device="cuda")
    err = (phase - want).cpu().numpy().astype(np.int64)                         # the centred representative
    bound = L * (1 + k * n) * 2 ** (w - beta * ell - 1)
    print("largest |phase error| = %d, bound = %d" % (int(np.abs(err).max()), bound))
    assert int(np.abs(err).max()) <= bound, (int(np.abs(err).max()), bound)
    decoded = ((phase >> 60) + 1 >> 1) & 7
    assert decoded.cpu().tolist() == [pbs_f(int(m)) for m in msgs.cpu()]


# -- 7. graph capture ---------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_bootstrap_with_a_caller_workspace():
    torch = _torch()
    n, L, k, beta, ell, batch = 1024, 8, 1, 8, 3, 37
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(7)
    lwe = dev(torch, random_words(rng, plan, batch * (L + 1)))
    lut = dev(torch, random_words(rng, plan, (k + 1) * n))
    kr = key_planes(torch, plan, random_key_words(rng, plan, L * (k + 1) * ell * (k + 1)))
    ws = workspace(torch, plan, L, k, ell, batch)
    eager = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.bootstrap_batch(eager, lwe, lut, kr, L, k, beta, ell, workspace=ws)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.bootstrap_batch(out, lwe, lut, kr, L, k, beta, ell, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(out, eager)


# -- 8. the C example -----------------------------------------------------------------------------------------------------------------------
def test_pbs_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pbs"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pbs")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 4 and not any("WRONG" in ln for ln in lines), r.stdout
