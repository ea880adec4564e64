"""The LWE keyswitch of the native plans (include/cntt_keyswitch.h) on the MI355X.  Bit-exact throughout, no tolerance anywhere: the
kernel against a big-integer model (Python ints; the model is checked against the header's phase identity in
tests/test_native_keyswitch_abi.py and restated here) on shapes that cross every tile edge, on deterministic worst cases and on
encrypted messages; cntt_native_keyswitch_bootstrap_batch against the two calls it replaces; two chained rounds; graph capture; the C
example."""
import os
import subprocess
import zlib

import numpy as np
import pytest

from concrete_ntt_amd import native32, native64, native128

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = {32: native32.Plan32, 64: native64.Plan32, 128: native128.Plan32}
# the kernel's tile (native_keyswitch.hpp): batch elements x columns per workgroup, and digit rows per chunk of mask words
TILE_B = {32: 64, 64: 64, 128: 32}
TILE_C = 128
ROWS = 128


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# -- the model: plain Python ints (as in tests/test_native_keyswitch_abi.py) ------------------------------------------------------------
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


def model_keyswitch_batch(lwe, ksk, lin, lout, stride, w, beta, ell, batch):
    """lwe: batch * (lin + 1) ints; ksk: flat ints, row r at r * stride -> batch * (lout + 1) ints.  The sums run over Python ints in
    object arrays: exact, reduced modulo 2^w at the end."""
    M = 1 << w
    body = [lwe[b * (lin + 1) + lin] for b in range(batch)]
    if lin == 0:
        return [x for b in range(batch) for x in [0] * lout + [body[b]]]
    D = np.array([[d for i in range(lin) for d in digits(lwe[b * (lin + 1) + i], w, beta, ell)] for b in range(batch)], dtype=object)
    Kmat = np.array([ksk[r * stride:r * stride + lout + 1] for r in range(lin * ell)], dtype=object)
    acc = D.dot(Kmat)
    out = []
    for b in range(batch):
        row = [(-int(x)) % M for x in acc[b]]
        row[lout] = (row[lout] + body[b]) % M
        out += row
    return out


# -- words <-> arrays ---------------------------------------------------------------------------------------------------------------
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


def rand_ints(rng, w, count):
    raw = rng.bytes(count * (w // 8))
    return [int.from_bytes(raw[i * (w // 8):(i + 1) * (w // 8)], "little") for i in range(count)]


def random_words(rng, plan, count):
    return rng.integers(0, np.iinfo(plan.word_dtype).max, size=count * (2 if plan.WORD == 16 else 1), dtype=plan.word_dtype, endpoint=True)


def key_planes(torch, plan, key_words):
    per = plan.ntt_size() * (2 if plan.WORD == 16 else 1)
    kr = [torch.empty(len(key_words) // per * plan.ntt_size(), dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(dev(torch, key_words), kr)
    return kr


def run_keyswitch(torch, plan, where, lwe, ksk, lin, lout, stride, beta, ell, batch):
    """the call on int lists -> the output as ints; the output buffer starts out poisoned"""
    mult = 2 if plan.WORD == 16 else 1
    la, ka = to_array(plan, lwe), to_array(plan, ksk)
    poison = np.full(batch * (lout + 1) * mult, 0xA5, dtype=plan.word_dtype)
    if where == "host":
        plan.keyswitch_batch(poison, la, ka, lin, lout, beta, ell, row_stride=stride)
        return to_ints(plan, poison)
    out = dev(torch, poison)
    kt = dev(torch, ka) if len(ksk) else torch.empty(0, dtype=out.dtype, device="cuda")
    plan.keyswitch_batch(out, dev(torch, la), kt, lin, lout, beta, ell, row_stride=stride)
    torch.cuda.synchronize()
    return to_ints(plan, host(out, plan.word_dtype))


def key_len(lin, ell, lout, stride):
    return ((lin * ell - 1) * stride + lout + 1) if lin else 0   # the last row ends after its lout + 1 words


# -- 1. the kernel against the model across every tile edge -------------------------------------------------------------------------------
def shapes(w):
    """(batch, lin, lout, stride pad, beta, ell): batch 1 / tile - 1 / tile + 1 / a few hundred; lout + 1 one column, below, above and
    several times the column tile; lin 0, one word, and one below / above the chunk of ROWS // ell words; packed and padded rows;
    beta * ell = w and < w; beta = 1 and beta = 31."""
    tb = TILE_B[w]
    full = {32: (8, 4), 64: (16, 4), 128: (16, 8)}[w]          # beta * ell = w
    top = {32: (31, 1), 64: (31, 2), 128: (31, 4)}[w]           # beta = 31
    return [(1, ROWS // 3 - 1, TILE_C, 0, 5, 3),
            (tb - 1, ROWS // full[1] + 1, TILE_C - 2, 3, *full),
            (tb + 1, ROWS // 3 + 1, TILE_C + 1, 1, 5, 3),
            (200, 37, 2 * TILE_C + 43, 0, 4, 3),
            (tb + 3, 1, 5, 2, *top),
            (3, ROWS // 7 + 2, TILE_C - 1, 5, 1, 7),
            (5, 0, 9, 0, 6, 2),
            (tb + 1, 11, 0, 0, 6, 2),
            (2, 3, 0, 4, *top)]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("w", [32, 64, 128])
def test_keyswitch_matches_model(w, where):
    torch = _torch()
    plan = WORDS[w].try_new(32)                                  # ntt_size plays no part
    for batch, lin, lout, pad, beta, ell in shapes(w):
        rng = np.random.default_rng(seed(w, where, batch, lin, lout))
        stride = lout + 1 + pad
        lwe = rand_ints(rng, w, batch * (lin + 1))
        ksk = rand_ints(rng, w, key_len(lin, ell, lout, stride))  # padding words poisoned with random bits
        want = model_keyswitch_batch(lwe, ksk, lin, lout, stride, w, beta, ell, batch)
        got = run_keyswitch(torch, plan, where, lwe, ksk, lin, lout, stride, beta, ell, batch)
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
        assert not bad, (w, where, batch, lin, lout, pad, beta, ell, "first bad word", bad[0], hex(got[bad[0]]), hex(want[bad[0]]), len(bad))
        if pad and where == "device":                            # other padding words, the same result
            other = list(ksk)
            for r in range(lin * ell - 1):
                for c in range(lout + 1, stride):
                    other[r * stride + c] ^= (1 << w) - 1
            assert run_keyswitch(torch, plan, where, lwe, other, lin, lout, stride, beta, ell, batch) == got, (w, batch, "padding read")


# -- 2. deterministic worst cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 64, 128])
def test_keyswitch_worst_cases(w):
    """Every digit -B/2 against all-ones key words, every digit B/2 - 1 against 2^(w-1), and words 2^w - 1 that round up across the top
    (to all-zero digits when s > 0): a wrong sign fix-up or a lost carry shows in every word."""
    torch = _torch()
    plan = WORDS[w].try_new(32)
    M = 1 << w
    batch, lout = TILE_B[w] + 1, TILE_C + 1
    for beta, ell in ((4, 3), (1, 5), (31, w // 32), (w // 4, 4)):
        if beta > 31:
            continue
        s, B = w - beta * ell, 1 << beta
        lin = ROWS // ell + 2
        low = (sum(-(B // 2) << (beta * j) for j in range(ell)) % (1 << (beta * ell))) << s
        high = sum((B // 2 - 1) << (beta * (ell - 1 - j)) for j in range(ell)) << s
        assert digits(low, w, beta, ell) == [-B // 2] * ell and digits(high, w, beta, ell) == [B // 2 - 1] * ell
        assert s == 0 or digits(M - 1, w, beta, ell) == [0] * ell
        rng = np.random.default_rng(seed(w, beta, ell))
        for word, keyword in ((low, M - 1), (high, 1 << (w - 1)), (M - 1, None)):
            lwe = [word] * (batch * (lin + 1))
            ksk = [keyword] * (lin * ell * (lout + 1)) if keyword is not None else rand_ints(rng, w, lin * ell * (lout + 1))
            want = model_keyswitch_batch(lwe, ksk, lin, lout, lout + 1, w, beta, ell, batch)
            got = run_keyswitch(torch, plan, "device", lwe, ksk, lin, lout, lout + 1, beta, ell, batch)
            assert got == want, (w, beta, ell, hex(word))


# -- 3. decryption ------------------------------------------------------------------------------------------------------------------------
def test_keyswitch_decrypts_under_the_output_key():
    """w = 64: 3-bit messages at 2^61 under a binary key of dimension k n = 256, a noisy key (|e| < 2^20) to a binary key of dimension
    L = 40 with base_log 4, levels 6.  The model's output decrypts every message -- asserted first, on the CPU -- and the device words
    are the model's.  (Rounding error at most 256 * 2^39 = 2^47, key noise at most 256 * 6 * 8 * 2^20 < 2^34: far below 2^60.)"""
    torch = _torch()
    w, lin, lout, beta, ell, batch = 64, 256, 40, 4, 6, 16
    M = 1 << w
    plan = WORDS[w].try_new(256)
    rng = np.random.default_rng(seed("decrypt"))
    s_in = [int(x) for x in rng.integers(0, 2, size=lin)]
    s_out = [int(x) for x in rng.integers(0, 2, size=lout)]
    ksk = []
    for i in range(lin):
        for l in range(1, ell + 1):
            a = rand_ints(rng, w, lout)
            e = int(rng.integers(-2 ** 20 + 1, 2 ** 20))
            ksk += a + [(sum(x * t for x, t in zip(a, s_out)) + s_in[i] * (1 << (w - beta * l)) + e) % M]
    msgs = [b % 8 for b in range(batch)]
    lwe = []
    for m in msgs:
        a = rand_ints(rng, w, lin)
        e = int(rng.integers(-2 ** 40 + 1, 2 ** 40))
        lwe += a + [(sum(x * t for x, t in zip(a, s_in)) + (m << 61) + e) % M]
    want = model_keyswitch_batch(lwe, ksk, lin, lout, lout + 1, w, beta, ell, batch)

    def decrypt(ct):
        phase = (ct[lout] - sum(x * t for x, t in zip(ct, s_out))) % M
        return (((phase >> 60) + 1) >> 1) & 7

    assert [decrypt(want[b * (lout + 1):(b + 1) * (lout + 1)]) for b in range(batch)] == msgs     # the model, on the CPU
    for where in ("device", "host"):
        assert run_keyswitch(torch, plan, where, lwe, ksk, lin, lout, lout + 1, beta, ell, batch) == want, where


# -- 4. keyswitch + bootstrap == the two calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,where,with_ws", [(1024, "device", True), (1024, "device", False), (1024, "host", True), (1024, "host", False),
                                             (8192, "device", True), (8192, "device", False), (8192, "host", False)])
def test_keyswitch_bootstrap_equals_the_two_calls(n, where, with_ws):
    """native64 Plan32: n = 1024 runs the fused external product, n = 8192 the composed one"""
    torch = _torch()
    plan = native64.Plan32.try_new(n)
    L, k, beta, batch, ks_beta, ks_ell, pad = 4, 1, 7, 5, 4, 3, 1
    ell = min(3, plan.max_terms() // (k + 1))
    big, stride = k * n, L + 1 + pad
    rng = np.random.default_rng(seed(n, where, with_ws))
    in_a = random_words(rng, plan, batch * (big + 1))
    ksk_a = random_words(rng, plan, key_len(big, ks_ell, L, stride))
    lut_a = random_words(rng, plan, (k + 1) * n)
    kr = key_planes(torch, plan, random_words(rng, plan, L * (k + 1) * ell * (k + 1) * n))
    if where == "host":
        to, fro = (lambda a: a.copy()), (lambda a, dt: a)
        kr = [host(p, plan.res_dtype).copy() for p in kr]
        ws = np.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=np.uint8) if with_ws else None
    else:
        to, fro = (lambda a: dev(torch, a)), host
        ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=torch.uint8, device="cuda") if with_ws else None
    in_t, ksk_t, lut_t = to(in_a), to(ksk_a), to(lut_a)
    one = to(np.zeros(batch * (big + 1), dtype=plan.word_dtype))
    plan.keyswitch_bootstrap_batch(one, in_t, ksk_t, ks_beta, ks_ell, lut_t, kr, L, k, beta, ell, workspace=ws, row_stride=stride)
    mid = to(np.zeros(batch * (L + 1), dtype=plan.word_dtype))
    two = to(np.zeros(batch * (big + 1), dtype=plan.word_dtype))
    plan.keyswitch_batch(mid, in_t, ksk_t, big, L, ks_beta, ks_ell, row_stride=stride)
    plan.bootstrap_batch(two, mid, lut_t, kr, L, k, beta, ell)
    if where == "device":
        torch.cuda.synchronize()
    assert np.array_equal(fro(one, plan.word_dtype), fro(two, plan.word_dtype)), (n, where, with_ws)
    assert fro(one, plan.word_dtype).any() and fro(mid, plan.word_dtype).any()


# -- 5. two chained rounds evaluate g o f ------------------------------------------------------------------------------------------------------
def pbs_f(m):
    return (3 * m + 2) & 3


def pbs_g(m):
    return (m * m + 1) & 3


def table(fn, n, k):
    """trivial GLWE, body X^(-n/8) v0 with v0[j] = fn(j / (n/4)) 2^61"""
    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = fn((t % n) // (n // 4)) << 61
        lut[k * n + j] = v if t < n else (-v) % (1 << 64)
    return lut


class Circuit:
    """native64 Plan32, n = 1024, k = 1, L = 32; noiseless bootstrapping key base_log 8, levels 4 (the recipe of
    tests/test_gpu_native_pbs.py); keyswitch key from the flattened GLWE key to the LWE key, base_log 5, levels 5, |noise| < 2^20;
    messages of 2 bits under one padding bit, encrypted under the flattened GLWE key with noise below 2^40."""
    n, k, beta, ell, L, w, ks_beta, ks_ell = 1024, 1, 8, 4, 32, 64, 5, 5

    def __init__(self, torch, reps):
        n, k, beta, ell, L, w = self.n, self.k, self.beta, self.ell, self.L, self.w
        self.plan = plan = native64.Plan32.try_new(n)
        g = torch.Generator(device="cuda").manual_seed(4242)

        def rand64(*shape):
            return torch.randint(-2 ** 63, 2 ** 63 - 1, shape, dtype=torch.int64, device="cuda", generator=g)

        s = torch.randint(0, 2, (L,), dtype=torch.int64, device="cuda", generator=g)
        self.S = S = torch.randint(0, 2, (k, n), dtype=torch.int64, device="cuda", generator=g)
        rows = (k + 1) * ell
        key = torch.zeros((L, rows, k + 1, n), dtype=torch.int64, device="cuda")
        key[:, :, :k, :] = rand64(L, rows, k, n)
        A = key[:, :, :k, :].contiguous()
        prod = torch.zeros_like(A)
        plan.negacyclic_polymul_batch(prod.view(-1), A.view(-1), S.expand(L, rows, k, n).contiguous().view(-1))
        key[:, :, k, :] = prod.sum(dim=2)
        for p in range(k + 1):
            for l in range(1, ell + 1):
                key[:, p * ell + l - 1, p, 0] += s << (w - beta * l)
        self.kr = [torch.empty(key.numel(), dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
        plan.fwd_batch(key.view(-1), self.kr)
        # ksk[i][l]: (a, <a, s> + S_i 2^(w - ks_beta l) + e), rows packed
        big = k * n
        a = rand64(big, self.ks_ell, L)
        e = torch.randint(-2 ** 20 + 1, 2 ** 20, (big, self.ks_ell), dtype=torch.int64, device="cuda", generator=g)
        shifts = torch.tensor([w - self.ks_beta * l for l in range(1, self.ks_ell + 1)], dtype=torch.int64, device="cuda")
        body = (a * s).sum(dim=2) + (S.view(-1)[:, None] << shifts[None, :]) + e
        self.ksk = torch.cat([a, body[:, :, None]], dim=2).contiguous().view(-1)
        self.msgs = torch.arange(4, dtype=torch.int64, device="cuda").repeat(reps)
        batch = self.batch = self.msgs.numel()
        a = rand64(batch, big)
        noise = torch.randint(-2 ** 40 + 1, 2 ** 40, (batch,), dtype=torch.int64, device="cuda", generator=g)
        body = (a * S.view(-1)).sum(dim=1) + (self.msgs << 61) + noise
        self.ct = torch.cat([a, body[:, None]], dim=1).contiguous().view(-1)

    def round(self, torch, ct_in, fn, workspace=None):
        out = torch.zeros_like(ct_in)
        self.plan.keyswitch_bootstrap_batch(out, ct_in, self.ksk, self.ks_beta, self.ks_ell, dev(torch, table(fn, self.n, self.k)), self.kr,
                                            self.L, self.k, self.beta, self.ell, workspace=workspace)
        return out

    def decode(self, ct):
        ct = ct.view(self.batch, self.k * self.n + 1)
        phase = ct[:, self.k * self.n] - (ct[:, :self.k * self.n] * self.S.view(-1)).sum(dim=1)    # int64 arithmetic wraps: mod 2^64
        return (((phase >> 60) + 1 >> 1) & 7).cpu().tolist()


def test_two_chained_rounds_evaluate_g_of_f():
    torch = _torch()
    c = Circuit(torch, reps=4)
    first = c.round(torch, c.ct, pbs_f)
    second = c.round(torch, first, pbs_g)
    torch.cuda.synchronize()
    msgs = [int(m) for m in c.msgs.cpu()]
    assert c.decode(first) == [pbs_f(m) for m in msgs]
    assert c.decode(second) == [pbs_g(pbs_f(m)) for m in msgs]


# -- 6. graph capture -------------------------------------------------------------------------------------------------------------------------
def test_graph_capture_of_keyswitch_bootstrap_with_a_caller_workspace():
    """captured once, replayed on fresh inputs written into the captured buffers"""
    torch = _torch()
    n, L, k, beta, ell, batch, ks_beta, ks_ell = 1024, 8, 1, 8, 3, 37, 4, 4
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(11)
    big = k * n
    ct = dev(torch, random_words(rng, plan, batch * (big + 1)))
    ksk = dev(torch, random_words(rng, plan, big * ks_ell * (L + 1)))
    lut = dev(torch, random_words(rng, plan, (k + 1) * n))
    kr = key_planes(torch, plan, random_words(rng, plan, L * (k + 1) * ell * (k + 1) * n))
    ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros_like(ct)
    plan.keyswitch_bootstrap_batch(out, ct, ksk, ks_beta, ks_ell, lut, kr, L, k, beta, ell, workspace=ws)   # warm-up: tables, code objects
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):   # a linear chain of kernels: no allocation with a caller workspace at this size
        plan.keyswitch_bootstrap_batch(out, ct, ksk, ks_beta, ks_ell, lut, kr, L, k, beta, ell, workspace=ws)
    fresh = dev(torch, random_words(rng, plan, batch * (big + 1)))
    eager = torch.zeros_like(ct)
    plan.keyswitch_bootstrap_batch(eager, fresh, ksk, ks_beta, ks_ell, lut, kr, L, k, beta, ell)
    ct.copy_(fresh)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert eager.any() and torch.equal(out, eager)


# -- 7. the C example -------------------------------------------------------------------------------------------------------------------------
def test_ks_pbs_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "ks_pbs"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "ks_pbs")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("message ")]
    assert len(lines) == 4 and not any("WRONG" in ln for ln in lines), r.stdout
