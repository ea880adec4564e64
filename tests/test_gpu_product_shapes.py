"""product::Plan shapes any caller can reach through the public API and no other test runs: five, six and seven primes (the
Garner kernel is instantiated for k = 1 ... 7, the rest of the suite stops at four), three u32 primes next to a u64 one at the
smallest size, plans at n = 8192 / 16384 (per-prime transforms on the wave-block walk, the u32x2 inverse composed because the
fused kernel stops at n = 4096) and a u32 pair whose primes sit in different arithmetic classes (composed inverse by default).
Each shape is compared with the oracle's Product word for word -- including the ntt buffer that inv leaves behind -- and with
Python integers."""
import numpy as np
import pytest

from test_product import _ref_primes

pytestmark = pytest.mark.gpu

SMALL = [193, 257, 449, 577, 641, 769, 1153]    # all = 1 mod 64; the product of the seven is about 7.3e18 < 2^64
# A u32x2_u64x1 plan does not exist at n = 8192 (test_gpu_product_shape_counts says why); the two plans next to it that do exist
# stand in for it: three u32 primes (Garner over three planes) and one u32 prime beside a u64 one (both plane widths in one buffer).
SHAPES = ["u32x5", "u32x6", "u32x7", "u32x3_u64x1", "u32x2@8192", "u64x1@8192", "u32x3@8192", "u32x1_u64x1@8192", "u32x2@16384",
          "mixed@512"]
MANY = {"u32x5", "u32x6", "u32x7"}


def _shape(oracle, name):
    """(n, primes ascending, modulus)"""
    lp = oracle.largest_prime_in_arithmetic_progression64
    if name in MANY:
        n, primes = 32, SMALL[:int(name[-1])]
    elif name == "u32x3_u64x1":
        n, primes = 32, SMALL[:3] + [lp(64, 1, 0, 2**33)]
    elif name == "mixed@512":
        n, primes = 512, [lp(1024, 1, 0, 2**32 - 1), lp(1024, 1, 0, 2**30)]
    elif name == "u32x3@8192":
        n, primes = 8192, [lp(16384, 1, 0, 2**18)]
        for _ in range(2):
            primes.append(lp(16384, 1, 0, primes[-1] - 1))
    elif name == "u32x1_u64x1@8192":
        n, primes = 8192, [lp(16384, 1, 0, 2**32 + 2**24), 65537]
    else:
        kind, size = name.split("@")
        n = int(size)
        primes = _ref_primes(oracle, n, kind)
    assert all(p is not None and p % (2 * n) == 1 for p in primes), primes
    big = 1
    for p in primes:
        big *= p
    assert big < 2**64
    return n, sorted(primes), big


def _plans(oracle, name):
    from concrete_ntt_amd import product
    n, primes, big = _shape(oracle, name)
    plan, oplan = product.Plan.try_new(n, big, primes), oracle.Product.try_new(n, big, primes)
    assert plan is not None and oplan is not None, name
    assert plan.primes() == primes and plan.ntt_domain_len() == oplan.ntt_domain_len()
    return n, primes, big, plan, oplan


def _negacyclic(a, b, n, big):
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] += int(x) * int(y)
            else:
                out[k - n] -= int(x) * int(y)
    return [v % big for v in out]


def test_gpu_product_shape_counts(oracle):
    from concrete_ntt_amd import product
    for name, want in (("u32x5", (5, 0)), ("u32x6", (6, 0)), ("u32x7", (7, 0)), ("u32x3_u64x1", (3, 1)), ("u32x2@8192", (2, 0)),
                       ("u64x1@8192", (0, 1)), ("u32x3@8192", (3, 0)), ("u32x1_u64x1@8192", (1, 1)), ("u32x2@16384", (2, 0)),
                       ("mixed@512", (2, 0))):
        n, primes, big = _shape(oracle, name)
        plan = product.Plan.try_new(n, big, primes)
        assert (len(plan.plan_32()), len(plan.plan_64())) == want, name
    # Two u32 primes and a u64 one at n = 8192: 65537 and 114689 are the two smallest primes = 1 mod 16384 (16385, 32769, 49153,
    # 81921 and 98305 are composite), and 65537 * 114689 * 2^32 is already past 2^64 -- the reference-shaped helper finds no third
    # prime, and neither implementation accepts the smallest candidate.
    lp = oracle.largest_prime_in_arithmetic_progression64
    assert lp(16384, 1, 0, 65536) is None and lp(16384, 1, 65538, 114689) == 114689 and 65537 * 114689 * 2**32 > 2**64
    assert _ref_primes(oracle, 8192, "u32x2_u64x1")[2] is None
    p64 = lp(16384, 1, 2**32, 2**33)
    for impl in (product.Plan, oracle.Product):
        assert impl.try_new(8192, 65537 * 114689 * p64 % 2**64, [65537, 114689, p64]) is None
    # the mixed pair really is mixed (cntt_prime32_plan_info): otherwise the case is the one-class u32x2 plan again
    n, primes, big = _shape(oracle, "mixed@512")
    classes = [q.info().arith_class for q in product.Plan.try_new(n, big, primes).plan_32()]
    assert classes[0] != classes[1], classes


@pytest.mark.parametrize("name", SHAPES)
def test_gpu_product_shape_calls(oracle, name):
    """fwd Generic, inv Replace / Accumulate (onto modulus - 1 everywhere, so every add wraps), the three pointwise calls; the
    round trip inv(fwd x) n^-1 = x in Python integers; at n = 32 the product against a schoolbook negacyclic product."""
    from concrete_ntt_amd import product
    n, primes, big, plan, oplan = _plans(oracle, name)
    dl = plan.ntt_domain_len()
    a = oracle.fill_uniform(n, big, 71 + n, 64)
    b = oracle.fill_uniform(n, big, 72 + n, 64)
    a[0], a[n - 1], b[0] = big - 1, big - 1, big - 1
    fa, fb, ofa, ofb = (np.zeros(dl, dtype=np.uint64) for _ in range(4))
    plan.fwd(fa, a, product.FwdMode.Generic)
    plan.fwd(fb, b, product.FwdMode.Generic)
    oplan.fwd(ofa, a)
    oplan.fwd(ofb, b)
    assert np.array_equal(fa, ofa) and np.array_equal(fb, ofb)
    ninv = pow(n, -1, big)
    for acc, mode in ((False, product.InvMode.Replace), (True, product.InvMode.Accumulate)):
        s = np.full(n, big - 1 if acc else 0, dtype=np.uint64)
        os_, t, ot = s.copy(), ofa.copy(), ofa.copy()
        plan.inv(s, t, mode)
        oplan.inv(os_, ot, acc)
        assert np.array_equal(s, os_) and np.array_equal(t, ot), acc
        back = [(int(x) - (big - 1 if acc else 0)) * ninv % big for x in s]
        assert back == [int(x) for x in a], acc
    t, ot = ofa.copy(), ofa.copy()
    plan.mul_assign_normalize(t, ofb)
    oplan.mul_assign_normalize(ot, ofb)
    assert np.array_equal(t, ot)
    prod = np.zeros(n, dtype=np.uint64)
    plan.inv(prod, t, product.InvMode.Replace)
    if n == 32:
        assert [int(x) for x in prod] == _negacyclic(a, b, n, big)
    t, ot = ofa.copy(), ofa.copy()
    plan.normalize(t)
    oplan.normalize(ot)
    assert np.array_equal(t, ot)
    t, ot = ofb.copy(), ofb.copy()
    plan.mul_accumulate(t, ofa, ofb)
    oplan.mul_accumulate(ot, ofa, ofb)
    assert np.array_equal(t, ot)


def _poly(buf, i, n, n32, n64, batch):
    """polynomial i's reference-layout ntt buffer out of a plane-major batch buffer (include/cntt.h)"""
    parts = []
    if n32:
        w32 = buf[: (n // 2) * n32 * batch].view(np.uint32).reshape(n32, batch, n)
        parts.append(np.ascontiguousarray(w32[:, i, :]).reshape(-1).view(np.uint64))
    if n64:
        w64 = buf[(n // 2) * n32 * batch:].reshape(n64, batch, n)
        parts.append(np.ascontiguousarray(w64[:, i, :]).reshape(-1))
    return np.concatenate(parts)


@pytest.mark.parametrize("name", SHAPES)
def test_gpu_product_shape_batch_layout(oracle, name):
    """fwd_batch -> mul_assign_normalize_batch -> inv_batch on device tensors, five polynomials, each against the oracle's
    single-polynomial calls"""
    import torch
    from concrete_ntt_amd import product
    n, primes, big, plan, oplan = _plans(oracle, name)
    batch, dl = 5, plan.ntt_domain_len()
    n32 = sum(p < 2**32 for p in primes)
    n64 = len(primes) - n32
    a = oracle.fill_uniform(n * batch, big, 81 + n, 64)
    b = oracle.fill_uniform(n * batch, big, 82 + n, 64)
    a[:n] = big - 1
    b[:n] = big - 1

    def dev(x):
        return torch.from_numpy(x.view(np.int64).copy()).cuda()

    def host(t):
        return t.cpu().numpy().view(np.uint64)

    fa, fb = torch.zeros(dl * batch, dtype=torch.int64, device="cuda"), torch.zeros(dl * batch, dtype=torch.int64, device="cuda")
    plan.fwd_batch(fa, dev(a), product.FwdMode.Generic)
    plan.fwd_batch(fb, dev(b), product.FwdMode.Generic)
    hfa = host(fa)
    plan.mul_assign_normalize_batch(fa, fb)
    hprod = host(fa)
    out = torch.zeros(n * batch, dtype=torch.int64, device="cuda")
    plan.inv_batch(out, fa, product.InvMode.Replace)
    hout, hleft = host(out), host(fa)
    for i in range(batch):
        x, y = np.zeros(dl, dtype=np.uint64), np.zeros(dl, dtype=np.uint64)
        oplan.fwd(x, a[i * n:(i + 1) * n].copy())
        oplan.fwd(y, b[i * n:(i + 1) * n].copy())
        assert np.array_equal(_poly(hfa, i, n, n32, n64, batch), x), i
        oplan.mul_assign_normalize(x, y)
        assert np.array_equal(_poly(hprod, i, n, n32, n64, batch), x), i
        r = np.zeros(n, dtype=np.uint64)
        oplan.inv(r, x)
        assert np.array_equal(hout[i * n:(i + 1) * n], r), i
        assert np.array_equal(_poly(hleft, i, n, n32, n64, batch), x), i      # the residues inv leaves behind


@pytest.mark.parametrize("name", ["u32x5", "u32x7"])
@pytest.mark.parametrize("accumulate", [False, True])
def test_gpu_product_shape_external_product(oracle, name, accumulate):
    """cntt_product_external_product_batch, J = 2, O = 2, against the oracle's fwd / mul_accumulate / inv in sequence"""
    import torch
    from concrete_ntt_amd import product
    n, primes, big, plan, oplan = _plans(oracle, name)
    J, O, batch, dl = 2, 2, 3, plan.ntt_domain_len()
    terms = oracle.fill_uniform(batch * J * n, big, 91, 64)
    terms[:n] = big - 1
    init = np.full(batch * O * n, big - 1, dtype=np.uint64)
    planes = [oracle.fill_uniform(J * O * n, p, 95 + i, 64) for i, p in enumerate(primes)]   # key[j][o] at index j * O + o
    key = np.concatenate([pl.astype(np.uint32) for pl in planes]).view(np.uint64)
    want = np.zeros(batch * O * n, dtype=np.uint64)
    for b in range(batch):
        acc = [np.zeros(dl, dtype=np.uint64) for _ in range(O)]
        for j in range(J):
            t = np.zeros(dl, dtype=np.uint64)
            oplan.fwd(t, terms[(b * J + j) * n:(b * J + j + 1) * n].copy())
            for o in range(O):
                i = j * O + o
                kp = np.concatenate([pl[i * n:(i + 1) * n].astype(np.uint32) for pl in planes]).view(np.uint64)
                oplan.mul_accumulate(acc[o], t, kp)
        for o in range(O):
            r = init[(b * O + o) * n:(b * O + o + 1) * n].copy() if accumulate else np.zeros(n, dtype=np.uint64)
            oplan.inv(r, acc[o], accumulate)
            want[(b * O + o) * n:(b * O + o + 1) * n] = r
    dout = torch.from_numpy((init if accumulate else np.zeros_like(init)).view(np.int64).copy()).cuda()
    dterms = torch.from_numpy(terms.view(np.int64).copy()).cuda()
    dkey = torch.from_numpy(key.view(np.int64).copy()).cuda()
    plan.external_product_batch(dout, dterms, dkey, J, O, product.FwdMode.Generic,
                                product.InvMode.Accumulate if accumulate else product.InvMode.Replace)
    assert np.array_equal(dout.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("name", sorted(MANY))
def test_gpu_product_shape_split_edge_values(oracle, name):
    """The boundary inputs of test_gpu_product_split_edge_values (0, 1, 2^64 - 1, values around the modulus and around multiples
    of each prime) through the division-free `% p` of five, six and seven primes; the list is longer than one polynomial of
    n = 32, so it runs as a batch."""
    import torch
    from concrete_ntt_amd import product
    n, primes, big, plan, oplan = _plans(oracle, name)
    vals = [0, 1, 2**64 - 1, 2**63, 2**63 - 1, big - 1, big % 2**64, big // 2, big // 2 + 1]
    for p in primes:
        for m in (1, 2, 3, (2**64 - 1) // p):
            vals += [(m * p + d) % 2**64 for d in (-1, 0, 1)]
    batch = (len(vals) + n - 1) // n
    std = np.array((vals * 2)[:batch * n], dtype=np.uint64)
    dl, k = plan.ntt_domain_len(), len(primes)
    dntt = torch.zeros(dl * batch, dtype=torch.int64, device="cuda")
    plan.fwd_batch(dntt, torch.from_numpy(std.view(np.int64).copy()).cuda(), product.FwdMode.Generic)
    hntt = dntt.cpu().numpy().view(np.uint64)
    for i in range(batch):
        x, g = np.zeros(dl, dtype=np.uint64), np.zeros(dl, dtype=np.uint64)
        oplan.fwd(x, std[i * n:(i + 1) * n].copy())
        assert np.array_equal(_poly(hntt, i, n, k, 0, batch), x), i
        plan.fwd(g, std[i * n:(i + 1) * n].copy(), product.FwdMode.Generic)     # and the host-slice call
        assert np.array_equal(g, x), i
