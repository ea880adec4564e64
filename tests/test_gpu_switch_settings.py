"""Every setting of the kernel-selection switches that no other test launches a kernel under (include/cntt.h, "testing only":
blk, mul32_blk, ext32_blk, ext_one, ext_split, product_fused).  The header promises bit-identical results for every setting, and
the A/B figures in profiles/ only mean something if both sides compute the same words: each row runs the library under the
non-default value and under the default, and both must equal the oracle word for word.  The shapes are the smallest at which
the two settings take different kernels (read off the dispatch code named next to each row: a test cannot see which kernel
ran).  Polynomial 0 of every batch is the all-(p - 1) one, the others are seeded uniform fills.
Plans are created inside the `with` block (none of these six switches is read at plan creation; "fp" and "pm64" are)."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import prime32, prime64, product
from test_product import _ref_primes

pytestmark = pytest.mark.gpu

P62, P63 = 4611686018427322369, 9223372036853661697
P50, P51 = 1125899904679937, 2251799813554177
SOLINAS, PM64 = 18446744069414584321, 18446744073707716609
P30, P31, P32 = 1062862849, 2147352577, 4293918721
LAZY, STRICT, FP, FP51, PM, FPW = 0, 1, 3, 4, 5, 6   # cntt_plan_info_t.arith_class


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.dtype("i%d" % a.dtype.itemsize)).copy()).cuda()


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _dtype(bits):
    return np.uint64 if bits == 64 else np.uint32


def _polys(oracle, count, n, p, seed, bits):
    """count polynomials: the first all p - 1, the others uniform below p"""
    x = oracle.fill_uniform(count * n, p, seed, bits)
    x[:n] = p - 1
    return x


def _add_mod(a, b, p):
    """(a + b) mod p on canonical words of one unsigned dtype, with the carry out of the word"""
    s = a + b
    return np.where((s < a) | (s >= a.dtype.type(p)), s - a.dtype.type(p), s)


def _new_plan(bits, n, p):
    plan = (prime64 if bits == 64 else prime32).Plan.try_new(n, p)
    assert plan is not None, (n, p)
    return plan


def _both(switches, run):
    """run(tag) under `switches` and under the defaults"""
    with cntt.debug_switches(**switches):
        run("%r" % (switches,))
    with cntt.debug_switches(**{k: -1 for k in switches}):
        run("default")


# ------------------------------------------------------------------------------------------------
# blk = 0: the plain transform kernels (one polynomial per workgroup) of the sizes whose default is the wave-block walk
# ------------------------------------------------------------------------------------------------
BLK_ROWS = [(64, n, p, cls, 5) for n in (4096, 8192, 16384)
            for p, cls in ((P62, LAZY), (P63, STRICT), (P50, FP), (P51, FP51), (PM64, PM), (SOLINAS, PM))]
BLK_ROWS += [(32, n, p, cls, 3) for n in (16384, 32768) for p, cls in ((P30, LAZY), (P31, STRICT), (P32, FPW))]


@pytest.mark.parametrize("bits,n,p,cls,batch", BLK_ROWS)
def test_gpu_blk_off_transforms(oracle, bits, n, p, cls, batch):
    """fwd_batch / inv_batch.  (The inverse of the 31-bit class at n = 16384 is the plain kernel under both values: the walk is
    not used there; its forward differs.)"""
    ref = oracle.Plan.try_new(n, p, bits)
    x = _polys(oracle, batch, n, p, 100 + n % 1000, bits)
    for name in ("fwd", "inv"):
        want = x.copy()
        getattr(ref, name + "_batch")(want, 4)

        def run(tag):
            plan = _new_plan(bits, n, p)
            assert plan.info().arith_class == cls     # the row runs the class it names
            d = _dev(x)
            getattr(plan, name + "_batch")(d)
            assert np.array_equal(_host(d, _dtype(bits)), want), (name, tag)

        _both({"blk": 0}, run)


# ------------------------------------------------------------------------------------------------
# mul32_blk = 0: MulOne for the 32-bit shapes whose fused product runs on the walk
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p,cls", [(16384, P30, LAZY), (32768, P30, LAZY), (32768, P31, STRICT), (16384, P32, FPW)])
def test_gpu_mul32_blk_off_fused_product(oracle, n, p, cls):
    ref = oracle.Plan.try_new(n, p, 32)
    for batch in (1, 3):
        a = _polys(oracle, batch, n, p, 210 + batch, 32)
        bn = _polys(oracle, batch, n, p, 220 + batch, 32)
        ref.fwd_batch(bn, 4)
        want = a.copy()
        ref.fwd_batch(want, 4)
        ref.mul_assign_normalize(want, bn)
        ref.inv_batch(want, 4)

        def run(tag):
            plan = _new_plan(32, n, p)
            assert plan.info().arith_class == cls
            d = _dev(a)
            plan.mul_ntt_batch(d, _dev(bn))
            assert np.array_equal(_host(d, np.uint32), want), (batch, tag)

        _both({"mul32_blk": 0}, run)


# ------------------------------------------------------------------------------------------------
# the mul_accumulate chain: ext32_blk, ext_one, ext_split
# ------------------------------------------------------------------------------------------------
def _chain_case(oracle, bits, n, p, J, O, batch):
    """terms, key, init and the oracle's fwd / mul_accumulate / inv sequence (tests/test_external_product.py: _expected) for
    both `accumulate` values.  Every [j][o] column of the key holds different values, so a wrong key or output stride of a
    split launch cannot cancel."""
    ref = oracle.Plan.try_new(n, p, bits)
    dt = _dtype(bits)
    terms = _polys(oracle, batch * J, n, p, 311 + n % 1000 + O, bits)
    key = _polys(oracle, J * O, n, p, 322 + n % 1000 + O, bits)
    init = oracle.fill_uniform(batch * O * n, p, 333 + n % 1000 + O, bits)
    init[:n] = p - 1
    tn = terms.copy()
    ref.fwd_batch(tn, 4)
    tn, kf = tn.reshape(batch, J, n), key.reshape(J, O, n)
    want = np.zeros((batch, O, n), dtype=dt)
    for b in range(batch):
        for o in range(O):
            acc = np.zeros(n, dtype=dt)
            for j in range(J):
                ref.mul_accumulate(acc, np.ascontiguousarray(tn[b, j]), np.ascontiguousarray(kf[j, o]))
            ref.inv(acc)
            want[b, o] = acc
    want = want.reshape(-1)
    return terms, key, init, {False: want, True: _add_mod(init, want, p)}


def _chain_row(oracle, switches, bits, n, p, cls, J, O, batch=2):
    terms, key, init, want = _chain_case(oracle, bits, n, p, J, O, batch)
    dt = _dtype(bits)

    def run(tag):
        plan = _new_plan(bits, n, p)
        assert plan.info().arith_class == cls
        for accumulate in (False, True):
            dout = _dev(init if accumulate else np.zeros_like(init))
            plan.external_product_batch(dout, _dev(terms), _dev(key), J, O, accumulate)
            assert np.array_equal(_host(dout, dt), want[accumulate]), (accumulate, tag)

    _both(switches, run)


@pytest.mark.parametrize("n,p,cls", [(16384, P30, LAZY), (16384, P32, FPW), (32768, P32, FPW)])
def test_gpu_ext32_blk_off_one_output_chain(oracle, n, p, cls):
    """ExtOne with one output where the default is the chain on the walk"""
    _chain_row(oracle, {"ext32_blk": 0}, 32, n, p, cls, 2, 1)


EXT_ONE_ROWS = [(n, p, cls, J, O) for n in (8192, 16384, 32768) for p, cls in ((P30, LAZY), (P31, STRICT), (P32, FPW))
                for J, O in ((2, 1), (3, 2)) + (((2, 4),) if n == 8192 else ())]


@pytest.mark.parametrize("n,p,cls,J,O", EXT_ONE_ROWS)
def test_gpu_ext_one_off_composed_chain(oracle, n, p, cls, J, O):
    """the composed pipeline (copy, batched forward, accumulate kernel, batched inverse) for 32-bit words above n = 4096"""
    _chain_row(oracle, {"ext_one": 0}, 32, n, p, cls, J, O)


@pytest.mark.parametrize("O", [3, 4])
@pytest.mark.parametrize("bits,n,p,cls", [(64, 16384, P62, LAZY), (64, 16384, P63, STRICT), (32, 32768, P31, STRICT), (32, 32768, P32, FPW)])
def test_gpu_ext_split_on_where_composed_is_the_default(oracle, bits, n, p, cls, O):
    """two fused launches of <= 2 outputs in the classes that compose by default; three outputs of the p >= 2^31 class end in the
    one-output kernel on the walk writing at output stride 3"""
    _chain_row(oracle, {"ext_split": 1}, bits, n, p, cls, 2, O)


@pytest.mark.parametrize("O", [3, 4])
@pytest.mark.parametrize("bits,n,p,cls", [(64, 16384, P50, FP), (64, 16384, P51, FP51), (64, 16384, SOLINAS, PM), (32, 32768, P30, LAZY)])
def test_gpu_ext_split_off_where_split_is_the_default(oracle, bits, n, p, cls, O):
    """the composed pipeline in the classes that split by default"""
    _chain_row(oracle, {"ext_split": 0}, bits, n, p, cls, 2, O)


# ------------------------------------------------------------------------------------------------
# product_fused: product::Plan of two u32 primes, fused / composed forward and inverse
# ------------------------------------------------------------------------------------------------
def _pair(oracle, n, shape):
    if shape == "u31x2":
        lp = oracle.largest_prime_in_arithmetic_progression64
        p0 = lp(2 * n, 1, 0, 2**31 - 1)
        return [p0, lp(2 * n, 1, 0, p0 - 1)]
    return _ref_primes(oracle, n, shape)


@pytest.mark.parametrize("n", [32, 512, 4096])
@pytest.mark.parametrize("shape,cls", [("u32x2", FPW), ("u30x2", LAZY), ("u31x2", STRICT)])
def test_gpu_product_fused_settings(oracle, shape, cls, n):
    """-1: composed forward, fused inverse; 0: neither fused; 1: both (the fused forward kernel and its Bounded fast path run under
    no other setting, the composed inverse of a one-class pair under none but 0).  Every call equals the oracle under each
    setting -- hence the settings agree --, including the ntt buffer that inv leaves behind."""
    primes = sorted(_pair(oracle, n, shape))
    big, batch = primes[0] * primes[1], 5
    oplan = oracle.Product.try_new(n, big, primes)
    assert oplan is not None
    dl = oplan.ntt_domain_len()
    assert dl == n
    std = oracle.fill_uniform(batch * n, big, 41 + n, 64)
    std[:n] = big - 1
    below, above = min(primes) - 1, max(primes) + 1      # Bounded: the fast path / the fall-back to `%`
    raw = oracle.fill_uniform(n, 2 * below - 1, 43 + n, 64)
    centred = np.array([(int(x) - below + 1) % big for x in raw], dtype=np.uint64)   # |value| < below
    init = oracle.fill_uniform(batch * n, big, 47 + n, 64)
    init[: 2 * n] = big - 1                                                          # the accumulating add wraps

    def ofwd(x, bound=None):
        t = np.zeros(dl, dtype=np.uint64)
        oplan.fwd(t, np.ascontiguousarray(x), bound)
        return t

    want_fwd = [ofwd(std[i * n:(i + 1) * n]) for i in range(batch)]
    want_bounded = {b: ofwd(centred, b) for b in (below, above)}
    assert np.array_equal(want_bounded[below], want_bounded[above]) and np.array_equal(want_bounded[below], ofwd(centred))
    want_inv = {}
    for acc in (False, True):
        for i in range(batch):
            s = init[i * n:(i + 1) * n].copy() if acc else np.zeros(n, dtype=np.uint64)
            t = want_fwd[i].copy()
            oplan.inv(s, t, acc)
            want_inv[acc, i] = (s, t)
    # plane-major batch buffers: u32 words [prime][polynomial][n]
    planes_fwd = np.stack([w.view(np.uint32).reshape(2, n) for w in want_fwd], axis=1).reshape(-1).view(np.uint64)

    for setting in (-1, 0, 1):
        with cntt.debug_switches(product_fused=setting):
            plan = product.Plan.try_new(n, big, primes)
            assert plan is not None and [q.info().arith_class for q in plan.plan_32()] == [cls, cls] and not plan.plan_64()
            got = np.zeros(dl, dtype=np.uint64)
            plan.fwd(got, std[:n].copy(), product.FwdMode.Generic)
            assert np.array_equal(got, want_fwd[0]), setting
            for b in (below, above):
                got = np.zeros(dl, dtype=np.uint64)
                plan.fwd(got, centred, product.FwdMode.Bounded(b))
                assert np.array_equal(got, want_bounded[b]), (setting, b)
            for acc, mode in ((False, product.InvMode.Replace), (True, product.InvMode.Accumulate)):
                s = init[:n].copy() if acc else np.zeros(n, dtype=np.uint64)
                t = want_fwd[0].copy()
                plan.inv(s, t, mode)
                assert np.array_equal(s, want_inv[acc, 0][0]) and np.array_equal(t, want_inv[acc, 0][1]), (setting, acc)
            dntt = _dev(np.zeros(dl * batch, dtype=np.uint64))
            plan.fwd_batch(dntt, _dev(std), product.FwdMode.Generic)
            assert np.array_equal(_host(dntt, np.uint64), planes_fwd), setting
            for acc, mode in ((False, product.InvMode.Replace), (True, product.InvMode.Accumulate)):
                ds, dt_ = _dev(init if acc else np.zeros_like(init)), _dev(planes_fwd)
                plan.inv_batch(ds, dt_, mode)
                hs, ht = _host(ds, np.uint64), _host(dt_, np.uint64).view(np.uint32).reshape(2, batch, n)
                for i in range(batch):
                    assert np.array_equal(hs[i * n:(i + 1) * n], want_inv[acc, i][0]), (setting, acc, i)
                    assert np.array_equal(ht[:, i, :].reshape(-1), want_inv[acc, i][1].view(np.uint32)), (setting, acc, i)
