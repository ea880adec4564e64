"""The range bookkeeping of the fused prime64 product at n = 1024 (csrc/ntt_kernel.hpp MulWp::run with JOIN, csrc/ntt_arith.hpp)
replayed in exact Python integers -- no GPU.  The device keeps 64-bit words; the kernel is right only if no intermediate that must not wrap
reaches 2^64 and every reduction meets the range it was written for.  The replay runs the device's own operation sequence

    forward:   stage on index bit b = 9 ... 0, twiddle entry 2^(9-b) + (e >> (b+1));  x <- csub_two_p(x) except in the first stage,
               t = shoup(y, w) in [0, 2p),  (x, y) <- (x + t, x - t + 2p)                         values below 4p, left as they are
    pointwise: u = hi(a b) + p - hi(m p),  m = lo(a b) p^-1 mod 2^64   (mul_fused_join)              in [1, 2p - 1]
    inverse:   stage on bit b = 0 ... 8:  (x, y) <- (csub_two_p(x + y), shoup(x + 2p - y, w))        both below 2p
               bit 9 (inv_norm_join): (x, y) <- (shoup(x + y, 2^64 / N), shoup(x + 2p - y, 2^64 w / N))   the sum goes in UNREDUCED
    finish:    csub_one_p                                                                            canonical

on whole arrays of unbounded integers, records the maximum of every intermediate stage by stage and asserts the bound written next to
each operation in the source.  The Shoup product is replayed as the device computes it (quotient floor(y ws / 2^64), ws = floor(w 2^64 / p))
and its TRUE value y w - q p is asserted to lie in [0, 2p) before it is taken modulo 2^64.  Primes and inputs are those of
test_gpu_fused_join_bounds.py; the result must also equal the oracle's fwd; mul_assign_normalize; inv, so the replay is the computation the
device is tested against and not a model of something else.  The twiddle tables are the oracle's own (Plan.table)."""
import numpy as np
import pytest

from random_cases import _search

N, LOGN = 1024, 10
W64 = 1 << 64
P62 = 4611686018427322369
SMALLEST_NAMED = 1152921504607338497   # tests/test_gpu_parity.py LAZY_ABOVE_POW2
PATTERNS = ("pm1", "zero", "alt", "delta0", "deltaN", "uniform")


def _primes():
    largest = _search(N, (1 << 62) - 1)
    floor = _search(N, (1 << 51) + (1 << 36))
    assert (1 << 51) < floor < SMALLEST_NAMED < P62 <= largest < (1 << 62)
    return [P62, SMALLEST_NAMED, largest, floor]


def obj(values):
    a = np.empty(len(values), dtype=object)
    a[:] = [int(v) for v in values]
    return a


class Replay:
    def __init__(self, oplan):
        self.p = p = int(oplan.p)
        self.tw, self.itw = obj(oplan.table("twid")), obj(oplan.table("inv_twid"))
        self.tws, self.itws = (self.tw << 64) // p, (self.itw << 64) // p
        n_inv = pow(N, -1, p)
        r = W64 % p
        # the inverse half runs on constants times 2^64 (mul_inv_params): the Montgomery product leaves a factor 2^-64
        self.mont_n_inv = n_inv * r % p
        self.mont_last_w = int(self.itw[1]) * n_inv * r % p
        self.pinv = pow(p, -1, W64)
        self.peak = {}

    def note(self, key, values, limit):
        m = int(values.max())
        self.peak[key] = max(self.peak.get(key, 0), m)
        assert m < limit, (key, m, limit)
        assert int(values.min()) >= 0, key

    def shoup(self, key, y, w, ws):
        self.note(key + " operand", y, W64)                 # shoup_core takes any word below 2^64 -- and nothing above
        q = (y * ws) >> 64
        t = y * w - q * self.p                              # the true value, before the device keeps its low 64 bits
        self.note(key + " product", t, 2 * self.p)
        return t

    def csub(self, key, x, m):
        self.note(key + " in", x, 2 * m)                    # csub_sign: x in [0, 2m), m < 2^63 -- the sign of x - m is the borrow
        assert 2 * m <= W64
        return np.where(x >= m, x - m, x)

    def forward(self, a):
        p = self.p
        a = a.copy()
        self.note("fwd input", a, p)
        idx = np.arange(N)
        for b in range(LOGN - 1, -1, -1):
            lo = idx[(idx >> b) & 1 == 0]
            hi = lo | (1 << b)
            ent = (1 << (LOGN - 1 - b)) + (lo >> (b + 1))
            x, y = a[lo], a[hi]
            if b != LOGN - 1:
                x = self.csub("fwd b=%d csub_two_p" % b, x, 2 * p)
            else:
                self.note("fwd b=%d x (canonical input, no csub)" % b, x, 2 * p)
            t = self.shoup("fwd b=%d" % b, y, self.tw[ent], self.tws[ent])
            a[lo], a[hi] = x + t, x - t + 2 * p
            self.note("fwd b=%d outputs" % b, a, min(4 * p, W64))
        return a

    def pointwise(self, a, b):
        p = self.p
        self.note("pointwise a", a, min(4 * p, W64))
        self.note("pointwise b", b, p)
        prod = a * b
        lo, hi = prod % W64, prod >> 64
        self.note("pointwise hi(a b)", hi, p)
        m = (lo * self.pinv) % W64
        mp = m * p
        assert all(int(v) == 0 for v in (mp - prod) % W64), "the low words must cancel exactly"
        q = mp >> 64
        self.note("pointwise hi(m p)", q, p)
        self.note("pointwise hi(a b) + p", hi + p, W64)
        u = hi + p - q
        self.note("pointwise u", u, 2 * p)
        assert int(u.min()) >= 1
        assert all(int(v) == 0 for v in (u * W64 - prod) % p), "u = a b 2^-64 mod p"
        return u

    def inverse(self, a):
        p = self.p
        a = a.copy()
        idx = np.arange(N)
        for b in range(LOGN):
            lo = idx[(idx >> b) & 1 == 0]
            hi = lo | (1 << b)
            ent = (1 << (LOGN - 1 - b)) + (lo >> (b + 1))
            x, y = a[lo], a[hi]
            self.note("inv b=%d inputs" % b, a, 2 * p)
            d = x + 2 * p - y
            self.note("inv b=%d x + 2p - y" % b, d, min(4 * p, W64))
            s = x + y
            self.note("inv b=%d x + y" % b, s, min(4 * p, W64))
            if b < LOGN - 1:
                a[lo] = self.csub("inv b=%d csub_two_p" % b, s, 2 * p)
                a[hi] = self.shoup("inv b=%d" % b, d, self.itw[ent], self.itws[ent])
            else:   # inv_norm_join: no reduction between the sum and its product
                assert all(int(e) == 1 for e in ent)
                a[lo] = self.shoup("inv b=%d sum / N" % b, s, self.mont_n_inv, (self.mont_n_inv << 64) // p)
                a[hi] = self.shoup("inv b=%d difference w / N" % b, d, self.mont_last_w, (self.mont_last_w << 64) // p)
        a = self.csub("finish csub_one_p", a, p)
        self.note("output", a, p)
        return a


def _pattern(oracle, name, p, seed):
    out = np.zeros(N, dtype=np.uint64)
    if name == "pm1":
        out[:] = p - 1
    elif name == "alt":
        out[1::2] = p - 1
    elif name == "delta0":
        out[0] = p - 1
    elif name == "deltaN":
        out[N - 1] = p - 1
    elif name == "uniform":
        out[:] = oracle.fill_uniform(N, p, seed, 64)
    return out


@pytest.mark.parametrize("which", range(4), ids=["headline", "smallest-named", "largest", "class-floor"])
def test_no_intermediate_reaches_two_to_the_64_and_outputs_are_canonical(oracle, which):
    p = _primes()[which]
    assert 4 * p < W64, "the lazy class: p < 2^62"
    oplan = oracle.Plan.try_new(N, p, 64)
    rp = Replay(oplan)
    lhs = {k: _pattern(oracle, k, p, 0x1700 + i) for i, k in enumerate(PATTERNS)}
    rhs = {k: _pattern(oracle, k, p, 0x1780 + i) for i, k in enumerate(PATTERNS)}
    for ka in PATTERNS:
        a_ntt = rp.forward(obj(lhs[ka]))
        want_ntt = lhs[ka].copy()
        oplan.fwd(want_ntt)
        assert all(int(g) % p == int(w) for g, w in zip(a_ntt, want_ntt)), ("forward residues", ka)
        for kb in PATTERNS:
            got = rp.inverse(rp.pointwise(a_ntt, obj(rhs[kb])))
            want = want_ntt.copy()
            oplan.mul_assign_normalize(want, rhs[kb].copy())
            oplan.inv(want)
            assert [int(v) for v in got] == [int(v) for v in want], ("replay vs oracle", p, ka, kb)
    # the extremes the inputs were chosen for are really met: the unreduced sum of the last inverse stage passes 2p (the reduction that
    # is gone would have fired); the pointwise product sees a above 2p
    assert rp.peak["inv b=9 sum / N operand"] >= 2 * p
    assert rp.peak["pointwise a"] >= 2 * p
    assert rp.peak["pointwise u"] >= p
    assert max(rp.peak.values()) < W64
