"""What a _batch call writes, and what it must not: every operand of every call below is an exact-size slice of ONE arena with a band
of position-dependent pattern words before and after it (tests/guard_arena.py), as a caller has them who carves its buffers out of one
allocation (the Rust shim, examples/multi_device.cpp).  Whole test tensors hide a store past the end in the allocator's padding; here it
lands in a band or in a neighbour.  Each case asserts
  * the written slices bit-exact against the CPU oracle (the chain calls: the oracle's fwd / mul_accumulate / inv in sequence);
  * every band word and every read-only operand byte for byte what it was (GuardArena.check).
The band behind a written operand holds a full workgroup's worth of polynomials of the serving kernel and at least 64 (guard_polys).

Shapes: n = 16, 32 and one size per kernel family -- LDS-resident walk (n = 1024), wave-block walk (u64 n = 4096, u32 n = 8192 / 16384), the
single-pass size past LDS (u64 n = 32768), global stages (u64 n = 32768 in the Montgomery class, u32 n = 65536) -- and every arithmetic
class once at n = 64.  Batches: 1, 3, PPB - 1 and PPB + 1 of the serving kernel (restated from the launch code by
test_gpu_multitrip_transforms.transform_shape / mul_shape and ext_ppb below), and the smallest row of that module's table over several
trips of the persistent grid.  Slices start 16-byte aligned and, in a second parametrisation, one word past a 16-byte boundary: u32 at
4-byte, u64 at 8-byte alignment, all that include/cntt.h ("Operands") asks for.

The pointwise kernel's scalar tail: n is a multiple of the vector width, so a _batch call never has a tail and no public call runs it on
caller-visible device memory.  The host-slice calls, which take any length, do reach it (test_host_slice_scalar_tail: 1 and 3 words, the whole
call in the tail, and 35), but on the library's own staging copies: that test checks the tail's VALUES and the byte counts of the copies in
and out, not the kernel's footprint -- a stray device store would land in the staging allocation, out of sight.  What guards the tail loop is
every device case here: with a count that is a multiple of the vector width the loop must run zero times, and a bound one word too wide
writes the first band word.

The later headers (cntt_ext.h, cntt_gadget.h, cntt_pbs.h, cntt_prime_pbs.h): one small case per call at the end of this file, the
caller's workspace a written slice of the arena with bands of its own.  The calls on LWE ciphertexts (cntt_keyswitch.h,
cntt_prime_keyswitch.h, cntt_pack.h, cntt_prime_pack.h) follow in tests/test_gpu_footprint_lwe.py, which takes guard, guard_both, Family,
_dev and batches_of from here."""
import numpy as np
import pytest

from guard_arena import GuardArena, trailing_guard
from test_gpu_multitrip_transforms import (LAZY, P30, P62, PRIMES, cus, img_entries, make_plans, mul_shape, multitrip_batch, prime_of, sched, tpp,
                                           transform_shape)
from test_product import _ref_primes

pytestmark = pytest.mark.gpu


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def guard_polys(bits, n):
    """an upper bound of PPB for every kernel that serves (bits, n): no workgroup has more than 1024 threads and a polynomial takes at
    least the fewest threads any schedule family gives it"""
    logn = n.bit_length() - 1
    t = min(tpp(bits, logn, inv, fam) for inv in (False, True) for fam in (0, 1, 2)) if logn <= (15 if bits == 32 else 14) else 1024
    return max(1, 1024 // t)


def guard(bits, n, words_per_coeff=1):
    return trailing_guard(n, guard_polys(bits, n), words_per_coeff)


def guard_both(n, words_per_coeff=1):
    """the band behind a value or NTT-domain operand of the native and product plans: their kernels run the 32-bit schedules on the
    residues, and 64-bit per-prime kernels where a plan has u64 primes, so the larger of the two widths' bands"""
    return max(guard(32, n, words_per_coeff), guard(64, n, words_per_coeff))


def ext_ppb(bits, n):
    """ExtWp::PPB of the chain kernel (csrc/ntt_ext_inst.inc ext_one_fam, ExtShape): 256 threads, 512 when the twiddle image is past 16 KiB"""
    logn, w = n.bit_length() - 1, bits // 8
    if logn > (12 if bits == 32 else 11) or sched(bits, logn, False)["NPASS"] == 1:
        return 1
    block = 256 if img_entries(bits, logn, False) * 2 * w <= 16384 else 512
    return max(1, min(block // tpp(bits, logn, False, f) for f in (0, 1)))


def batches_of(ppbs):
    out = {1, 3}
    for q in ppbs:
        if q > 1:
            out |= {q - 1, q + 1}
    return sorted(out)


def prime_batches(bits, n, cls, op):
    ncu = cus()
    if n.bit_length() - 1 > (15 if bits == 32 else 14):   # past LDS: the single-pass kernel or global stages, one polynomial per workgroup
        return [1, 2, 3]
    if op in ("fwd", "inv"):
        return batches_of([transform_shape(bits, n, cls, op == "inv", ncu)[2]])
    if op == "mul_ntt":
        return batches_of([mul_shape(bits, n, cls, ncu)[2]])
    if op == "ext":
        return batches_of([ext_ppb(bits, n)])
    return [1, 3]   # pointwise: grid-stride over words, no polynomial slots


def add_mod(a, b, p):
    if a.dtype == np.uint32:
        return ((a.astype(np.uint64) + b.astype(np.uint64)) % np.uint64(p)).astype(np.uint32)
    with np.errstate(over="ignore"):
        s = a + b
        return np.where((s < a) | (s >= np.uint64(p)), s - np.uint64(p), s)


def ext_expected(oplan, terms, key, init, n, J, O, batch, p, accumulate):
    """fwd; mul_accumulate; inv in sequence (src/prime64.rs:794, :1085-1128, :872), out[b][o] (+)= that"""
    tn = terms.copy()
    oplan.fwd_batch(tn)
    tn, kf = tn.reshape(batch, J, n), key.reshape(J, O, n)
    out = np.zeros((batch, O, n), dtype=terms.dtype)
    for o in range(O):
        acc = np.zeros(batch * n, dtype=terms.dtype)
        for j in range(J):   # mul_accumulate is word by word: one call takes term j of every element against key[j][o]
            oplan.mul_accumulate(acc, np.ascontiguousarray(tn[:, j, :]).reshape(-1), np.tile(kf[j, o], batch))
        out[:, o, :] = acc.reshape(batch, n)
    out = np.ascontiguousarray(out).reshape(-1)
    oplan.inv_batch(out)
    return add_mod(out, init, p) if accumulate else out


# ---- one call of the prime family on an arena ----------------------------------------------------------------------------------------
EXT_FULL = [(O, acc) for O in (1, 2, 3) for acc in (0, 1)]
EXT_SOME = [(2, 0), (1, 1), (3, 1)]


def run_prime(oracle, plan, oplan, bits, n, p, op, batch, odd, device=True, ext=EXT_SOME, J=2, same=False):
    dt = np.uint64 if bits == 64 else np.uint32
    seed = 0x5EED + bits + 3 * n + 7 * batch + (1 if odd else 0)
    g = guard(bits, n)
    a = oracle.fill_uniform(batch * n, p, seed + 1, bits)
    b = oracle.fill_uniform(batch * n, p, seed + 2, bits)
    c = oracle.fill_uniform(batch * n, p, seed + 3, bits)
    a[:n] = p - 1   # the first polynomial at the range edge
    tag = (op, bits, n, batch, "odd" if odd else "aligned", "device" if device else "host")

    def arena():
        return GuardArena(dt, device, seed, odd)

    if op in ("fwd", "inv", "normalize"):
        ar = arena().take("a", a, written=True, guard=g).build()
        getattr(plan, op + "_batch")(ar["a"])
        want = a.copy()
        {"fwd": oplan.fwd_batch, "inv": oplan.inv_batch, "normalize": oplan.normalize}[op](want)
        assert np.array_equal(ar.check()["a"], want), tag
    elif op in ("mul_assign_normalize", "mul_ntt"):
        ar = arena().take("a", a, written=True, guard=g).take("b", b).build()
        getattr(plan, op + "_batch")(ar["a"], ar["b"])
        want = a.copy()
        if op == "mul_ntt":
            oplan.fwd_batch(want)
        oplan.mul_assign_normalize(want, b)
        if op == "mul_ntt":
            oplan.inv_batch(want)
        assert np.array_equal(ar.check()["a"], want), tag
    elif op == "mul_accumulate":
        ar = arena().take("a", a, written=True, guard=g).take("b", b)
        if not same:
            ar.take("c", c)
        ar.build()
        plan.mul_accumulate_batch(ar["a"], ar["b"], ar["b" if same else "c"])
        want = a.copy()
        oplan.mul_accumulate(want, b, b if same else c)
        assert np.array_equal(ar.check()["a"], want), tag
    elif op == "ext":
        for (O, accumulate) in ext:
            terms = oracle.fill_uniform(batch * J * n, p, seed + 4, bits)
            key = oracle.fill_uniform(J * O * n, p, seed + 5, bits)
            init = oracle.fill_uniform(batch * O * n, p, seed + 6, bits)
            # key_ntt first: it coincides with nothing, and a store that falls short of `out` lands in it or in its band
            ar = arena().take("key", key).take("out", init if accumulate else batch * O * n, written=True, guard=g).take("terms", terms).build()
            plan.external_product_batch(ar["out"], ar["terms"], ar["key"], J, O, bool(accumulate))
            want = ext_expected(oplan, terms, key, init, n, J, O, batch, p, accumulate)
            assert np.array_equal(ar.check()["out"], want), tag + (O, accumulate)
    else:
        raise KeyError(op)


OPS = ["fwd", "inv", "mul_assign_normalize", "normalize", "mul_accumulate", "mul_ntt", "ext"]
# (bits, n, name, p, cls): one lazy prime per size, the Montgomery class where the size past LDS takes global stages
SIZE_CASES = [(64, n, "lazy", P62, LAZY) for n in (16, 32, 1024, 4096, 32768)] + [(64, 32768, "generic", None, 2)] + [
    (32, n, "lazy", P30, LAZY) for n in (32, 1024, 8192, 16384, 65536)]
CLASS_CASES = [(bits, 64, name, p, cls) for (bits, name, p, cls) in PRIMES]


def _ids(cases):
    return ["u%d-%s-n%d" % (b, nm, n) for (b, n, nm, _, _) in cases]


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits,n,name,p,cls", SIZE_CASES, ids=_ids(SIZE_CASES))
def test_prime_footprint_sizes(oracle, bits, n, name, p, cls, op, odd):
    import torch
    p = prime_of(oracle, p)
    plan, oplan = make_plans(oracle, bits, n, p, cls)
    ext = EXT_FULL if n == 1024 else EXT_SOME
    for batch in prime_batches(bits, n, cls, op):
        run_prime(oracle, plan, oplan, bits, n, p, op, batch, odd, ext=ext)
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("bits,n,name,p,cls", CLASS_CASES, ids=_ids(CLASS_CASES))
def test_prime_footprint_classes(oracle, bits, n, name, p, cls, op):
    p = prime_of(oracle, p)
    plan, oplan = make_plans(oracle, bits, n, p, cls)
    for batch in prime_batches(bits, n, cls, op):
        run_prime(oracle, plan, oplan, bits, n, p, op, batch, odd=(batch % 2 == 1), ext=EXT_FULL)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("op", ["fwd", "inv", "mul_ntt"])
def test_prime_footprint_multitrip(oracle, op, odd):
    """the smallest row of test_gpu_multitrip_transforms' table (u64, n = 16, lazy class): two rounds of the persistent grid and a ragged tail"""
    bits, n, p, cls = 64, 16, P62, LAZY
    plan, oplan = make_plans(oracle, bits, n, p, cls)
    batch, _ = multitrip_batch(bits, n, cls, p, cus())
    run_prime(oracle, plan, oplan, bits, n, p, op, batch, odd)


@pytest.mark.parametrize("bits,p", [(64, P62), (32, P30)], ids=["u64", "u32"])
@pytest.mark.parametrize("op", OPS)
def test_prime_footprint_host_path(oracle, bits, p, op):
    """CNTT_MEM_HOST: the copies in and out move word counts computed on the host; numpy arenas, n = 32, batch 3, odd word offsets"""
    plan, oplan = make_plans(oracle, bits, 32, p, LAZY)
    run_prime(oracle, plan, oplan, bits, 32, p, op, 3, odd=True, device=False, ext=EXT_FULL)


@pytest.mark.parametrize("bits,p", [(64, P62), (32, P30)], ids=["u64", "u32"])
@pytest.mark.parametrize("count", [1, 3, 35])
def test_host_slice_scalar_tail(oracle, bits, p, count):
    """mul_assign_normalize / normalize / mul_accumulate of `count` words through the host-slice calls: 1 and 3 words are below the vector
    width of u32 (1 of u64), so the whole call is the pointwise kernel's scalar tail; 35 is vectors and a tail.  The kernel works on staging
    copies, so the bands here see the copy back (its byte count), not the kernel's stores: the values are what this test pins."""
    plan, oplan = make_plans(oracle, bits, 32, p, LAZY)
    dt = np.uint64 if bits == 64 else np.uint32
    a, b, c = (oracle.fill_uniform(count, p, 900 + i + count, bits) for i in range(3))
    for op in ("mul_assign_normalize", "normalize", "mul_accumulate"):
        ar = GuardArena(dt, False, 77 + count, odd=True).take("a", a, written=True).take("b", b).take("c", c).build()
        want = a.copy()
        if op == "normalize":
            plan.normalize(ar["a"])
            oplan.normalize(want)
        elif op == "mul_assign_normalize":
            plan.mul_assign_normalize(ar["a"], ar["b"])
            oplan.mul_assign_normalize(want, b)
        else:
            plan.mul_accumulate(ar["a"], ar["b"], ar["c"])
            oplan.mul_accumulate(want, b, c)
        assert np.array_equal(ar.check()["a"], want), (op, bits, count)


# ---- operand identity (include/cntt.h, "Operands"): read-only operands may be one buffer ---------------------------------------------
@pytest.mark.parametrize("bits,n,p", [(64, 64, P62), (64, 1024, P62), (32, 64, P30), (32, 1024, P30)])
def test_mul_accumulate_same_lhs_and_rhs(oracle, bits, n, p):
    plan, oplan = make_plans(oracle, bits, n, p, LAZY)
    for batch in (1, 3):
        run_prime(oracle, plan, oplan, bits, n, p, "mul_accumulate", batch, odd=False, same=True)
        run_prime(oracle, plan, oplan, bits, n, p, "mul_accumulate", batch, odd=True, same=True, device=False)


# ---- native plans ----------------------------------------------------------------------------------------------------------------------
def native_plans(oracle, kind, n):
    import concrete_ntt_amd as cntt
    mod = getattr(cntt, kind)
    plan, oplan = mod.Plan32.try_new(n), oracle.Native.try_new(kind + "_plan32", n)
    assert plan is not None and oplan is not None, (kind, n)
    return plan, oplan


def ppb32(n):
    """whole products / transforms per 256-thread workgroup of the u32 kernels (csrc/native_fused_inst.inc, product_fused_inst.hip)"""
    return max(1, 256 // tpp(32, n.bit_length() - 1, False))


def native_words(oplan, batch, seed, small=False):
    wpc = 2 if oplan.word == 16 else 1
    v = np.array(np.random.default_rng(seed).integers(0, 2**63, size=batch * oplan.n * wpc, dtype=np.uint64) * 2 + 1)
    v[:wpc] = np.iinfo(np.uint64).max
    if small:
        v &= np.uint64(1)
    return v.astype(np.uint32) if oplan.word == 4 else v


# u128 words are 16-byte aligned (include/cntt.h, "Operands"): the native128 cases have no odd offset to run
NATIVE_T = [(k, n, odd) for (k, n) in [("native32", 32), ("native64", 32), ("native64", 2048), ("native128", 32), ("native_binary64", 32),
                                       ("native_binary64", 2048)] for odd in (False, True) if not (odd and k == "native128")]


@pytest.mark.parametrize("kind,n,odd", NATIVE_T, ids=["%s-n%d-%s" % (k, n, "odd" if o else "aligned") for (k, n, o) in NATIVE_T])
def test_native_transform_footprint(oracle, kind, n, odd):
    """fwd_batch / fwd_binary_batch / inv_batch: the value in one arena, every residue plane carved from a second one (u32 residues),
    back to back with a band between the planes"""
    plan, oplan = native_plans(oracle, kind, n)
    wpc = 2 if oplan.word == 16 else 1
    vdt = np.uint32 if oplan.word == 4 else np.uint64
    k = oplan.nprimes
    pp = transform_shape(32, n, LAZY, False, cus())[2]
    for batch in batches_of([pp]):
        value = native_words(oplan, batch, 11 * n + batch)
        want_res = [np.zeros(batch * n, dtype=np.uint32) for _ in range(k)]
        for b in range(batch):
            r = oplan.residues()
            oplan.fwd(np.ascontiguousarray(value[b * n * wpc:(b + 1) * n * wpc]), r)
            for i in range(k):
                want_res[i][b * n:(b + 1) * n] = r[i]
        modes = [False] + ([True] if oplan.binary else [])
        for binary in modes:
            v = value & np.array(1, dtype=value.dtype) if binary else value
            va = GuardArena(vdt, True, 5 + batch, odd).take("value", v).build()
            ra = GuardArena(np.uint32, True, 6 + batch, odd)
            for i in range(k):
                ra.take("r%d" % i, batch * n, written=True, guard=guard(32, n))
            ra.build()
            plan.fwd_batch(va["value"], [ra["r%d" % i] for i in range(k)], binary=binary)
            va.check()
            got = ra.check()
            if binary:
                for b in range(batch):
                    r = oplan.residues()
                    oplan.fwd_binary(np.ascontiguousarray(v[b * n * wpc:(b + 1) * n * wpc]), r)
                    for i in range(k):
                        assert np.array_equal(got["r%d" % i][b * n:(b + 1) * n], r[i]), (kind, n, batch, "fwd_binary", i, b)
            else:
                for i in range(k):
                    assert np.array_equal(got["r%d" % i], want_res[i]), (kind, n, batch, "fwd", i)
        # inv: the planes are transformed in place and the value is written
        va = GuardArena(vdt, True, 7 + batch, odd).take("value", batch * n * wpc, written=True, guard=guard_both(n, wpc)).build()
        ra = GuardArena(np.uint32, True, 8 + batch, odd)
        for i in range(k):
            ra.take("r%d" % i, want_res[i], written=True, guard=guard(32, n))
        ra.build()
        plan.inv_batch(va["value"], [ra["r%d" % i] for i in range(k)])
        got_v, got_r = va.check()["value"], ra.check()
        for b in range(batch):
            r = [np.ascontiguousarray(want_res[i][b * n:(b + 1) * n]) for i in range(k)]
            w = oplan.words()
            oplan.inv(w, r)
            assert np.array_equal(got_v[b * n * wpc:(b + 1) * n * wpc], w), (kind, n, batch, "inv value", b)
            for i in range(k):
                assert np.array_equal(got_r["r%d" % i][b * n:(b + 1) * n], r[i]), (kind, n, batch, "inv residues", i, b)


POLYMUL = [(k, n, acc, odd) for (k, n, acc) in [("native32", 32, None), ("native32", 1024, None), ("native64", 32, 1), ("native64", 1024, 1),
                                                ("native64", 1024, 0), ("native64", 16384, 1), ("native128", 32, None),
                                                ("native128", 1024, None)] for odd in (False, True) if not (odd and k == "native128")]


@pytest.mark.parametrize("kind,n,acc,odd", POLYMUL, ids=["%s-n%d-acc%s-%s" % (k, n, a, "odd" if o else "aligned") for (k, n, a, o) in POLYMUL])
def test_native_polymul_footprint(oracle, kind, n, acc, odd):
    """negacyclic_polymul_batch: u32, u64 (both settings of the native_acc switch; n = 16384 parks tiles in the plan's workspace) and u128
    words; the last batch squares: prod = a (*) a with lhs and rhs the SAME buffer"""
    import concrete_ntt_amd as cntt
    plan, oplan = native_plans(oracle, kind, n)
    wpc = 2 if oplan.word == 16 else 1
    vdt = np.uint32 if oplan.word == 4 else np.uint64
    batches = batches_of([ppb32(n)]) if n < 16384 else [1, 3]
    try:
        if acc is not None:
            cntt.debug_set("native_acc", acc)
        for batch in batches:
            for same in ((False, True) if batch == 3 else (False,)):
                lhs, rhs = native_words(oplan, batch, 21 * n + batch), native_words(oplan, batch, 22 * n + batch)
                ar = GuardArena(vdt, True, 9 + batch, odd).take("lhs", lhs)
                ar.take("prod", batch * n * wpc, written=True, guard=guard_both(n, wpc))
                if not same:
                    ar.take("rhs", rhs)
                ar.build()
                plan.negacyclic_polymul_batch(ar["prod"], ar["lhs"], ar["lhs" if same else "rhs"])
                want = np.zeros_like(lhs)
                oplan.negacyclic_polymul_batch(want, lhs, lhs if same else rhs, batch)
                assert np.array_equal(ar.check()["prod"], want), (kind, n, acc, batch, same)
    finally:
        cntt.debug_set("reset", 0)


# ---- product::Plan -----------------------------------------------------------------------------------------------------------------------
def product_plans(oracle, shape, n):
    from concrete_ntt_amd import product
    primes = sorted(_ref_primes(oracle, n, shape))
    big = 1
    for q in primes:
        big *= q
    plan, oplan = product.Plan.try_new(n, big, primes), oracle.Product.try_new(n, big, primes)
    assert plan is not None and oplan is not None and plan.primes() == primes
    return plan, oplan, primes, big


def planes_of(polys, n, n32, n64):
    """plane-major batch buffer (include/cntt.h) out of one reference-layout ntt buffer per polynomial"""
    batch = len(polys)
    w32 = np.zeros((n32, batch, n), dtype=np.uint32)
    w64 = np.zeros((n64, batch, n), dtype=np.uint64)
    for i, x in enumerate(polys):
        if n32:
            w32[:, i, :] = x[:(n // 2) * n32].view(np.uint32).reshape(n32, n)
        if n64:
            w64[:, i, :] = x[(n // 2) * n32:].reshape(n64, n)
    return np.concatenate([w32.reshape(-1).view(np.uint64), w64.reshape(-1)])


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("shape,n", [("u30x2", 32), ("u30x2", 1024), ("u32x2_u64x1", 32), ("u32x2_u64x1", 1024)])
def test_product_footprint(oracle, shape, n, odd):
    """fwd, inv (Replace and Accumulate; it writes BOTH of its buffers), the three pointwise calls and the external product on the
    two-u32-prime fused shape and a mixed u32 + u64 plan; NTT-domain operands plane-major"""
    from concrete_ntt_amd import product
    plan, oplan, primes, big = product_plans(oracle, shape, n)
    n32 = sum(q < 2**32 for q in primes)
    n64 = len(primes) - n32
    dl = plan.ntt_domain_len()
    gs, gd = guard_both(n), guard_both(n) // n * dl   # the same count of polynomials behind a standard and an NTT-domain operand

    def arena(seed):
        return GuardArena(np.uint64, True, seed, odd)

    for batch in batches_of([ppb32(n)]):
        std = oracle.fill_uniform(batch * n, big, 31 + batch, 64)
        std2 = oracle.fill_uniform(batch * n, big, 32 + batch, 64)
        std[0] = big - 1
        fa, fb = [], []
        for i in range(batch):
            x, y = np.zeros(dl, dtype=np.uint64), np.zeros(dl, dtype=np.uint64)
            oplan.fwd(x, np.ascontiguousarray(std[i * n:(i + 1) * n]))
            oplan.fwd(y, np.ascontiguousarray(std2[i * n:(i + 1) * n]))
            fa.append(x)
            fb.append(y)
        pa, pb = planes_of(fa, n, n32, n64), planes_of(fb, n, n32, n64)
        tag = (shape, n, batch, odd)
        # fwd
        ar = arena(1).take("ntt", batch * dl, written=True, guard=gd).take("std", std).build()
        plan.fwd_batch(ar["ntt"], ar["std"])
        assert np.array_equal(ar.check()["ntt"], pa), tag + ("fwd",)
        # pointwise
        for op in ("mul_assign_normalize", "normalize", "mul_accumulate"):
            ar = arena(2).take("a", pa, written=True, guard=gd).take("b", pb).take("c", pa).build()
            want = []
            for i in range(batch):
                x = fa[i].copy()
                if op == "normalize":
                    oplan.normalize(x)
                elif op == "mul_assign_normalize":
                    oplan.mul_assign_normalize(x, fb[i])
                else:
                    oplan.mul_accumulate(x, fb[i], fa[i])
                want.append(x)
            if op == "normalize":
                plan.normalize_batch(ar["a"])
            elif op == "mul_assign_normalize":
                plan.mul_assign_normalize_batch(ar["a"], ar["b"])
            else:
                plan.mul_accumulate_batch(ar["a"], ar["b"], ar["c"])
            assert np.array_equal(ar.check()["a"], planes_of(want, n, n32, n64)), tag + (op,)
        # mul_accumulate(acc, x, x): lhs and rhs the same buffer
        ar = arena(3).take("a", pa, written=True, guard=gd).take("b", pb).build()
        plan.mul_accumulate_batch(ar["a"], ar["b"], ar["b"])
        want = []
        for i in range(batch):
            x = fa[i].copy()
            oplan.mul_accumulate(x, fb[i], fb[i])
            want.append(x)
        assert np.array_equal(ar.check()["a"], planes_of(want, n, n32, n64)), tag + ("mul_accumulate same",)
        # inv, both modes
        for accumulate in (False, True):
            init = oracle.fill_uniform(batch * n, big, 33 + batch, 64)
            ar = arena(4).take("ntt", pa, written=True, guard=gd).take("std", init if accumulate else batch * n, written=True, guard=gs).build()
            plan.inv_batch(ar["std"], ar["ntt"], product.InvMode.Accumulate if accumulate else product.InvMode.Replace)
            got = ar.check()
            ws, wn = [], []
            for i in range(batch):
                s = init[i * n:(i + 1) * n].copy() if accumulate else np.zeros(n, dtype=np.uint64)
                x = fa[i].copy()
                oplan.inv(s, x, accumulate)
                ws.append(s)
                wn.append(x)
            assert np.array_equal(got["std"], np.concatenate(ws)), tag + ("inv", accumulate)
            assert np.array_equal(got["ntt"], planes_of(wn, n, n32, n64)), tag + ("inv leaves the residues", accumulate)
    # external product: batch 3, two terms, two outputs, against fwd / mul_accumulate / inv of the oracle
    batch, J, O = 3, 2, 2
    terms = oracle.fill_uniform(batch * J * n, big, 41, 64)
    kstd = oracle.fill_uniform(J * O * n, big, 42, 64)
    kf = []
    for i in range(J * O):
        x = np.zeros(dl, dtype=np.uint64)
        oplan.fwd(x, np.ascontiguousarray(kstd[i * n:(i + 1) * n]))
        kf.append(x)
    for accumulate in (False, True):
        init = oracle.fill_uniform(batch * O * n, big, 43, 64)
        ar = arena(5).take("key", planes_of(kf, n, n32, n64)).take("out", init if accumulate else batch * O * n, written=True, guard=gs)
        ar.take("terms", terms).build()
        plan.external_product_batch(ar["out"], ar["terms"], ar["key"], J, O, product.FwdMode.Generic,
                                    product.InvMode.Accumulate if accumulate else product.InvMode.Replace)
        want = []
        for b in range(batch):
            for o in range(O):
                acc = np.zeros(dl, dtype=np.uint64)
                for j in range(J):
                    t = np.zeros(dl, dtype=np.uint64)
                    oplan.fwd(t, np.ascontiguousarray(terms[(b * J + j) * n:(b * J + j + 1) * n]))
                    oplan.mul_accumulate(acc, t, kf[j * O + o])
                s = init[(b * O + o) * n:(b * O + o + 1) * n].copy() if accumulate else np.zeros(n, dtype=np.uint64)
                oplan.inv(s, acc, accumulate)
                want.append(s)
        assert np.array_equal(ar.check()["out"], np.concatenate(want)), (shape, n, "external_product", accumulate)


# ---- the later headers: cntt_ext.h, cntt_gadget.h, cntt_pbs.h, cntt_prime_pbs.h --------------------------------------------------------
# One small case per call.  Words live in an arena of the plan's word type, rotation exponents and the native plans' key residue planes
# in a u32 arena, and a caller workspace is a written slice with bands of its own: its content belongs to the call, its bands do not.
# References: the integer models of the files that own each call, the oracle's negacyclic_polymul for the external product, and for the
# blind rotation and the bootstrap the per-iteration / per-step public calls on plain tensors (pinned to the models by those files).
class Family:
    """what the native64 plan and the prime plans differ in, for the cases below"""

    def __init__(self, name, n):
        import test_gpu_native_pbs as tnp
        import test_gpu_prime_pbs as tpp_
        import test_prime_pbs_model as pm
        self.name, self.n, self.native = name, n, name == "native64"
        if self.native:
            from concrete_ntt_amd import native64
            self.plan, self.p, self.bits, self.beta = native64.Plan32.try_new(n), 1 << 64, 64, 6
            self.model_modswitch = lambda lwe, L, batch: tnp.model_modswitch(lwe, L, batch, 64, n.bit_length() - 1)
            self.model_extract = lambda glwe, h: tnp.model_extract(glwe, h, 64)
        else:
            self.p = P62 if name == "prime64" else P30
            self.plan, self.bits, self.beta = tpp_.make_plan(self.p, n), 64 if name == "prime64" else 32, 7
            self.model_modswitch = lambda lwe, L, batch: pm.model_modswitch(lwe, L, batch, self.p, n.bit_length() - 1)
            self.model_extract = lambda glwe, h: pm.model_extract(glwe, h, self.p)
        assert self.plan is not None
        self.dt = np.uint64 if self.bits == 64 else np.uint32
        self.tnp, self.tpp = tnp, tpp_

    def words(self, rng, count):
        return rng.integers(0, self.p, size=count, dtype=np.uint64).astype(self.dt)

    def arena(self, seed, odd):
        return GuardArena(self.dt, True, seed, odd)

    def key(self, torch, rng, npoly, odd):
        """(the key argument of the calls with every part of it a read-only arena slice, the arenas to check, the same key on plain
        tensors for the reference)"""
        kw = self.words(rng, npoly * self.n)
        if not self.native:
            ar = self.arena(91, odd).take("bsk", kw).build()       # any canonical words do for a comparison with the public calls
            return ar["bsk"], [ar], self.tpp.dev(torch, kw)
        plain = self.tnp.key_planes(torch, self.plan, kw)
        ar = GuardArena(np.uint32, True, 92, odd)
        for i, t in enumerate(plain):
            ar.take("k%d" % i, self.tnp.host(t, np.uint32))
        ar.build()
        return [ar["k%d" % i] for i in range(len(plain))], [ar], plain

    def reference_rotation(self, torch, lut_t, rot_t, key, L, k, ell, batch):
        if self.native:
            return self.tnp.per_iteration_references(torch, self.plan, lut_t, False, rot_t, key, L, k, self.beta, ell, batch)[0]
        return self.tpp.per_iteration_reference(torch, self.plan, self.p, lut_t, False, rot_t, key, L, k, self.beta, ell, batch)


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


FAMILIES = [(f, odd) for f in ("native64", "prime64", "prime32") for odd in (False, True)]
FAM_IDS = ["%s-%s" % (f, "odd" if o else "aligned") for (f, o) in FAMILIES]
PBS_N, PBS_L, PBS_K, PBS_ELL, PBS_BATCH = 64, 3, 1, 2, 3


@pytest.mark.parametrize("fam,odd", FAMILIES, ids=FAM_IDS)
def test_modswitch_footprint(fam, odd):
    """lwe_modswitch_batch: rot_t (uint32, written) and lwe (read) against the integer model; batch 3 and one past the 32-wide transpose tile"""
    f = Family(fam, PBS_N)
    rng = np.random.default_rng(101)
    for batch in (3, 33):
        lwe = f.words(rng, batch * (PBS_L + 1))
        la = f.arena(1, odd).take("lwe", lwe).build()
        ra = GuardArena(np.uint32, True, 2, odd).take("rot_t", batch * (PBS_L + 1), written=True, guard=4096).build()
        f.plan.lwe_modswitch_batch(ra["rot_t"], la["lwe"], PBS_L)
        la.check()
        want = f.model_modswitch([int(x) for x in lwe], PBS_L, batch)
        assert [int(x) for x in ra.check()["rot_t"]] == want, (fam, batch)


@pytest.mark.parametrize("fam,odd", FAMILIES, ids=FAM_IDS)
def test_sample_extract_footprint(fam, odd):
    """sample_extract_batch: lwe_out (written) and glwe (read) against the integer model, first, second and last coefficient"""
    f = Family(fam, PBS_N)
    n, k, batch = PBS_N, 2, 3
    rng = np.random.default_rng(102)
    glwe = f.words(rng, batch * (k + 1) * n)
    g = [int(x) for x in glwe]
    for index in (0, 1, n - 1):
        ar = f.arena(3, odd).take("glwe", glwe).take("lwe_out", batch * (k * n + 1), written=True, guard=guard(f.bits, n)).build()
        f.plan.sample_extract_batch(ar["lwe_out"], ar["glwe"], k, index)
        want = []
        for b in range(batch):
            base = b * (k + 1) * n
            want += f.model_extract([g[base + q * n:base + (q + 1) * n] for q in range(k + 1)], index)
        assert [int(x) for x in ar.check()["lwe_out"]] == want, (fam, index)


@pytest.mark.parametrize("fam,odd", FAMILIES, ids=FAM_IDS)
def test_blind_rotate_footprint(fam, odd):
    """blind_rotate_batch with the caller's workspace: acc and the workspace written, lut, rot_t and the key read; against the loop of
    gadget_decompose_batch(cmux) + external_product_batch(accumulate) on plain tensors"""
    import torch
    f = Family(fam, PBS_N)
    n, L, k, ell, batch = PBS_N, PBS_L, PBS_K, PBS_ELL, PBS_BATCH
    rng = np.random.default_rng(103)
    lut = f.words(rng, (k + 1) * n)
    rot = (f.tnp if f.native else f.tpp).rot_rows(rng, n, L, batch)
    key, key_arenas, key_plain = f.key(torch, rng, L * (k + 1) * ell * (k + 1), odd)
    wsb = f.plan.pbs_workspace_bytes(L, k, ell, batch)
    isz = np.dtype(f.dt).itemsize
    assert wsb % isz == 0
    ar = f.arena(4, odd).take("lut", lut).take("acc", batch * (k + 1) * n, written=True, guard=guard(f.bits, n))
    ar.take("ws", wsb // isz, written=True, guard=guard(f.bits, n), aligned=True).build()
    ra = GuardArena(np.uint32, True, 5, odd).take("rot_t", rot).build()
    f.plan.blind_rotate_batch(ar["acc"], ar["lut"], ra["rot_t"], key, L, k, f.beta, ell, workspace=ar["ws"], lut_per_element=False)
    got = ar.check()["acc"]
    for a in [ra] + key_arenas:
        a.check()
    want = f.reference_rotation(torch, _dev(torch, lut), _dev(torch, rot), key_plain, L, k, ell, batch)
    assert np.array_equal(got, want.cpu().numpy().view(f.dt)), fam
    assert got.any()


@pytest.mark.parametrize("fam,odd", FAMILIES, ids=FAM_IDS)
def test_bootstrap_footprint(fam, odd):
    """bootstrap_batch with the caller's workspace (rot_t, the accumulator and the digits live in it): lwe_out and the workspace written,
    lwe_in, lut and the key read; against lwe_modswitch_batch, blind_rotate_batch, sample_extract_batch on plain tensors"""
    import torch
    f = Family(fam, PBS_N)
    n, L, k, ell, batch = PBS_N, PBS_L, PBS_K, PBS_ELL, PBS_BATCH
    rng = np.random.default_rng(104)
    lwe, lut = f.words(rng, batch * (L + 1)), f.words(rng, (k + 1) * n)
    key, key_arenas, key_plain = f.key(torch, rng, L * (k + 1) * ell * (k + 1), odd)
    wsb = f.plan.pbs_workspace_bytes(L, k, ell, batch)
    isz = np.dtype(f.dt).itemsize
    ar = f.arena(6, odd).take("lwe_in", lwe).take("lwe_out", batch * (k * n + 1), written=True, guard=guard(f.bits, n)).take("lut", lut)
    ar.take("ws", wsb // isz, written=True, guard=guard(f.bits, n), aligned=True).build()
    f.plan.bootstrap_batch(ar["lwe_out"], ar["lwe_in"], ar["lut"], key, L, k, f.beta, ell, workspace=ar["ws"])
    got = ar.check()["lwe_out"]
    for a in key_arenas:
        a.check()
    lwe_t, lut_t = _dev(torch, lwe), _dev(torch, lut)
    rot_t = torch.zeros((L + 1) * batch, dtype=torch.int32, device="cuda")
    acc, steps = torch.zeros(batch * (k + 1) * n, dtype=lwe_t.dtype, device="cuda"), torch.zeros(batch * (k * n + 1), dtype=lwe_t.dtype, device="cuda")
    f.plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    f.plan.blind_rotate_batch(acc, lut_t, rot_t, key_plain, L, k, f.beta, ell)
    f.plan.sample_extract_batch(steps, acc, k, 0)
    torch.cuda.synchronize()
    assert np.array_equal(got, steps.cpu().numpy().view(f.dt)), fam
    assert got.any()


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
def test_native_external_product_footprint(oracle, odd):
    """cntt_ext.h, cntt_native_external_product_batch (native64, the fused kernel): out written, terms and the key residue planes read;
    replace and accumulate, against the oracle's negacyclic_polymul summed mod 2^64; batches around the products a workgroup holds"""
    import torch
    import test_gpu_native_external_product as tex
    from concrete_ntt_amd import native64
    n, J, O = 64, 3, 2
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(105)
    keyw = tex.random_words(rng, plan, J * O)
    planes = [tex.host(t, np.uint32) for t in tex.key_residues(torch, plan, keyw, J * O)]
    for batch in batches_of([ppb32(n)]):
        terms, prior = tex.random_words(rng, plan, batch * J), tex.random_words(rng, plan, batch * O)
        want = tex.expected(oracle, "native64_plan32", plan, terms, keyw, batch, J, O)
        for accumulate in (False, True):
            ka = GuardArena(np.uint32, True, 7, odd)
            for i, q in enumerate(planes):
                ka.take("k%d" % i, q)
            ka.build()
            ar = GuardArena(np.uint64, True, 8 + batch, odd).take("terms", terms)
            ar.take("out", prior if accumulate else batch * O * n, written=True, guard=guard_both(n)).build()
            plan.external_product_batch(ar["out"], ar["terms"], [ka["k%d" % i] for i in range(len(planes))], J, O, accumulate=accumulate)
            ka.check()
            assert np.array_equal(ar.check()["out"], tex.wadd(prior, want, 8) if accumulate else want), (batch, accumulate)


@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
def test_native_gadget_footprint(odd):
    """cntt_gadget.h (native64): gadget_decompose_batch in the three source modes against the integer model -- terms written, polys and rot
    read -- and external_product_decomposed_batch(cmux, addend = polys) against decompose + external product on plain tensors"""
    import torch
    import test_gpu_native_gadget as tg
    from concrete_ntt_amd import native64
    n, npolys, beta, ell, batch = 64, 2, 5, 3, 3
    plan = native64.Plan32.try_new(n)
    rng = np.random.default_rng(106)
    polys = tg.make_polys(rng, plan, batch, npolys, beta, ell)
    rot = tg.exponents(rng, n, batch)
    pa, rota = tg.to_array(plan, tg.flat(polys)), np.array(rot, dtype=np.uint32)
    for mode in tg.MODES:
        ar = GuardArena(np.uint64, True, 9, odd).take("polys", pa).take("terms", pa.size * ell, written=True, guard=guard_both(n)).build()
        ra = GuardArena(np.uint32, True, 10, odd).take("rot", rota).build()
        plan.gadget_decompose_batch(ar["terms"], ar["polys"], beta, ell, rot=ra["rot"], mode=mode)
        ra.check()
        want = tg.to_array(plan, tg.flat(tg.model_terms(polys, rot, 64, beta, ell, mode)))
        assert np.array_equal(ar.check()["terms"], want), mode
    keyw = tg.key_words(rng, plan, npolys * ell * npolys)
    plain = tg.key_residues(torch, plan, keyw)
    ka = GuardArena(np.uint32, True, 11, odd)
    for i, t in enumerate(plain):
        ka.take("k%d" % i, tg.host(t, np.uint32))
    ka.build()
    ar = GuardArena(np.uint64, True, 12, odd).take("polys", pa).take("out", pa.size, written=True, guard=guard_both(n)).build()
    ra = GuardArena(np.uint32, True, 13, odd).take("rot", rota).build()
    plan.external_product_decomposed_batch(ar["out"], ar["polys"], [ka["k%d" % i] for i in range(len(plain))], beta, ell, npolys, rot=ra["rot"],
                                           mode="cmux", addend=ar["polys"])
    ra.check()
    ka.check()
    pt, rt = _dev(torch, pa), _dev(torch, rota)
    terms, out = torch.zeros(pa.size * ell, dtype=torch.int64, device="cuda"), pt.clone()
    plan.gadget_decompose_batch(terms, pt, beta, ell, rot=rt, mode="cmux")
    plan.external_product_batch(out, terms, plain, npolys * ell, npolys, accumulate=True)
    torch.cuda.synchronize()
    assert np.array_equal(ar.check()["out"], out.cpu().numpy().view(np.uint64))
