"""The NON-TEMPORAL branches (round 5) in every device arithmetic class, and byte offsets past 2^32 on 64-bit words in the
persistent walk.

csrc/host_prime.hip decides per call whether a batch streams through the chip: ntt_device sets ModParams::stream when the batch is larger
than STREAM_BYTES, and the wp / blk walks then load and store through gather_async_rt / issue_rt / scatter_tile_rt with nt = true
(csrc/ntt_kernel.hpp, csrc/ntt_blk.hpp); pointwise_device runs pointwise_kernel<T, OP, true> when NARR x count x word exceeds it
(NARR = 1 normalize, 2 mul_assign_normalize, 3 mul_accumulate).  Every case runs the FIRST size that streams:
  * fwd_batch / inv_batch of floor(STREAM_BYTES / (N x word)) + 1 polynomials against the oracle, every polynomial, bit-exact, and
    against the same input split into two calls below the threshold (the default policy: an independent device path);
  * the three pointwise operations on an ODD element count just past their own rule (the vector tail runs in the streaming
    instantiation too), every word against the oracle;
  * u64 N = 1024 (ntt_kernel_wp) on 2^29 / 1024 + 1 polynomials: 4 GiB + one polynomial, byte offsets past 2^32."""
import os

import numpy as np
import pytest

from test_gpu_multitrip_transforms import (FP50, FP50_P, LAZY, P62, PRIMES, STREAM_BYTES, cus, first_bad, make_plans,
                                           prime_of, transform_shape)

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def streamed_batch(bits, n):
    """the first batch that streams: batch x N x word > STREAM_BYTES (csrc/host_prime.hip ntt_device)"""
    w = bits // 8
    batch = STREAM_BYTES // (n * w) + 1
    assert batch * n * w > STREAM_BYTES and (batch - 1) * n * w <= STREAM_BYTES
    return batch


# wp and blk shapes (csrc/ntt_launch_one.hpp): u64 wp at 16 / 4 / 2 polynomials per workgroup, blk at four / one workgroups per CU; u32 wp with
# 16 and 32 coefficients per thread (N = 1024 / 4096), blk at two / one workgroups per CU
SIZES = [(64, 256), (64, 1024), (64, 2048), (64, 4096), (64, 16384), (32, 1024), (32, 4096), (32, 16384), (32, 32768)]
CASES = [(bits, n, name, p, cls) for (bits, name, p, cls) in PRIMES for (b2, n) in SIZES if b2 == bits]


@pytest.mark.parametrize("bits,n,name,p,cls", CASES, ids=["u%d-%s-n%d" % (b, nm, n) for (b, n, nm, _, _) in CASES])
def test_gpu_streamed_transforms(oracle, bits, n, name, p, cls):
    import torch
    import concrete_ntt_amd as cntt
    p = prime_of(oracle, p)
    plan, oplan = make_plans(oracle, bits, n, p, cls)
    dt = np.uint64 if bits == 64 else np.uint32
    batch = streamed_batch(bits, n)
    half = batch // 2
    ncu = cus()
    x = torch.empty(batch * n, dtype=torch.int64 if bits == 64 else torch.int32, device="cuda")
    cntt.fill_uniform(x, p, 0x57EA + n + cls)
    x[n:2 * n] = 0
    x[(batch - 1) * n:] = (p - 1) - ((p - 1) >> (bits - 1) << bits)      # p - 1 as the signed word of the same bits
    a = _host(x, dt).copy()
    for inv, what in ((False, "fwd"), (True, "inv")):
        rnd = transform_shape(bits, n, cls, inv, ncu)[1]
        y = x.clone()
        (plan.inv_batch if inv else plan.fwd_batch)(y)                   # streams
        z = x.clone()
        for part in (z[:half * n], z[half * n:]):                       # two calls below the threshold
            (plan.inv_batch if inv else plan.fwd_batch)(part)
        torch.cuda.synchronize()
        assert torch.equal(y, z), first_bad(_host(y, dt), _host(z, dt), n, rnd, what + ": streamed vs split in two calls")
        del z
        got = _host(y, dt)
        del y
        want = a.copy()
        (oplan.inv_batch if inv else oplan.fwd_batch)(want, THREADS)
        msg = first_bad(got, want, n, rnd, what + " (streamed, batch %d) vs oracle" % batch)
        assert msg is None, msg
        assert int(got.max()) < p


PW = [("normalize", 1), ("mul_assign_normalize", 2), ("mul_accumulate", 3)]
PW_CASES = [(bits, name, p, cls, op, narr) for (bits, name, p, cls) in PRIMES for (op, narr) in PW]


@pytest.mark.parametrize("bits,name,p,cls,op,narr", PW_CASES, ids=["u%d-%s-%s" % (b, nm, op) for (b, nm, _, _, op, _) in PW_CASES])
def test_gpu_streamed_pointwise(oracle, bits, name, p, cls, op, narr):
    """host slices of any length go through pointwise_device as they are (csrc/host_prime.hip prime_op): an odd count past the rule"""
    p = prime_of(oracle, p)
    plan, oplan = make_plans(oracle, bits, 1024, p, cls)
    w = bits // 8
    count = STREAM_BYTES // (narr * w) + 1
    count |= 1
    assert narr * count * w > STREAM_BYTES and count % (16 // w) != 0
    seed = 0x9E00 + narr * 16 + cls
    x = oracle.fill_uniform(count, p, seed, bits)
    x[:8] = 0
    x[-8:] = p - 1
    want, got = x.copy(), x.copy()
    if op == "normalize":
        oplan.normalize(want)
        plan.normalize(got)
    else:
        y = oracle.fill_uniform(count, p, seed + 1, bits)
        y[-3:] = p - 1
        if op == "mul_assign_normalize":
            oplan.mul_assign_normalize(want, y)
            plan.mul_assign_normalize(got, y)
        else:
            z = oracle.fill_uniform(count, p, seed + 2, bits)
            oplan.mul_accumulate(want, y, z)
            plan.mul_accumulate(got, y, z)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s (streamed, %d words): %d words differ from the oracle, the first at %d" % (op, count, bad.size, bad[0])


def _equal(torch, a, b, chunk=1 << 27):
    for i in range(0, a.numel(), chunk):
        if not torch.equal(a[i:i + chunk], b[i:i + chunk]):
            return i
    return None


@pytest.mark.parametrize("name,p,cls", [("lazy", P62, LAZY), ("fp50", FP50_P, FP50)])
def test_gpu_u64_wp_walk_past_4_gib(oracle, name, p, cls):
    """ntt_kernel_wp<u64, 10> on 4 GiB + one polynomial (tile byte offsets past 2^32; streams): the first, the last and the polynomials
    on both sides of the 2^32-byte boundary against the oracle, every polynomial through normalize(inv(fwd(x))) == x"""
    import torch
    import concrete_ntt_amd as cntt
    n = 1024
    plan, oplan = make_plans(oracle, 64, n, p, cls)
    batch = (1 << 29) // n + 1
    count = batch * n
    edge = (1 << 32) // (8 * n)            # the first polynomial at byte offset 2^32
    assert edge * n * 8 == 1 << 32 and count * 8 > (1 << 32) + 8 * n - 1
    free, _ = torch.cuda.mem_get_info()
    if free < 2.2 * count * 8:
        pytest.skip("needs two 4 GiB buffers; %.0f GiB free" % (free / 2**30))
    x = torch.empty(count, dtype=torch.int64, device="cuda")
    cntt.fill_uniform(x, p, 0x4619B + cls)
    torch.cuda.synchronize()
    picks = (0, edge - 1, edge, batch - 1)
    ends = {i: _host(x[i * n:(i + 1) * n], np.uint64).copy() for i in picks}
    y = x.clone()
    plan.fwd_batch(y)
    torch.cuda.synchronize()
    for i, v in ends.items():
        want = v.copy()
        oplan.fwd(want)
        assert np.array_equal(_host(y[i * n:(i + 1) * n], np.uint64), want), ("fwd", i, batch)
    plan.inv_batch(y)
    torch.cuda.synchronize()
    for i, v in ends.items():
        want = v.copy()
        oplan.fwd(want)
        oplan.inv(want)
        assert np.array_equal(_host(y[i * n:(i + 1) * n], np.uint64), want), ("inv(fwd)", i, batch)
    plan.normalize_batch(y)                # inv(fwd(x)) = N x
    torch.cuda.synchronize()
    off = _equal(torch, y, x)
    assert off is None, ("normalize(inv(fwd(x))) != x", off // n, batch)
