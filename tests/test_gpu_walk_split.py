"""How the persistent walks END.  ntt_kernel_wp / mul_kernel_wp (csrc/ntt_kernel.hpp NttWp::run / MulWp::run) walk `full` complete rounds
of the resident grid and then hand the `rem` leftover polynomials out one WAVEFRONT at a time over all workgroups ("wave w of workgroup
g", g fastest: WalkArgs / walk_plan), where a polynomial lives in one wavefront; the shapes whose polynomial spans several wavefronts
(s_barrier in the tile body: u64 n = 2048) keep the tile-by-tile walk.  The testing switch "walk_split" = 0 gives every shape the
tile-by-tile walk.  The words written must not depend on any of this.

Batches sit on every edge of that arithmetic for the 768-thread fused kernel of prime64 n = 1024 (12 polynomials per workgroup, one
workgroup per CU, G = CUs): below / at / above one tile, one short of / exactly / one past a full round, a round plus one leftover per SIMD
(4 G: the headline benchmark's own remainder pattern), one more, and two rounds plus 7.  Per batch, with the switch at its default:
  * mul_ntt_batch(a, b^) == fwd_batch; mul_assign_normalize_batch; inv_batch on the whole batch;
  * == the CPU oracle word for word on polynomials {0, middle, last};
  * == the "walk_split" = 0 result on the whole batch;
  * fwd_batch / inv_batch alone: the oracle on the same three polynomials, and the "walk_split" = 0 result on the whole batch;
  * two polynomials of 0xA5 pattern behind the batch are untouched after every call, and b^ is unchanged.
Further: u64 n = 256 (four polynomials per wavefront) and u32 n = 1024 (the other word width) at {1, round + 1, round + grid + 3} of
their own launch shapes, and the barrier shape u64 n = 2048 at {1, 6 G + 5}."""
import numpy as np
import pytest

import concrete_ntt_amd as cntt
from test_gpu_multitrip_transforms import LAZY, P30, P62, cus, make_plans, mul_shape, transform_shape

pytestmark = pytest.mark.gpu

GUARD_POLYS = 2


def _alloc(bits, n, batch, p, seed):
    """batch polynomials of uniform residues followed by GUARD_POLYS polynomials of 0xA5 bytes, one allocation; returns (whole, view)"""
    import torch
    dt = torch.int64 if bits == 64 else torch.int32
    whole = torch.empty((batch + GUARD_POLYS) * n, dtype=dt, device="cuda:0")
    view = whole[:batch * n]
    cntt.fill_uniform(view, p, seed)
    whole[batch * n:] = -0x5A5A5A5A5A5A5A5B if bits == 64 else -0x5A5A5A5B   # 0xA5A5... as a signed word
    return whole, view


def _guard_ok(whole, n, batch):
    tail = whole[batch * n:]
    want = -0x5A5A5A5A5A5A5A5B if whole.element_size() == 8 else -0x5A5A5A5B
    return bool((tail == want).all().item())


def _poly(t, n, i, dt):
    return t[i * n:(i + 1) * n].cpu().numpy().view(dt).copy()


def _check_case(oracle, bits, n, p, cls, batch):
    import torch
    plan, oplan = make_plans(oracle, bits, n, p, cls)
    dt = np.uint64 if bits == 64 else np.uint32
    seed = 7 * batch + n + bits
    picks = sorted({0, batch // 2, batch - 1})
    wa, a0 = _alloc(bits, n, batch, p, seed + 1)
    wb, b0 = _alloc(bits, n, batch, p, seed + 2)
    a_host = {i: _poly(a0, n, i, dt) for i in picks}
    b_host = {i: _poly(b0, n, i, dt) for i in picks}

    def run(op, src, split, rhs=None):
        """op on a guarded copy of src with walk_split = split; the guard band and rhs must come back as they were"""
        w = torch.empty_like(wa)
        w.copy_(torch.cat([src, wa[batch * n:]]))
        v = w[:batch * n]
        rhs0 = rhs.clone() if rhs is not None else None
        with cntt.debug_switches(walk_split=split):
            if op == "fwd":
                plan.fwd_batch(v)
            elif op == "inv":
                plan.inv_batch(v)
            elif op == "mul":
                plan.mul_ntt_batch(v, rhs)
            else:
                plan.fwd_batch(v)
                plan.mul_assign_normalize_batch(v, rhs)
                plan.inv_batch(v)
        torch.cuda.synchronize()
        assert _guard_ok(w, n, batch), ("stores past the end of the batch", op, split, batch)
        if rhs is not None:
            assert torch.equal(rhs, rhs0), ("rhs_ntt changed", op, split, batch)
        return v

    # ---- stand-alone transforms ------------------------------------------------------------------------------------------------
    for op in ("fwd", "inv"):
        new, old = run(op, a0, 1), run(op, a0, 0)
        assert torch.equal(new, old), ("walk_split 1 vs 0", op, bits, n, batch)
        for i in picks:
            want = a_host[i].copy()
            (oplan.fwd if op == "fwd" else oplan.inv)(want)
            assert np.array_equal(_poly(new, n, i, dt), want), (op + " vs oracle", bits, n, batch, i)
        del new, old
    # ---- the fused product ---------------------------------------------------------------------------------------------------------
    bhat = run("fwd", b0, 1)
    assert _guard_ok(wb, n, batch)
    fused = run("mul", a0, 1, bhat)
    assert torch.equal(fused, run("three", a0, 1, bhat)), ("fused vs three launches", bits, n, batch)
    assert torch.equal(fused, run("mul", a0, 0, bhat)), ("walk_split 1 vs 0", "mul", bits, n, batch)
    for i in picks:
        want, bn = a_host[i].copy(), b_host[i].copy()
        oplan.fwd(want)
        oplan.fwd(bn)
        oplan.mul_assign_normalize(want, bn)
        oplan.inv(want)
        assert np.array_equal(_poly(fused, n, i, dt), want), ("mul_ntt vs oracle", bits, n, batch, i)


def _headline_batches():
    g = cus()
    return [1, 11, 12, 13, 12 * g - 1, 12 * g, 12 * g + 1, 12 * g + 4 * g, 12 * g + 4 * g + 1, 2 * 12 * g + 7]


@pytest.mark.parametrize("k", range(10), ids=["b1", "b11", "b12", "b13", "round-1", "round", "round+1", "round+4G", "round+4G+1", "2rounds+7"])
def test_headline_walk_ends(oracle, k):
    batch = _headline_batches()[k]
    assert mul_shape(64, 1024, LAZY, cus())[1:] == (12 * cus(), 12), "the fused kernel's launch shape moved: restate the batches"
    _check_case(oracle, 64, 1024, P62, LAZY, batch)


def _shape_batches(bits, n):
    """{1, round + 1, round + grid + 3} for each launch shape that serves (bits, n): the fused product's and the transforms'"""
    out = {1}
    shapes = [mul_shape(bits, n, LAZY, cus())] + [transform_shape(bits, n, LAZY, inv, cus()) for inv in (False, True)]
    for kernel, rnd, ppb in shapes:
        assert kernel == "wp", (kernel, bits, n)
        out |= {rnd + 1, rnd + rnd // ppb + 3}
    return sorted(out)


@pytest.mark.parametrize("bits,n,p", [(64, 256, P62), (32, 1024, P30)], ids=["u64-n256", "u32-n1024"])
def test_other_wave_private_shapes(oracle, bits, n, p):
    for batch in _shape_batches(bits, n):
        _check_case(oracle, bits, n, p, LAZY, batch)


@pytest.mark.parametrize("which", [0, 1], ids=["b1", "6G+5"])
def test_barrier_shape_keeps_its_walk(oracle, which):
    """u64 n = 2048: 128 threads per polynomial, s_barrier in the tile body -- the walk is workgroup-uniform whatever the switch says"""
    _check_case(oracle, 64, 2048, P62, LAZY, [1, 6 * cus() + 5][which])
