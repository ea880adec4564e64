"""The STREAM = true instantiations of the three kernels of native_automorphism.hpp, each at the smallest batch whose byte count passes
STREAM_BYTES at its launch site (host_native_automorphism.inc compares 2 * polys * n * word for calls 1 and 2 -- per residue plane in
call 2 -- and batch * k * levels * n * word, the digit polynomials, for call 3), sized the way tests/test_gpu_prime_streaming.py sizes
its cases: one unit more than fits.  Under both settings of the "autom_lds" switch.  Every word against the same call over two halves of
the batch, which do not stream, and the first and the last element against the model or the public calls; the non-temporal stores must
not change a word."""
import gc

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import test_gpu_native_automorphism as tna
from native_automorphism_model import ntt_permutation
from test_gpu_native_pbs import KINDS, STREAM_BYTES, _torch, host, seed

pytestmark = pytest.mark.gpu


def cleanup(torch):
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lds", [1, 0], ids=["staged", "global"])
def test_automorphism_of_a_streaming_batch(lds):
    """native_automorphism_kernel<uint32_t, true, LDS> at n = 32"""
    torch = _torch()
    n, t = 32, 2 * 32 - 5
    plan = KINDS["native32_plan32"].try_new(n)
    unit = 2 * n * plan.WORD
    polys = STREAM_BYTES // unit + 1
    assert polys * unit > STREAM_BYTES >= (polys - 1) * unit and (polys - polys // 2) * unit <= STREAM_BYTES
    gen = torch.Generator(device="cuda").manual_seed(seed("autom-stream"))
    a = torch.randint(-2 ** 31, 2 ** 31 - 1, (polys * n,), dtype=torch.int32, device="cuda", generator=gen)
    out = torch.full((polys * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    half = polys // 2
    small = torch.empty((polys - half) * n, dtype=torch.int32, device="cuda")
    with cntt.debug_switches(autom_lds=lds):
        plan.automorphism_batch(out, a, t)
        for lo, hi in ((0, half), (half, polys)):
            part = small[:(hi - lo) * n]
            part.fill_(0x5A5A5A5A)
            plan.automorphism_batch(part, a[lo * n:hi * n], t)
            assert torch.equal(part, out[lo * n:hi * n]), (lds, lo, hi)
    for e in (0, polys - 1):
        got = host(out[e * n:(e + 1) * n], np.uint32)
        assert got.any() and np.array_equal(got, tna.sigma(plan, host(a[e * n:(e + 1) * n], np.uint32), t)), (lds, e)
    del a, out, small
    cleanup(torch)


@pytest.mark.parametrize("lds", [1, 0], ids=["staged", "global"])
def test_automorphism_ntt_of_a_streaming_batch(lds):
    """native_automorphism_ntt_kernel<uint32_t, true, LDS> at n = 32, on the two residue planes of native_binary32 Plan32 (the
    permutation does not look at the words, so any residues do)"""
    torch = _torch()
    n, t = 32, 32 + 1
    plan = KINDS["native_binary32_plan32"].try_new(n)
    assert plan.NPRIMES == 2 and plan.RES == 4
    unit = 2 * n * plan.RES
    polys = STREAM_BYTES // unit + 1
    assert polys * unit > STREAM_BYTES >= (polys - 1) * unit
    gen = torch.Generator(device="cuda").manual_seed(seed("autom-ntt-stream"))
    ins = [torch.randint(0, 2 ** 30, (polys * n,), dtype=torch.int32, device="cuda", generator=gen) for _ in range(2)]
    outs = [torch.full((polys * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2)]
    with cntt.debug_switches(autom_lds=lds):
        plan.automorphism_ntt_batch(outs, ins, t)
    torch.cuda.synchronize()
    src = torch.from_numpy(ntt_permutation(t, n)).cuda()
    for i in range(2):
        assert torch.equal(outs[i].view(polys, n), ins[i].view(polys, n)[:, src]), (lds, i)
    del ins, outs
    cleanup(torch)


@pytest.mark.parametrize("lds", [1, 0], ids=["staged", "global"])
@pytest.mark.parametrize("kind,beta", [("native64_plan32", 4), ("native32_plan32", 2)])
def test_autoks_of_a_streaming_batch(kind, beta, lds):
    """native_automorphism_gadget_kernel<W, true, LDS> at n = 1024, k = 1 and 15 levels, with a caller workspace of exactly the workspace
    formula"""
    torch = _torch()
    n, k, ell, t = 1024, 1, 15, 1024 + 1
    plan = KINDS[kind].try_new(n)
    w = plan.WORD
    rng = np.random.default_rng(seed("autoks-stream", kind))
    kr = tna.ak_planes(torch, plan, rng, k, ell)
    tt, lo_, hi_ = (torch.int32, -2 ** 31, 2 ** 31 - 1) if w == 4 else (torch.int64, -2 ** 63, 2 ** 63 - 1)
    gen = torch.Generator(device="cuda").manual_seed(seed("autoks-stream", kind))
    unit = k * ell * n * w
    batch = STREAM_BYTES // unit + 1
    assert batch * unit > STREAM_BYTES >= (batch - 1) * unit and (batch - batch // 2) * unit <= STREAM_BYTES
    per_ct = (k + 1) * n
    a = torch.randint(lo_, hi_, (batch * per_ct,), dtype=tt, device="cuda", generator=gen)
    out = torch.full((batch * per_ct,), 0x5A5A5A5A, dtype=tt, device="cuda")
    ws = torch.empty(plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch), dtype=torch.uint8, device="cuda")
    half = batch // 2
    small = torch.empty((batch - half) * per_ct, dtype=tt, device="cuda")
    with cntt.debug_switches(autom_lds=lds):
        plan.glwe_automorphism_keyswitch_batch(out, a, kr, t, k, beta, ell, True, workspace=ws)
        for lo, hi in ((0, half), (half, batch)):
            part = small[:(hi - lo) * per_ct]
            part.fill_(0x5A5A5A5A)
            plan.glwe_automorphism_keyswitch_batch(part, a[lo * per_ct:hi * per_ct], kr, t, k, beta, ell, True)
            assert torch.equal(part, out[lo * per_ct:hi * per_ct]), (kind, lds, lo, hi)
    for e in (0, batch - 1):
        got = host(out[e * per_ct:(e + 1) * per_ct], plan.word_dtype)
        want = tna.compose_autoks(torch, plan, host(a[e * per_ct:(e + 1) * per_ct], plan.word_dtype), kr, t, k, beta, ell, True)
        assert got.any() and np.array_equal(got, want), (kind, lds, e, tna.first_difference(got, want))
    del a, out, ws, small
    cleanup(torch)
