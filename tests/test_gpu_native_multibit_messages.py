"""The multi-bit bootstrap of the native plans (include/cntt_multibit.h) end to end on the MI355X: four encrypted messages through a
look-up table on native64 with noisy keys in the documented key convention, g = 2 and 3; the C example; and the refusals of the header
that need operands on the device or that the other test files leave out, each with the written operands untouched."""
import os
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from test_gpu_native_pbs import KINDS, _torch, dev, host, key_planes, seed

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f(m):
    return (3 * m + 2) & 3


@pytest.mark.parametrize("g", [2, 3])
def test_bootstrap_evaluates_the_table_on_encrypted_messages(g):
    """native64, n = 1024, k = 1, L = 12, base_log 8, levels 4; binary keys.  Key (r, t), row (q, l): a GLWE encryption of zero (uniform
    mask, body = mask * S + e, |e| < 2^10) plus [t == the group's secret pattern] times 2^(64 - base_log l) on coefficient 0 of
    polynomial q -- the GGSW of prod_{i in t} s_i prod_{i not in t} (1 - s_i).  Four messages (twice) under one padding bit, enc(m) =
    m 2^61, the table X^(-n/8) v0 with boxes of n / 4 coefficients, input noise below 2^20.

    Why the decoding must succeed.  The exponent sum errs by at most (L + 1) / 2 + 2 < 128 = half a box.  The phase error of one group
    step: the gadget rounding, at most (1 + k n) 2^(s-1) with s = 64 - 32; and the key noise, each of the 2^g J rows contributing a
    digit polynomial (|d| <= 2^7) times a noise polynomial (< 2^10): below 2^g J n 2^17.  Over G = L / g steps:
    G ((1 + n) 2^31 + 2^g 8 n 2^17) < 6 (2^41 + 2^33) < 2^44, far below the decoding margin 2^60."""
    torch = _torch()
    n, k, beta, ell, L, reps = 1024, 1, 8, 4, 12, 2
    G, J = L // g, (k + 1) * ell
    plan = KINDS["native64_plan32"].try_new(n)
    rng = np.random.default_rng(seed("nmb/functional", g))
    s = [int(x) for x in rng.integers(0, 2, size=L)]
    S = rng.integers(0, 2, size=k * n).astype(np.uint64)
    key = np.zeros((G, 1 << g, J, k + 1, n), dtype=np.uint64)
    key[..., :k, :] = rng.integers(0, 2 ** 64 - 1, size=(G, 1 << g, J, k, n), dtype=np.uint64, endpoint=True)
    masks = dev(torch, np.ascontiguousarray(key[..., :k, :]).reshape(-1))
    Sb = dev(torch, np.ascontiguousarray(np.broadcast_to(S.reshape(1, 1, 1, k, n), (G, 1 << g, J, k, n))).reshape(-1))
    prod = torch.zeros_like(masks)
    plan.negacyclic_polymul_batch(prod, masks, Sb)
    torch.cuda.synchronize()
    with np.errstate(over="ignore"):
        body = host(prod, np.uint64).reshape(G, 1 << g, J, k, n).sum(axis=3, dtype=np.uint64)
        body += rng.integers(-2 ** 10 + 1, 2 ** 10, size=body.shape).astype(np.int64).view(np.uint64)
        for r in range(G):
            pattern = sum(s[r * g + i] << i for i in range(g))
            for q in range(k + 1):
                for l in range(1, ell + 1):
                    j = q * ell + l - 1
                    if q == k:
                        body[r, pattern, j, 0] += np.uint64(1 << (64 - beta * l))
                    else:
                        key[r, pattern, j, q, 0] += np.uint64(1 << (64 - beta * l))
    key[..., k, :] = body
    bsk = key_planes(torch, plan, key.reshape(-1))
    M = 1 << 64
    lut = np.zeros((k + 1) * n, dtype=np.uint64)
    for j in range(n):
        t = j + n // 8
        v = f((t % n) // (n // 4)) << 61
        lut[k * n + j] = v if t < n else (-v) % M
    msgs = [m for _ in range(reps) for m in range(4)]
    batch = len(msgs)
    a = rng.integers(0, 2 ** 64 - 1, size=(batch, L), dtype=np.uint64, endpoint=True)
    noise = [int(x) for x in rng.integers(-2 ** 20 + 1, 2 ** 20, size=batch)]
    lwe_in = np.zeros((batch, L + 1), dtype=np.uint64)
    lwe_in[:, :L] = a
    for b in range(batch):
        lwe_in[b, L] = (sum(int(a[b, i]) * s[i] for i in range(L)) + (msgs[b] << 61) + noise[b]) % M
    lwe_out = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
    plan.multibit_bootstrap_batch(lwe_out, dev(torch, lwe_in.reshape(-1)), dev(torch, lut), bsk, L, k, beta, ell, g)
    torch.cuda.synchronize()
    ct = host(lwe_out, np.uint64).reshape(batch, k * n + 1)
    Si = [int(x) for x in S]
    for b in range(batch):
        phase = (int(ct[b, k * n]) - sum(int(ct[b, i]) * Si[i] for i in range(k * n))) % M
        err = (phase - (f(msgs[b]) << 61) + M // 2) % M - M // 2
        assert abs(err) < 1 << 44, (g, b, msgs[b], err)
        assert (((phase >> 60) + 1) >> 1) & 7 == f(msgs[b]), (g, b)


def test_pbs_multibit_example_builds_and_runs():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples"), "pbs_multibit"], check=True)
    r = subprocess.run([os.path.join(ROOT, "examples", "pbs_multibit")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Success!" in r.stdout, (r.returncode, r.stdout, r.stderr)
    lines = [ln for ln in r.stdout.splitlines() if "message " in ln]
    assert len(lines) == 8 and not any("WRONG" in ln for ln in lines), r.stdout
    assert sum(ln.startswith("g = 2") for ln in lines) == 4 and sum(ln.startswith("g = 3") for ln in lines) == 4


def test_remaining_refusals_leave_the_written_operands_untouched():
    """a misaligned operand and workspace, the NULL arguments, the host path's exponent rule for the rotation inside and outside the
    bootstrap, the accumulate's refusals: CNTT_EINVAL each, acc / out planes / lwe_out as they were"""
    import ctypes
    from concrete_ntt_amd._lib import EINVAL, MEM_DEVICE, last_error
    torch = _torch()
    n, k, L, batch, ell, beta, g = 32, 1, 4, 2, 2, 8, 2
    plan = KINDS["native64_plan32"].try_new(n)
    J, NP = (k + 1) * ell, plan.NPRIMES
    lib = cntt.lib()

    def buf(words, dtype=torch.int64, fill=9):
        return torch.full((words,), fill, dtype=dtype, device="cuda")

    acc, lut, rot = buf(batch * (k + 1) * n + 2), buf((k + 1) * n + 2), buf((L + 1) * batch, torch.int32, 0)
    lwe_in, lwe_out = buf(batch * (L + 1) + 2), buf(batch * (k * n + 1) + 2)
    kp = [buf(((L // g) * J * (k + 1) << g) * n, torch.int32, 1) for _ in range(NP)]
    ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, ell, g, batch) + 16, dtype=torch.uint8, device="cuda")
    keys = (ctypes.c_void_p * NP)(*[x.data_ptr() for x in kp])
    rotate, boot, accum = (lib.cntt_native_multibit_blind_rotate_batch, lib.cntt_native_multibit_bootstrap_batch,
                           lib.cntt_native_multibit_accumulate_batch)

    def rot_args(a=acc.data_ptr(), lu=lut.data_ptr(), r=rot.data_ptr(), w=None, wb=0):
        return (plan._h, a, lu, 0, r, keys, L, k, beta, ell, g, batch, w, wb, MEM_DEVICE, None)

    def boot_args(o=lwe_out.data_ptr(), i=lwe_in.data_ptr(), lu=lut.data_ptr(), w=None, wb=0):
        return (plan._h, o, i, lu, 0, keys, L, k, beta, ell, g, batch, w, wb, MEM_DEVICE, None)

    for fn, args, text in (
            (rotate, rot_args(a=acc.data_ptr() + 4), "acc is not 8-byte aligned"), (rotate, rot_args(a=None), "acc is NULL"),
            (rotate, rot_args(lu=None), "lut is NULL"), (rotate, rot_args(r=None), "rot_t is NULL"),
            (rotate, rot_args(lu=lut.data_ptr() + 4), "lut is not 8-byte aligned"),
            (rotate, rot_args(w=ws.data_ptr() + 8, wb=ws.numel() - 8), "workspace is not 16-byte aligned"),
            (rotate, rot_args(lu=acc.data_ptr()), "acc overlaps lut"),
            (boot, boot_args(o=None), "lwe_out is NULL"), (boot, boot_args(i=None), "lwe_in is NULL"), (boot, boot_args(lu=None), "lut is NULL"),
            (boot, boot_args(o=lwe_out.data_ptr() + 4), "lwe_out is not 8-byte aligned"),
            (boot, boot_args(w=ws.data_ptr() + 8, wb=ws.numel() - 8), "workspace is not 16-byte aligned"),
            (boot, boot_args(w=lwe_out.data_ptr(), wb=lwe_out.numel() * 8), "workspace_bytes")):
        assert fn(*args) == EINVAL and text in last_error(), (text, last_error())
    # the accumulate call: misaligned plane, NULL rot_rows, grouping
    out = [buf(batch * (k + 1) * n + 1, torch.int32, 7) for _ in range(NP)]
    terms = [buf(batch * J * n, torch.int32, 1) for _ in range(NP)]
    grp = [buf((J * (k + 1) << g) * n, torch.int32, 1) for _ in range(NP)]
    arr = lambda ts, off=0: (ctypes.c_void_p * NP)(*[x.data_ptr() + off for x in ts])   # noqa: E731
    rows = buf(g * batch, torch.int32, 0)
    for args, text in (((arr(out, 2), arr(terms), rows.data_ptr(), arr(grp), J, k + 1, g), "out_ntt[0] is not 4-byte aligned"),
                       ((arr(out), arr(terms), None, arr(grp), J, k + 1, g), "rot_rows is NULL"),
                       ((arr(out), arr(terms), rows.data_ptr(), arr(grp), J, k + 1, 5), "grouping = 5"),
                       ((arr(out), arr(out), rows.data_ptr(), arr(grp), k + 1, k + 1, g), "overlaps")):
        assert accum(plan._h, *args, batch, MEM_DEVICE, None) == EINVAL and text in last_error(), (text, last_error())
    torch.cuda.synchronize()
    assert all(bool((t == 9).all()) for t in (acc, lwe_out)) and all(bool((t == 7).all()) for t in out)
    # host path: an exponent that is not below 2n, in the rotation and in the accumulate
    h_acc, h_lut = np.full(batch * (k + 1) * n, 9, np.uint64), np.zeros((k + 1) * n, np.uint64)
    h_rot = np.zeros((L + 1) * batch, np.uint32)
    h_rot[3] = 2 * n
    h_keys = [np.ones(((L // g) * J * (k + 1) << g) * n, np.uint32) for _ in range(NP)]
    with pytest.raises(cntt.Panic, match=r"rot_t\[3\] = 64 is not below 2n"):
        plan.multibit_blind_rotate_batch(h_acc, h_lut, h_rot, h_keys, L, k, beta, ell, g)
    assert (h_acc == 9).all()
