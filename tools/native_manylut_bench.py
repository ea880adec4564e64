#!/usr/bin/env python3
"""Timing of the native plans' many-LUT bootstrap and one-rotation circuit bootstrap (include/cntt_manylut.h) on device-resident data, on
one GPU: native64 and native32 Plan32, n = 1024, k = 1, lwe_dim L, PBS gadget (22, 2) on 64-bit and (11, 2) on 32-bit words, keyswitch
gadget (22, 1), cbs_base_log = 4.  Per word width, Lc (t = ceil(log2 Lc)) and batch, each figure the time per call of a warmed-up,
event-timed window, all routes in the same process on the same words, every call with a caller workspace:
  cbs-1rot  cntt_native_circuit_bootstrap_manylut_batch: one blind rotation over batch elements
  cbs       cntt_native_circuit_bootstrap_batch: one blind rotation over batch * Lc elements
  pbs-many  cntt_native_bootstrap_manylut_batch with lut_count = Lc
  pbs x Lc  Lc calls of cntt_native_bootstrap_batch
  ext-many  cntt_native_sample_extract_many_batch with count = Lc on the accumulators alone
  ext x Lc  Lc calls of cntt_native_sample_extract_batch
Rows where a new call loses are marked LOSES.  The GPU clock / power are read before and after (rocm-smi, read-only).
    python tools/native_manylut_bench.py [--out profiles/r30_native_manylut.txt] [--lwe-dim 630] [--batches 1 64 1024] [--cbs-levels 2 4]
                                         [--words 64 32]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prime_automorphism_bench import smi, timed  # noqa: E402

KS = (22, 1)
PBS = {64: (22, 2), 32: (11, 2)}
CBS_BASE_LOG = 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lwe-dim", type=int, default=630)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--cbs-levels", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--words", type=int, nargs="+", default=[64, 32])
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native32, native64

    n, k, L = 1024, 1, args.lwe_dim
    ct, lin = (k + 1) * n, k * n
    kb, kl = KS
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()),
             "# Plan32 kinds, n = %d, k = %d, lwe_dim = %d, pbs gadget (22, 2) on 64-bit and (11, 2) on 32-bit words, ks gadget %s, cbs_base_log = %d; "
             "times in ms per call" % (n, k, L, KS, CBS_BASE_LOG),
             "%2s %2s %1s %5s | %9s %9s %6s | %9s %9s %6s | %9s %9s %6s" % ("w", "Lc", "t", "batch", "cbs-1rot", "cbs", "ratio", "pbs-many", "pbs x Lc",
                                                                         "ratio", "ext-many", "ext x Lc", "ratio")]
    gen = torch.Generator(device="cuda").manual_seed(30)

    for w in args.words:
        plan = (native64 if w == 64 else native32).Plan32.try_new(n)
        wt = torch.int64 if w == 64 else torch.int32
        np_ = plan.NPRIMES
        pbs = PBS[w]

        def words(count):
            return torch.randint(-2 ** (w - 1), 2 ** (w - 1) - 1, (max(count, 1),), dtype=wt, device="cuda", generator=gen)[:count]

        def planes(count):     # any residues time alike: no call looks at the keys' content
            return [torch.randint(0, 1 << 29, (max(count, 1),), dtype=torch.int32, device="cuda", generator=gen)[:count] for _ in range(np_)]

        def u8(nbytes):
            return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

        bsk = planes(L * (k + 1) * pbs[1] * ct)
        fk = words((k + 1) * (lin + 1) * kl * ct)
        lut = words(ct)
        for Lc in args.cbs_levels:
            t = (Lc - 1).bit_length()
            for batch in args.batches:
                lwe = words(batch * (L + 1))
                acc = words(batch * ct)
                out = [torch.empty(batch * (k + 1) * Lc * ct, dtype=torch.int32, device="cuda") for _ in range(np_)]
                out1 = [torch.empty_like(o) for o in out]
                rows = torch.empty(batch * Lc * (lin + 1), dtype=wt, device="cuda")
                one = torch.empty(batch * (lin + 1), dtype=wt, device="cuda")
                ws1 = u8(plan.circuit_bootstrap_manylut_workspace_bytes(L, k, pbs[1], kl, Lc, batch))
                ws = u8(plan.circuit_bootstrap_workspace_bytes(L, k, pbs[1], kl, Lc, batch))
                ws_pbs = u8(plan.pbs_workspace_bytes(L, k, pbs[1], batch))

                def cbs1():
                    plan.circuit_bootstrap_manylut_batch(out1, lwe, bsk, fk, L, k, pbs[0], pbs[1], kb, kl, CBS_BASE_LOG, Lc, t, workspace=ws1)

                def cbs():
                    plan.circuit_bootstrap_batch(out, lwe, bsk, fk, L, k, pbs[0], pbs[1], kb, kl, CBS_BASE_LOG, Lc, workspace=ws)

                def pbs_many():
                    plan.bootstrap_manylut_batch(rows, lwe, lut, bsk, L, k, pbs[0], pbs[1], t, Lc, workspace=ws_pbs)

                def pbs_each():
                    for _ in range(Lc):
                        plan.bootstrap_batch(one, lwe, lut, bsk, L, k, pbs[0], pbs[1], workspace=ws_pbs)

                def ext_many():
                    plan.sample_extract_many_batch(rows, acc, k, Lc)

                def ext_each():
                    for h in range(Lc):
                        plan.sample_extract_batch(one, acc, k, h)

                f = [timed(torch, fn) for fn in (cbs1, cbs, pbs_many, pbs_each, ext_many, ext_each)]
                lose = " LOSES" if f[0] > f[1] or f[2] > f[3] or f[4] > f[5] else ""
                lines.append("%2d %2d %1d %5d | %9.4f %9.4f %6.2f | %9.4f %9.4f %6.2f | %9.4f %9.4f %6.2f%s"
                             % (w, Lc, t, batch, f[0], f[1], f[1] / f[0], f[2], f[3], f[3] / f[2], f[4], f[5], f[5] / f[4], lose))
                print(lines[-1], flush=True)
                del lwe, acc, out, out1, rows, one, ws1, ws, ws_pbs
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f_:
            f_.write(text)
    print(text)


if __name__ == "__main__":
    main()
