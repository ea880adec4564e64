#!/usr/bin/env python3
"""Timing of the prime plans' circuit bootstrap (include/cntt_prime_cbs.h) on device-resident data, on one GPU, with
p = 4611686018427322369 (62 bits), n = 1024, k = 1, lwe_dim L.  Per keyswitch gadget, Lc and batch, each figure the time per call of a
warmed-up, event-timed window, both routes in the same process on the same words:
  cbs       cntt_prime64_circuit_bootstrap_batch (caller workspace)
  seq       the public-call sequence it replaces: Lc bootstrap_batch (torch adds Q4 and H_l to the bodies), (k + 1) Lc
            pack_keyswitch_batch at lwe_count = 1 on (u, 0), one fwd_batch and one normalize_batch over all rows
  ks        the call at lwe_dim = 0: no blind rotation -- the set-up, the extraction, the digit x key product and the sum of the slabs; the
            product dominates.  key GB/s = the bytes of fpksk_ntt once per tile of 8 elements over that time, to be held against the
            6.29 TB/s a float4 copy measures on this part (8.0 TB/s spec): the key fits the 256 MiB Infinity Cache, so later tiles and
            later calls need not come from HBM at all.
The GPU clock / power are read before and after (rocm-smi, read-only).
    python tools/prime_cbs_bench.py [--out profiles/r24_prime_cbs.txt] [--lwe-dim 630] [--batches 1 10 64] [--cbs-levels 2 4]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prime_automorphism_bench import P, smi, timed  # noqa: E402

KS_GADGETS = [(22, 1), (11, 2)]
PBS = (22, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lwe-dim", type=int, default=630)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 64])
    ap.add_argument("--cbs-levels", type=int, nargs="+", default=[2, 4])
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import prime64

    n, k, L = 1024, 1, args.lwe_dim
    ct, lin = (k + 1) * n, k * n
    plan = prime64.Plan.try_new(n, P)
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()),
             "# p = %d, n = %d, k = %d, lwe_dim = %d, pbs gadget %s, cbs_base_log = 8; times in ms per call" % (P, n, k, L, PBS),
             "%3s %2s %2s %5s | %9s %9s %8s | %9s %9s" % ("kbl", "Lk", "Lc", "batch", "cbs", "seq", "seq/cbs", "ks", "key GB/s")]

    def uniform(count, sd):
        t = torch.empty(max(count, 1), dtype=torch.int64, device="cuda")
        cntt.fill_uniform(t, P, sd)
        return t[:count]

    def u8(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

    bsk = uniform(L * (k + 1) * PBS[1] * ct, 1)          # any canonical words time alike: no call looks at the keys' content
    for kb, kl in KS_GADGETS:
        R = (lin + 1) * kl
        fk = uniform((k + 1) * R * ct, 2)
        key_bytes = fk.numel() * 8
        for Lc in args.cbs_levels:
            H = [1 << (62 - 8 * l - 1) for l in range(1, Lc + 1)]
            luts = []
            for h in H:
                lut = torch.zeros(ct, dtype=torch.int64, device="cuda")
                lut[k * n:] = P - h
                luts.append(lut)
            for batch in args.batches:
                lwe = uniform(batch * (L + 1), 3)
                out = torch.empty(batch * (k + 1) * Lc * ct, dtype=torch.int64, device="cuda")
                ws = u8(plan.circuit_bootstrap_workspace_bytes(L, k, PBS[1], kl, Lc, batch))
                ws0 = u8(plan.circuit_bootstrap_workspace_bytes(0, k, PBS[1], kl, Lc, batch))
                ws_pbs = u8(plan.pbs_workspace_bytes(L, k, PBS[1], batch))
                ws_pack = u8(plan.pack_workspace_bytes(lin + 1, kl, batch))
                u = torch.empty(batch * (lin + 1), dtype=torch.int64, device="cuda")
                cts = torch.zeros(batch, lin + 2, dtype=torch.int64, device="cuda")
                seq_out = torch.empty(batch, (k + 1) * Lc, ct, dtype=torch.int64, device="cuda")
                g = torch.empty(batch * ct, dtype=torch.int64, device="cuda")
                q4 = (P + 2) // 4

                def cbs():
                    plan.circuit_bootstrap_batch(out, lwe, bsk, fk, L, k, PBS[0], PBS[1], kb, kl, 8, Lc, workspace=ws)

                def ks_only():
                    plan.circuit_bootstrap_batch(out, lwe[:batch], None, fk, 0, k, PBS[0], PBS[1], kb, kl, 8, Lc, workspace=ws0)

                def seq():
                    x = lwe.clone().view(batch, L + 1)
                    b = x[:, L] + q4                      # canonical words below 2^62 in int64
                    x[:, L] = b - (b >= P) * P
                    for l in range(Lc):
                        plan.bootstrap_batch(u, x.view(-1), luts[l], bsk, L, k, PBS[0], PBS[1], workspace=ws_pbs)
                        cts[:, :lin + 1] = u.view(batch, lin + 1)
                        b = cts[:, lin] + H[l]
                        cts[:, lin] = b - (b >= P) * P
                        for q in range(k + 1):
                            plan.pack_keyswitch_batch(g, cts.view(-1), fk[q * R * ct:(q + 1) * R * ct], lin + 1, 1, k, kb, kl, workspace=ws_pack)
                            seq_out[:, q * Lc + l] = g.view(batch, ct)
                    flat = seq_out.view(-1)
                    plan.fwd_batch(flat)
                    plan.normalize_batch(flat)
                    return flat

                a, b_ = timed(torch, cbs), timed(torch, seq)
                cbs()
                assert torch.equal(seq(), out)            # the two routes are timed on the same words
                c = timed(torch, ks_only)
                tiles = (batch * Lc + 7) // 8
                lines.append("%3d %2d %2d %5d | %9.4f %9.4f %8.2f | %9.4f %9.1f" % (kb, kl, Lc, batch, a, b_, b_ / a, c, key_bytes * tiles / c / 1e6))
                print(lines[-1], flush=True)
                del lwe, out, ws, ws0, ws_pbs, ws_pack, u, cts, seq_out, g
        del fk
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
