#!/usr/bin/env python3
"""Timing of the native plans' circuit bootstrap (include/cntt_cbs.h) on device-resident data, on one GPU, on native64 Plan32 and
native32 Plan32 at n = 1024, k = 1, lwe_dim L.  Per kind, keyswitch gadget, Lc and batch, each figure the time per call of a
warmed-up, event-timed window, both routes in the same process on the same words:
  cbs       cntt_native_circuit_bootstrap_batch (caller workspace)
  seq       the public-call sequence it replaces: Lc bootstrap_batch (torch adds 2^(w - 2) and H_l to the bodies), (k + 1) Lc
            pack_keyswitch_batch at lwe_count = 1 on (u, 0) against the residue planes of F_q, one fwd_batch over all rows
  ks        the call at lwe_dim = 0: no blind rotation -- the set-up, the extraction, the digit x key product, the sum of the slabs, the
            split and the transforms; the product dominates.  key GB/s = the bytes of fpksk once per tile of 8 elements over that time, to
            be held against the 6.29 TB/s a float4 copy measures on this part (profiles/r24_prime_cbs.txt's yardstick): the key fits the
            256 MiB Infinity Cache, so later tiles and later calls need not come from HBM at all.
The GPU clock / power are read before and after (rocm-smi, read-only).
    python tools/native_cbs_bench.py [--out profiles/r26_native_cbs.txt] [--lwe-dim 630] [--batches 1 10 64] [--cbs-levels 2 4]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prime_automorphism_bench import smi, timed  # noqa: E402

KS_GADGETS = [(22, 1), (11, 2)]
PBS = {64: (22, 2), 32: (11, 2)}     # the analogous gadget on 32-bit words: the same share of the word


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--lwe-dim", type=int, default=630)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10, 64])
    ap.add_argument("--cbs-levels", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--words", type=int, nargs="+", default=[64, 32])
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native32, native64

    n, k, L = 1024, 1, args.lwe_dim
    ct, lin = (k + 1) * n, k * n
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()),
             "# Plan32 kinds, n = %d, k = %d, lwe_dim = %d, pbs gadget (22, 2) on 64-bit and (11, 2) on 32-bit words, cbs_base_log = 4; times in ms per call"
             % (n, k, L),
             "%2s %3s %2s %2s %5s | %9s %9s %8s | %9s %9s" % ("w", "kbl", "Lk", "Lc", "batch", "cbs", "seq", "seq/cbs", "ks", "key GB/s")]
    gen = torch.Generator(device="cuda").manual_seed(26)

    for w in args.words:
        plan = (native64 if w == 64 else native32).Plan32.try_new(n)
        wt, wb = (torch.int64, 8) if w == 64 else (torch.int32, 4)
        np_ = plan.NPRIMES
        pbs = PBS[w]

        def words(count):
            return torch.randint(-2 ** (w - 1), 2 ** (w - 1) - 1, (max(count, 1),), dtype=wt, device="cuda", generator=gen)[:count]

        def planes(count):     # any residues time alike: no call looks at the keys' content
            return [torch.randint(0, 1 << 29, (max(count, 1),), dtype=torch.int32, device="cuda", generator=gen)[:count] for _ in range(np_)]

        def u8(nbytes):
            return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

        bsk = planes(L * (k + 1) * pbs[1] * ct)
        for kb, kl in KS_GADGETS:
            R = (lin + 1) * kl
            fk = words((k + 1) * R * ct)
            fq = []
            for q in range(k + 1):
                p = [torch.empty(R * ct, dtype=torch.int32, device="cuda") for _ in range(np_)]
                plan.fwd_batch(fk[q * R * ct:(q + 1) * R * ct], p)
                fq.append(p)
            key_bytes = fk.numel() * wb
            for Lc in args.cbs_levels:
                H = [1 << (w - 4 * l - 1) for l in range(1, Lc + 1)]
                luts = []
                for h in H:
                    lut = torch.zeros(ct, dtype=wt, device="cuda")
                    lut[k * n:] = -h
                    luts.append(lut)
                for batch in args.batches:
                    lwe = words(batch * (L + 1))
                    rows = batch * (k + 1) * Lc * ct
                    out = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(np_)]
                    seq_planes = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(np_)]
                    ws = u8(plan.circuit_bootstrap_workspace_bytes(L, k, pbs[1], kl, Lc, batch))
                    ws0 = u8(plan.circuit_bootstrap_workspace_bytes(0, k, pbs[1], kl, Lc, batch))
                    ws_pbs = u8(plan.pbs_workspace_bytes(L, k, pbs[1], batch))
                    ws_pack = u8(plan.pack_workspace_bytes(lin + 1, kl, batch))
                    u = torch.empty(batch * (lin + 1), dtype=wt, device="cuda")
                    cts = torch.zeros(batch, lin + 2, dtype=wt, device="cuda")
                    seq_out = torch.empty(batch, (k + 1) * Lc, ct, dtype=wt, device="cuda")
                    g = torch.empty(batch * ct, dtype=wt, device="cuda")
                    quarter = -(1 << (w - 2)) if False else (1 << (w - 2))

                    def cbs():
                        plan.circuit_bootstrap_batch(out, lwe, bsk, fk, L, k, pbs[0], pbs[1], kb, kl, 4, Lc, workspace=ws)

                    def ks_only():
                        plan.circuit_bootstrap_batch(out, lwe[:batch], None, fk, 0, k, pbs[0], pbs[1], kb, kl, 4, Lc, workspace=ws0)

                    def seq():
                        x = lwe.clone().view(batch, L + 1)
                        x[:, L] += quarter                  # two's complement words wrap like the unsigned ones
                        for l in range(Lc):
                            plan.bootstrap_batch(u, x.view(-1), luts[l], bsk, L, k, pbs[0], pbs[1], workspace=ws_pbs)
                            cts[:, :lin + 1] = u.view(batch, lin + 1)
                            cts[:, lin] += H[l]
                            for q in range(k + 1):
                                plan.pack_keyswitch_batch(g, cts.view(-1), fq[q], lin + 1, 1, k, kb, kl, workspace=ws_pack)
                                seq_out[:, q * Lc + l] = g.view(batch, ct)
                        plan.fwd_batch(seq_out.view(-1), seq_planes)
                        return seq_planes

                    a, b_ = timed(torch, cbs), timed(torch, seq)
                    cbs()
                    assert all(torch.equal(s, o) for s, o in zip(seq(), out))            # the two routes are timed on the same words
                    c = timed(torch, ks_only)
                    tiles = (batch * Lc + 7) // 8
                    lines.append("%2d %3d %2d %2d %5d | %9.4f %9.4f %8.2f | %9.4f %9.1f" % (w, kb, kl, Lc, batch, a, b_, b_ / a, c, key_bytes * tiles / c / 1e6))
                    print(lines[-1], flush=True)
                    del lwe, out, seq_planes, ws, ws0, ws_pbs, ws_pack, u, cts, seq_out, g
            del fk, fq
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
