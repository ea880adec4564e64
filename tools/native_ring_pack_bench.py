#!/usr/bin/env python3
"""Timing of the native plans' ring packing (include/cntt_ring_pack.h) on device-resident data, on one GPU, on the Plan32 kinds native64
and native32, k = 1.  Per (kind, n, base_log, levels, batch, M), each figure the time per call of a warmed-up, event-timed window:
  ring      cntt_native_ring_pack_batch (caller workspace, the library's default "autom_lds")
  pksk      cntt_native_pack_keyswitch_batch at Lin = k n, m = M (caller workspace): the packing the library had before
  seq       the caller-side sequence of public calls ring_pack_batch replaces: glwe_embed_batch on all M ciphertexts, per stage the two
            halves made contiguous in torch and one glwe_merge_batch, then glwe_trace_batch
  lds0      ring_pack_batch with the testing switch "autom_lds" = 0 (global gather)
and, per (kind, n, base_log, levels, batch), the LWE-leaf stage against embed + merge: ring_pack_batch at M = 2 (leaf stage 1, then the
trace of log2 n - 1 steps) beside glwe_embed_batch + glwe_merge_batch + the same trace.  Key bytes of both routes follow.  The GPU clock /
power are read before and after (rocm-smi, read-only).  The shapes are those of tools/prime_ring_pack_bench.py, so that the two families
read side by side.
    python tools/native_ring_pack_bench.py [--out profiles/r28_native_ring_pack.txt] [--sizes 1024 2048] [--batches 1 16]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from native_automorphism_bench import GADGETS  # noqa: E402
from prime_automorphism_bench import smi, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--bits", type=int, nargs="+", default=[64, 32])
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native32, native64

    k = 1
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()), "# Plan32 kinds, k = 1, times in ms per call",
             "%8s %6s %3s %2s %6s %5s | %9s %9s %9s | %9s %9s | %9s %9s" %
             ("kind", "n", "bl", "lv", "batch", "M", "ring", "pksk", "pksk/ring", "seq", "seq/ring", "lds0", "lds0/ring")]
    gen = torch.Generator(device="cuda").manual_seed(28)

    def u8(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

    leaf = []
    for bits in args.bits:
        mod = native64 if bits == 64 else native32
        tt = torch.int64 if bits == 64 else torch.int32

        def words(count):   # uniform words: integer tensors wrap, which is the arithmetic mod 2^w
            return torch.randint(-2 ** (bits - 1), 2 ** (bits - 1) - 1, (count,), dtype=tt, device="cuda", generator=gen)

        for n in args.sizes:
            logn = n.bit_length() - 1
            row, ct = k * n + 1, (k + 1) * n
            plan = mod.Plan32.try_new(n)

            def residues(polys):   # any residues time alike: the calls do not look at the keys' content
                return [torch.randint(0, 1 << 29, (polys * n,), dtype=torch.int32, device="cuda", generator=gen) for _ in range(plan.NPRIMES)]

            for beta, ell in GADGETS[bits]:
                per = k * ell * ct
                keys = residues(logn * k * ell * (k + 1))
                pksk = residues(k * n * ell * (k + 1))
                for batch in args.batches:
                    for m in (1, 32, n):
                        lwe = words(batch * m * row)
                        out = torch.empty(batch * ct, dtype=tt, device="cuda")
                        ws = u8(plan.ring_pack_workspace_bytes(m, k, ell, batch))
                        pws = u8(plan.pack_workspace_bytes(k * n, ell, batch))
                        emb = torch.empty(batch * m * ct, dtype=tt, device="cuda")
                        half = torch.empty(max(batch * (m // 2), 1) * ct, dtype=tt, device="cuda")
                        mws = u8(plan.glwe_merge_workspace_bytes(k, ell, batch * max(m // 2, 1)))
                        tws = u8(plan.glwe_trace_workspace_bytes(k, ell, batch))
                        steps = logn - (m.bit_length() - 1)

                        def ring():
                            plan.ring_pack_batch(out, lwe, keys, m, k, beta, ell, workspace=ws)

                        def pack():
                            plan.pack_keyswitch_batch(out, lwe, pksk, k * n, m, k, beta, ell, workspace=pws)

                        def seq():
                            plan.glwe_embed_batch(emb, lwe, k)
                            cur, h, s = emb, m // 2, 1
                            while h >= 1:
                                v = cur[:batch * 2 * h * ct].view(batch, 2, h * ct)
                                e, o = v[:, 0].clone().view(-1), v[:, 1].clone().view(-1)   # copies: dst below may be where they came from
                                dst = half[:batch * h * ct] if cur is emb else emb[:batch * h * ct]
                                r = logn - s
                                plan.glwe_merge_batch(dst, e, o, [p[r * per:(r + 1) * per] for p in keys], n >> s, (1 << s) + 1, k, beta, ell,
                                                      workspace=mws)
                                cur, h, s = dst, h // 2, s + 1
                            plan.glwe_trace_batch(out, cur[:batch * ct], [p[:steps * per] for p in keys] if steps else None, steps, k, beta, ell,
                                                  workspace=tws)

                        a, b, c = timed(torch, ring), timed(torch, pack), timed(torch, seq)
                        with cntt.debug_switches(autom_lds=0):
                            a0 = timed(torch, ring)
                        lines.append("%8s %6d %3d %2d %6d %5d | %9.4f %9.4f %9.2f | %9.4f %9.2f | %9.4f %9.2f" %
                                     ("native%d" % bits, n, beta, ell, batch, m, a, b, b / a, c, c / a, a0, a0 / a))
                        print(lines[-1], flush=True)
                        del lwe, out, ws, pws, emb, half, mws, tws
                    # the leaf stage: M = 2, so that stage 1 is the only stage
                    lwe = words(batch * 2 * row)
                    out, node = (torch.empty(batch * ct, dtype=tt, device="cuda") for _ in range(2))
                    emb = torch.empty(batch * 2 * ct, dtype=tt, device="cuda")
                    ws, mws, tws = u8(plan.ring_pack_workspace_bytes(2, k, ell, batch)), u8(plan.glwe_merge_workspace_bytes(k, ell, batch)), u8(
                        plan.glwe_trace_workspace_bytes(k, ell, batch))

                    def with_leaves():
                        plan.ring_pack_batch(out, lwe, keys, 2, k, beta, ell, workspace=ws)

                    def embed_merge():
                        plan.glwe_embed_batch(emb, lwe, k)
                        v = emb.view(batch, 2, ct)
                        plan.glwe_merge_batch(node, v[:, 0].contiguous().view(-1), v[:, 1].contiguous().view(-1), [p[(logn - 1) * per:] for p in keys],
                                              n // 2, 3, k, beta, ell, workspace=mws)
                        plan.glwe_trace_batch(out, node, [p[:(logn - 1) * per] for p in keys], logn - 1, k, beta, ell, workspace=tws)

                    x, y = timed(torch, with_leaves), timed(torch, embed_merge)
                    leaf.append("#   native%d n = %5d bl = %2d lv = %d batch = %3d: leaves %9.4f ms, embed + merge %9.4f ms (%+.4f ms)" %
                                (bits, n, beta, ell, batch, x, y, y - x))
                    print(leaf[-1], flush=True)
                    del lwe, out, node, emb, ws, mws, tws
                del keys, pksk
    lines.append("# LWE-leaf stage 1 against glwe_embed_batch + glwe_merge_batch, both followed by the same trace of log2 n - 1 steps (M = 2):")
    lines += leaf
    lines.append("# key residues per plane, k = 1: the ring packing holds log2 n * k * levels * (k + 1) polynomials, pksk_ntt at Lin = k n holds "
                 "k n * levels * (k + 1)")
    for n in args.sizes:
        for ell in (2, 4):
            tr, pk = (n.bit_length() - 1) * k * ell * (k + 1) * n * 4, k * n * ell * (k + 1) * n * 4
            lines.append("#   n = %5d levels = %d: trace keys %10d bytes per plane, pksk_ntt %12d bytes per plane (%d x)" % (n, ell, tr, pk, pk // tr))
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
