#!/usr/bin/env python3
"""Timing of the native plans' CMux and CMux tree (include/cntt_cmux.h) on device-resident data, on one GPU, on native64 and native32
Plan32, k = 1.  Per (kind, n, base_log, levels), each figure the time per call of a warmed-up, event-timed window:
  tree      cntt_native_cmux_tree_batch at lut_count = M, `batch` tables (caller workspace)
  tree-seq  the header's public-call sequence for the same tree: per stage the prefill (a device copy of c0; stage 1: zero masks and the
            body), the wrapping difference in torch on the device, gadget_decompose_batch and external_product_batch(accumulate)
  cmux      cntt_native_glwe_cmux_batch on `cmux-batch` pairs of ciphertexts (caller workspace)
  cmux-seq  its sequence: the copy, the torch difference, gadget_decompose_batch, external_product_batch(accumulate)
The GPU clock / power are read before and after (rocm-smi, read-only).
    python tools/native_cmux_bench.py [--out profiles/r25_native_cmux.txt] [--sizes 1024] [--lut-count 256] [--batch 64] [--cmux-batch 4096]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from prime_automorphism_bench import smi, timed  # noqa: E402

GADGETS = {64: [(22, 2), (15, 4)], 32: [(12, 2), (7, 4)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024])
    ap.add_argument("--lut-count", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--cmux-batch", type=int, default=4096)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native32, native64

    k, m, batch, cb = 1, args.lut_count, args.batch, args.cmux_batch
    depth = m.bit_length() - 1
    assert m >= 2 and m & (m - 1) == 0, "--lut-count: a power of two, at least 2"
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()), "# Plan32 kinds, k = 1, M = %d, batch = %d, cmux batch = %d, times in ms per call" % (m, batch, cb),
             "%8s %6s %3s %2s | %9s %9s %9s | %9s %9s %9s" % ("kind", "n", "bl", "lv", "tree", "tree-seq", "seq/tree", "cmux", "cmux-seq", "seq/cmux")]
    gen = torch.Generator(device="cuda").manual_seed(25)

    def u8(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

    for bits, mod in ((64, native64), (32, native32)):
        tt = torch.int64 if bits == 64 else torch.int32

        def words(count):   # uniform words: integer tensors wrap, which is the arithmetic mod 2^w
            return torch.randint(-2 ** (bits - 1), 2 ** (bits - 1) - 1, (count,), dtype=tt, device="cuda", generator=gen)

        for n in args.sizes:
            ct = (k + 1) * n
            plan = mod.Plan32.try_new(n)
            for beta, ell in GADGETS[bits]:
                per = (k + 1) * ell * ct
                # any residues time alike: the calls do not look at the selectors' content
                sels = [torch.randint(0, 1 << 29, (depth * per,), dtype=torch.int32, device="cuda", generator=gen) for _ in range(plan.NPRIMES)]
                lut = words(batch * m * n)
                out = torch.empty(batch * ct, dtype=tt, device="cuda")
                ws = u8(plan.cmux_tree_workspace_bytes(m, k, ell, batch))
                terms = torch.empty(batch * max(m // 2, 1) * (k + 1) * ell * n, dtype=tt, device="cuda")

                def tree():
                    plan.cmux_tree_batch(out, lut, sels, m, k, beta, ell, workspace=ws)

                def tree_seq():
                    v = lut.view(batch, 2, (m // 2) * n)
                    h = m // 2
                    f0, f1 = v[:, 0].view(batch, h, n), v[:, 1].view(batch, h, n)
                    cur = torch.zeros(batch, h, k + 1, n, dtype=tt, device="cuda")
                    cur[:, :, k] = f0
                    cur = cur.view(-1)
                    t = terms[:batch * h * ell * n]
                    plan.gadget_decompose_batch(t, (f1 - f0).view(-1), beta, ell, mode="plain")
                    plan.external_product_batch(cur, t, [p[(depth - 1) * per + k * ell * ct:depth * per] for p in sels], ell, k + 1, accumulate=True)
                    for s in range(2, depth + 1):
                        h = m >> s
                        v = cur.view(batch, 2, h * ct)
                        nxt = v[:, 0].clone().view(-1)
                        t = terms[:batch * h * (k + 1) * ell * n]
                        plan.gadget_decompose_batch(t, (v[:, 1] - v[:, 0]).view(-1), beta, ell, mode="plain")
                        plan.external_product_batch(nxt, t, [p[(depth - s) * per:(depth - s + 1) * per] for p in sels], (k + 1) * ell, k + 1,
                                                    accumulate=True)
                        cur = nxt
                    return cur

                a, b = timed(torch, tree), timed(torch, tree_seq)
                assert torch.equal(tree_seq(), out)           # the two routes are timed on the same words
                del lut, out, ws, terms
                c0, c1 = words(cb * ct), words(cb * ct)
                out = torch.empty(cb * ct, dtype=tt, device="cuda")
                ws = u8(plan.glwe_cmux_workspace_bytes(k, ell, cb))
                terms = torch.empty(cb * (k + 1) * ell * n, dtype=tt, device="cuda")
                one = [p[:per] for p in sels]

                def cmux():
                    plan.glwe_cmux_batch(out, c0, c1, one, k, beta, ell, workspace=ws)

                def cmux_seq():
                    out.copy_(c0)
                    plan.gadget_decompose_batch(terms, c1 - c0, beta, ell, mode="plain")
                    plan.external_product_batch(out, terms, one, (k + 1) * ell, k + 1, accumulate=True)

                c, d = timed(torch, cmux), timed(torch, cmux_seq)
                lines.append("%8s %6d %3d %2d | %9.4f %9.4f %9.2f | %9.4f %9.4f %9.2f" % ("native%d" % bits, n, beta, ell, a, b, b / a, c, d, d / c))
                print(lines[-1], flush=True)
                del c0, c1, out, ws, terms
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
