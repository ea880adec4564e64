#!/usr/bin/env python3
"""Timing of the native plans' Galois keyswitch and trace (include/cntt_automorphism.h) on device-resident data, on one GPU, on native64
and native32 Plan32, k = 1.  Per (kind, n, base_log, levels, batch), each figure the time per call of a warmed-up, event-timed window:
  autoks      cntt_native_glwe_automorphism_keyswitch_batch with add_input (caller workspace), "autom_lds" = 1 (the default)
  autoks-g    the same with "autom_lds" = 0: the global gather
  autoks-seq  the header's public-call sequence: the prefill (torch on the device: a copy, automorphism_batch on the bodies, an add),
              automorphism_batch on the masks, gadget_decompose_batch, the negation of the digits in torch on the device,
              external_product_batch(accumulate)
  trace       cntt_native_glwe_trace_batch with steps = log2 n (caller workspace)
  trace-ks    log2 n calls of autoks with the trace's exponents, alternating between two buffers
  pack        cntt_native_pack_keyswitch_batch at lwe_dim_in = k n, lwe_count = n: the other way from LWE results to a GLWE ciphertext,
              for the key-size and time comparison (its key: k n levels (k + 1) polynomials against log2 n k levels (k + 1))
The two forms of every A/B alternate inside one run on the same box.  The GPU clock / power are read before and after (rocm-smi,
read-only).
    python tools/native_automorphism_bench.py [--out profiles/r27_native_automorphism.txt] [--sizes 1024 2048] [--batches 1 256 4096]"""
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 256, 4096])
    ap.add_argument("--pack-max-batch", type=int, default=256, help="the packing keyswitch reads batch * n LWE ciphertexts of k n + 1 words: capped")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native32, native64

    k = 1
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# command: %s" % " ".join(sys.argv),
             "# before: %s" % "; ".join(smi()), "# Plan32 kinds, k = 1, times in ms per call; seq/one > 1: the one-call form is faster",
             "%8s %5s %2s %2s %5s | %8s %8s %9s %8s %7s | %8s %8s %7s | %8s %9s %8s" %
             ("kind", "n", "bl", "lv", "batch", "autoks", "autoks-g", "autoks-seq", "seq/one", "g/lds", "trace", "trace-ks", "ks/one", "pack", "pack/trace", "keys")]
    gen = torch.Generator(device="cuda").manual_seed(27)

    def u8(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")

    for bits, mod in ((64, native64), (32, native32)):
        tt = torch.int64 if bits == 64 else torch.int32

        def words(count):   # uniform words: integer tensors wrap, which is the arithmetic mod 2^w
            return torch.randint(-2 ** (bits - 1), 2 ** (bits - 1) - 1, (count,), dtype=tt, device="cuda", generator=gen)

        for n in args.sizes:
            logn = n.bit_length() - 1
            plan = mod.Plan32.try_new(n)
            for beta, ell in GADGETS[bits]:
                per_key = k * ell * (k + 1) * n
                # any residues time alike: the calls do not look at the keys' content
                keys = [torch.randint(0, 1 << 29, (logn * per_key,), dtype=torch.int32, device="cuda", generator=gen) for _ in range(plan.NPRIMES)]
                one = [p[:per_key] for p in keys]
                for batch in args.batches:
                    ct = words(batch * (k + 1) * n)
                    out, tmp = torch.empty_like(ct), torch.empty_like(ct)
                    ws = u8(plan.glwe_trace_workspace_bytes(k, ell, batch))
                    view = ct.view(batch, k + 1, n)
                    masks, perm = torch.empty(batch * k * n, dtype=tt, device="cuda"), torch.empty(batch * k * n, dtype=tt, device="cuda")
                    bodies, rot = torch.empty(batch * n, dtype=tt, device="cuda"), torch.empty(batch * n, dtype=tt, device="cuda")
                    terms = torch.empty(batch * k * ell * n, dtype=tt, device="cuda")
                    t = n + 1

                    def autoks():
                        plan.glwe_automorphism_keyswitch_batch(out, ct, one, t, k, beta, ell, True, workspace=ws)

                    def autoks_seq():
                        masks.view(batch, k, n).copy_(view[:, :k])
                        bodies.view(batch, n).copy_(view[:, k])
                        out.copy_(ct)
                        plan.automorphism_batch(rot, bodies, t)
                        out.view(batch, k + 1, n)[:, k] += rot.view(batch, n)
                        plan.automorphism_batch(perm, masks, t)
                        plan.gadget_decompose_batch(terms, perm, beta, ell, mode="plain")
                        terms.neg_()
                        plan.external_product_batch(out, terms, one, k * ell, k + 1, accumulate=True)

                    def trace():
                        plan.glwe_trace_batch(out, ct, keys, logn, k, beta, ell, workspace=ws)

                    def trace_ks():
                        src = ct
                        for r in range(logn):
                            dst = out if (logn - 1 - r) % 2 == 0 else tmp
                            plan.glwe_automorphism_keyswitch_batch(dst, src, [p[r * per_key:(r + 1) * per_key] for p in keys], (n >> r) + 1, k, beta, ell,
                                                                   True, workspace=ws)
                            src = dst

                    # alternate the forms of every A/B
                    a1 = timed(torch, autoks)
                    s1 = timed(torch, autoks_seq)
                    with cntt.debug_switches(autom_lds=0):
                        g1 = timed(torch, autoks)
                    a2 = timed(torch, autoks)
                    s2 = timed(torch, autoks_seq)
                    with cntt.debug_switches(autom_lds=0):
                        g2 = timed(torch, autoks)
                    a, s, g = min(a1, a2), min(s1, s2), min(g1, g2)
                    tr1, tk1 = timed(torch, trace), timed(torch, trace_ks)
                    tr2, tk2 = timed(torch, trace), timed(torch, trace_ks)
                    tr, tk = min(tr1, tr2), min(tk1, tk2)
                    pk, ratio = "-", "-"
                    if batch <= args.pack_max_batch:
                        lin = k * n
                        pksk = [torch.randint(0, 1 << 29, (lin * ell * (k + 1) * n,), dtype=torch.int32, device="cuda", generator=gen) for _ in range(plan.NPRIMES)]
                        lwe = words(batch * n * (lin + 1))
                        pws = u8(plan.pack_workspace_bytes(lin, ell, batch))
                        p = timed(torch, lambda: plan.pack_keyswitch_batch(out, lwe, pksk, lin, n, k, beta, ell, workspace=pws))
                        pk, ratio = "%8.3f" % p, "%9.2f" % (p / tr)
                        del pksk, lwe, pws
                    lines.append("%8s %5d %2d %2d %5d | %8.4f %8.4f %9.4f %8.2f %7.2f | %8.3f %8.3f %7.2f | %8s %9s %8s" %
                                 ("native%d" % bits, n, beta, ell, batch, a, g, s, s / a, g / a, tr, tk, tk / tr, pk, ratio,
                                  "%d/%d" % (n * k * ell * (k + 1), logn * per_key // n)))
                    print(lines[-1], flush=True)
                    del ct, out, tmp, ws, masks, perm, bodies, rot, terms
                    torch.cuda.empty_cache()
    lines.append("# after: %s" % "; ".join(smi()))
    lines.append("# keys: polynomials of the packing key / of the log2 n trace keys.  Not measured: 128-bit words, the Plan52 kinds, k > 1.")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
