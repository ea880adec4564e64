#!/usr/bin/env python3
"""Timing of the prime plans' Galois keyswitch and trace (include/cntt_prime_automorphism.h) on device-resident data, on one GPU, with
p = 4611686018427322369 (62 bits), k = 1.  Per (n, base_log, levels, batch), each figure the time per call of a warmed-up, event-timed
window:
  ks        cntt_prime64_glwe_automorphism_keyswitch_batch (t = n / 2 + 1, add_input = 0, caller workspace)
  ks-seq    the caller-side sequence of public calls it replaces: automorphism_batch on the mask and on the body, gadget_decompose_batch,
            the digits negated elementwise in torch, external_product_batch
  trace     cntt_prime64_glwe_trace_batch with steps = log2 n (caller workspace)
  tr-seq    log2 n calls of the keyswitch, each followed by a modular add in torch
  ks/lds0   the keyswitch with the testing switch "autom_lds" = 0 (global gather); "ks" itself runs the library default
  au, au/lds0   cntt_prime64_automorphism_batch on the same ciphertexts, both settings
and the key bytes of a full trace beside the packing key of cntt_prime_pack.h at Lin = k n.  The GPU clock / power are read before and
after (rocm-smi, read-only).
    python tools/prime_automorphism_bench.py [--out profiles/r19_prime_automorphism.txt] [--sizes 1024 2048] [--batches 1 16 256 4096]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4611686018427322369
GADGETS = [(22, 1), (11, 2)]


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def timed(torch, fn, min_s=0.1):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 0
    while time.perf_counter() - t0 < 0.03:   # warm-up and rep count
        fn()
        reps += 1
        torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / reps
    reps = max(2, int(min_s / per))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 2048])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256, 4096])
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import prime64

    k = 1
    lines = ["# %s" % cntt.lib().cntt_version().decode(), "# device: %s" % torch.cuda.get_device_name(0), "# before: %s" % "; ".join(smi()),
             "# p = %d, k = 1, times in ms per call" % P,
             "%6s %3s %2s %6s | %9s %9s %6s | %9s %9s %6s | %9s %9s | %9s %9s" % ("n", "bl", "lv", "batch", "ks", "ks-seq", "ratio", "trace", "tr-seq",
                                                                              "ratio", "ks", "ks/lds0", "au", "au/lds0")]

    def uniform(count, sd):
        t = torch.empty(count, dtype=torch.int64, device="cuda")
        cntt.fill_uniform(t, P, sd)
        return t

    for n in args.sizes:
        logn = n.bit_length() - 1
        plan = prime64.Plan.try_new(n, P)
        for beta, ell in GADGETS:
            per = k * ell * (k + 1) * n
            keys = uniform(logn * per, 1)          # any canonical words time alike: the calls do not look at the key's content
            for batch in args.batches:
                ct = uniform(batch * (k + 1) * n, 2)
                out, tmp, cur = torch.empty_like(ct), torch.empty_like(ct), torch.empty_like(ct)
                ws = torch.empty(plan.glwe_trace_workspace_bytes(k, ell, batch), dtype=torch.uint8, device="cuda")
                terms = torch.empty(batch * k * ell * n, dtype=torch.int64, device="cuda")
                t = n // 2 + 1

                def ks():
                    plan.glwe_automorphism_keyswitch_batch(out, ct, keys[:per], t, k, beta, ell, False, workspace=ws)

                def ks_seq():
                    plan.automorphism_batch(tmp, ct, t)              # mask and body in one gather
                    v = tmp.view(batch, k + 1, n)
                    plan.gadget_decompose_batch(terms, v[:, :k].contiguous().view(-1), beta, ell, mode="plain")
                    neg = torch.where(terms == 0, terms, P - terms)
                    o = out.view(batch, k + 1, n)
                    o[:, :k] = 0
                    o[:, k] = v[:, k]
                    plan.external_product_batch(out, neg, keys[:per], k * ell, k + 1, accumulate=True)

                def trace():
                    plan.glwe_trace_batch(out, ct, keys, logn, k, beta, ell, workspace=ws)

                def tr_seq():
                    cur.copy_(ct)
                    for r in range(logn):
                        plan.glwe_automorphism_keyswitch_batch(tmp, cur, keys[r * per:(r + 1) * per], (n >> r) + 1, k, beta, ell, False, workspace=ws)
                        s = cur + tmp
                        torch.where(s >= P, s - P, s, out=cur)

                def au():
                    plan.automorphism_batch(tmp, ct, t)

                a, b, c, d, e = timed(torch, ks), timed(torch, ks_seq), timed(torch, trace), timed(torch, tr_seq), timed(torch, au)
                with cntt.debug_switches(autom_lds=0):
                    a0, e0 = timed(torch, ks), timed(torch, au)
                with cntt.debug_switches(autom_lds=1):
                    a1, e1 = timed(torch, ks), timed(torch, au)
                lines.append("%6d %3d %2d %6d | %9.4f %9.4f %6.2f | %9.4f %9.4f %6.2f | %9.4f %9.4f | %9.4f %9.4f" % (n, beta, ell, batch, a, b, b / a, c, d,
                                                                                                                   d / c, a1, a0, e1, e0))
                print(lines[-1], flush=True)
                del ct, out, tmp, cur, ws, terms
    lines.append("# columns 11-14: autom_lds = 1 | 0 for the keyswitch and for automorphism_batch alone")
    lines.append("# key bytes, k = 1: a full trace holds log2 n * k * levels * (k + 1) polynomials, the packing key of cntt_prime_pack.h at Lin = k n")
    lines.append("# holds k n * levels * (k + 1)")
    for n in args.sizes:
        for beta, ell in GADGETS:
            tr, pk = (n.bit_length() - 1) * k * ell * (k + 1) * n * 8, k * n * ell * (k + 1) * n * 8
            lines.append("#   n = %5d levels = %d: trace keys %10d bytes, pksk_ntt %12d bytes (%d x)" % (n, ell, tr, pk, pk // tr))
    lines.append("# after: %s" % "; ".join(smi()))
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
