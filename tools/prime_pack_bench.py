#!/usr/bin/env python3
"""Timing of the prime plans' LWE-to-GLWE packing keyswitch (include/cntt_prime_pack.h) on device-resident data against the direct route
that existed before it: cntt_prime*_keyswitch_batch on batch * m rows with row_stride = Lout + 1 = (k + 1) n (its rotate-and-sum left
out, which favours the baseline).  Per shape: time per call of each route (three repetitions of a warmed-up, event-timed window; the
spread of the direct route's three is the run-to-run noise) and the ratio; the table ends with the smallest m at which the NTT route is
the faster one.  The direct route is timed on at most --max-rows rows (4096 by default); past that its time is the per-row time at --max-rows times the
row count (it is a GEMM whose key no longer fits the caches: linear in the rows), and the table marks it.  One process under `timeout`
runs both routes; the driver prints one JSON line per shape, the GPU clock / power read before and after (rocm-smi, read-only), and
writes the table.
    python tools/prime_pack_bench.py [--out profiles/r14_prime_pack.txt] [--words 64] [--sizes 1024] [--batches 1]
    python tools/prime_pack_bench.py --label terms32 --no-baseline      (the CNTT_PRIME_PACK_TERMS A/B: one run per build of the library)
    python tools/prime_pack_bench.py --one W        (all shapes of one word width, this process; JSON lines on stdout)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def timed(torch, fn, min_s=0.2):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 0
    while time.perf_counter() - t0 < 0.05:   # warm-up and rep count
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


PRIMES = {64: 18446744069414584321, 32: 1062862849}      # 2^64 - 2^32 + 1 (W = 64); a 30-bit prime = 1 mod 16384


def one(w, sizes, batches, counts, gadget, max_rows, baseline, label):
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import prime32, prime64
    dt = torch.int64 if w == 64 else torch.int32
    p = PRIMES[w]
    beta, ell = gadget
    k = 1

    def uniform(count, sd):
        t = torch.empty(count, dtype=dt, device="cuda")
        cntt.fill_uniform(t, p, sd)
        return t

    for n in sizes:
        plan = {32: prime32, 64: prime64}[w].Plan.try_new(n, p)
        lin, cols = k * n, (k + 1) * n
        # one coefficient-domain key for both routes; the NTT route reads n^-1 fwd(key)
        keyw = uniform(lin * ell * cols, 1)
        kn = keyw.clone()
        plan.fwd_batch(kn)
        plan.normalize_batch(kn)
        torch.cuda.synchronize()
        if not baseline:
            del keyw
        per_row = {}
        for batch in batches:
            ws = torch.zeros(plan.pack_workspace_bytes(lin, ell, batch), dtype=torch.uint8, device="cuda")
            out = torch.zeros(batch * cols, dtype=dt, device="cuda")
            for m in [c if c else n for c in counts]:
                lwe = uniform(batch * m * (lin + 1), 2 + m)
                ms = [timed(torch, lambda: plan.pack_keyswitch_batch(out, lwe, kn, lin, m, k, beta, ell, workspace=ws)) for _ in range(3)]
                row = {"w": w, "n": n, "k": k, "lin": lin, "base_log": beta, "levels": ell, "batch": batch, "m": m, "label": label,
                       "pack_ms": [round(x, 4) for x in ms], "pack_spread": round(max(ms) / min(ms) - 1, 4)}
                if baseline:
                    rows = batch * m
                    timed_rows = min(rows, max_rows)
                    if timed_rows not in per_row:
                        rows_out = torch.zeros(timed_rows * cols, dtype=dt, device="cuda")
                        sub = lwe[:timed_rows * (lin + 1)]
                        per_row[timed_rows] = [timed(torch, lambda: plan.keyswitch_batch(rows_out, sub, keyw, lin, cols - 1, beta, ell), 0.1)
                                               for _ in range(3)]
                        del rows_out
                    d = per_row[timed_rows]
                    scale = rows / timed_rows
                    row.update({"direct_ms": [round(x * scale, 4) for x in d], "direct_rows_timed": timed_rows,
                                "direct_extrapolated": rows != timed_rows, "direct_spread": round(max(d) / min(d) - 1, 4),
                                "direct_over_pack": round(min(d) * scale / min(ms), 3)})
                print(json.dumps(row), flush=True)
                del lwe
        del kn
    return 0


def table(rows, notes):
    out = ["Packing keyswitch of the prime plans (cntt_prime*_pack_keyswitch_batch, through the NTT mod p) against the direct route",
           "(cntt_prime*_keyswitch_batch on batch * m rows of (k + 1) n words; its rotate-and-sum is not timed), device-resident, caller",
           "workspace, best of three event-timed windows per shape.  w = 64: p = 2^64 - 2^32 + 1; w = 32: p = 1062862849.  Lin = k n, k = 1.",
           "direct*: timed on `rows timed` rows and scaled by the row count.  ratio = direct / pack; spread: max / min - 1 of the three",
           "windows (pack / direct): the direct route's is the run-to-run noise.", ""]
    out.append("%-8s %3s %5s %4s %3s %6s %5s %11s %12s %10s %8s %14s" % ("label", "w", "n", "beta", "l", "batch", "m", "pack ms", "direct ms",
                                                                         "rows timed", "ratio", "spread"))
    for r in rows:
        if "direct_ms" in r:
            out.append("%-8s %3d %5d %4d %3d %6d %5d %11.4f %11.4f%s %10d %8.2f %6.1f%% /%5.1f%%" % (
                r["label"], r["w"], r["n"], r["base_log"], r["levels"], r["batch"], r["m"], min(r["pack_ms"]), min(r["direct_ms"]),
                "*" if r["direct_extrapolated"] else " ", r["direct_rows_timed"], r["direct_over_pack"], 100 * r["pack_spread"],
                100 * r["direct_spread"]))
        else:
            out.append("%-8s %3d %5d %4d %3d %6d %5d %11.4f %12s %10s %8s %6.1f%%" % (
                r["label"], r["w"], r["n"], r["base_log"], r["levels"], r["batch"], r["m"], min(r["pack_ms"]), "-", "-", "-",
                100 * r["pack_spread"]))
    for key in sorted({(r["label"], r["w"], r["n"], r["batch"]) for r in rows if "direct_ms" in r}):
        mine = sorted((r for r in rows if "direct_ms" in r and (r["label"], r["w"], r["n"], r["batch"]) == key), key=lambda r: r["m"])
        over = [r["m"] for r in mine if r["direct_over_pack"] > 1 + max(r["direct_spread"], r["pack_spread"])]
        first = [r for r in mine if r["m"] == min(over)][0] if over else None
        out.append("w = %d, n = %d, batch = %d: the NTT route is the faster one (by more than the noise) from m = %s of the m timed %s%s" % (
            key[1], key[2], key[3], first["m"] if first else "none", [r["m"] for r in mine],
            " -- against a direct time EXTRAPOLATED from %d rows, not measured" % first["direct_rows_timed"]
            if first and first["direct_extrapolated"] else ""))
    return "\n".join(out + [""] + notes) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, metavar="W")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_prime_pack.txt"))
    ap.add_argument("--words", default="64")
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--batches", default="1")
    ap.add_argument("--counts", default="1,8,64,0", help="lwe_count per GLWE; 0 stands for n")
    ap.add_argument("--gadget", default="4x3")
    ap.add_argument("--max-rows", type=int, default=4096, help="rows the direct route is timed on at most")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--label", default="-")
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]
    gadget = tuple(int(x) for x in args.gadget.split("x"))
    if args.one:
        return one(args.one, ints(args.sizes), ints(args.batches), ints(args.counts), gadget, args.max_rows, not args.no_baseline, args.label)
    rows, notes = [], ["before: " + "; ".join(smi())]
    rc = 0
    for w in ints(args.words):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(w), "--sizes", args.sizes,
               "--batches", args.batches, "--counts", args.counts, "--gadget", args.gadget, "--max-rows", str(args.max_rows), "--label",
               args.label] + (["--no-baseline"] if args.no_baseline else [])
        p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:
            print(line, end="", flush=True)
            try:
                rows.append(json.loads(line))
            except ValueError:
                continue
        rc = p.wait()
        if rc != 0:   # a failed, faulted or timed-out width ends the sweep: nothing more runs on the GPU
            notes.append("stopped at w = %d: exit %d" % (w, rc))
            break
    notes.append("after: " + "; ".join(smi()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(table(rows, notes))
    return rc


if __name__ == "__main__":
    sys.exit(main())
