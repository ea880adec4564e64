#!/usr/bin/env python3
"""Timing of the prime plans' LWE keyswitch (include/cntt_prime_keyswitch.h) on device-resident data, after
tools/native_keyswitch_bench.py.  Per word width (u32: p = 4293918721, W = 32; u64: p = 4611686018427322369, W = 62), at 2048 -> 742,
batch 4096, base_log 3 levels 5 and at the wide-digit setting base_log 31 levels 1 (a chunk of two rows): time per call of
cntt_prime*_keyswitch_batch and, in the same process on the same box, of cntt_native_keyswitch_batch of the same word width and shape
(three repetitions of a warmed-up, event-timed window; their spread is the run-to-run noise), multiply-accumulates per second, and the
fraction of the VALU issue bound implied by the VALU instructions per multiply-accumulate counted in the disassembly of the built
kernels.  Then, on u64 words, cntt_prime64_keyswitch_bootstrap_batch against its two halves.  One fresh process per word width under
`timeout`; the driver prints one JSON line per measurement, the GPU clock / power read before and after (rocm-smi, read-only), and
writes the table.
    python tools/prime_keyswitch_bench.py [--out profiles/r13_prime_keyswitch.txt] [--words 32,64] [--batch 4096]
    python tools/prime_keyswitch_bench.py --one W        (one word width, this process; JSON lines on stdout)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from native_keyswitch_bench import LANE_OPS_PER_S, VALU_PER_MAC as NATIVE_VALU_PER_MAC, smi, timed  # noqa: E402

# Counted in the disassembly of prime_keyswitch_kernel's row loop (hipcc -O3, gfx950; two key rows = 32 multiply-accumulates per trip):
#   u32    70 instructions, 43 of them VALU: 32 v_mad_u64_u32, 8 v_lshl_add_u64 (addresses and the key-word sums), 3 v_mov_b32
#   u64   109 instructions, 81 VALU: 64 v_mad_u64_u32, 8 v_lshl_add_u64, 4 v_cmp_lt_u64 + 2 v_addc_co + 2 v_cndmask (key-word sums), 1 v_mov
VALU_PER_MAC = {32: 43 / 32, 64: 81 / 32}
PRIME = {32: 4293918721, 64: 4611686018427322369}
SETTINGS = [(3, 5), (31, 1)]


def one(w, batch, lin, lout):
    sys.path.insert(0, ROOT)
    import torch

    from concrete_ntt_amd import native32, native64, prime32, prime64
    p = PRIME[w]
    plan = {32: prime32, 64: prime64}[w].Plan.try_new(1024, p)
    nplan = {32: native32.Plan32, 64: native64.Plan32}[w].try_new(1024)
    dt = torch.int64 if w == 64 else torch.int32
    g = torch.Generator(device="cuda").manual_seed(w)

    def words(count, mod=None):   # canonical words below p (mod None: any word), in the signed dtype torch has
        hi = mod if mod is not None else 1 << w
        t = torch.randint(0, min(hi, (1 << 63) - 1), (count,), dtype=torch.int64, device="cuda", generator=g)
        return t if w == 64 else t.to(torch.int32)   # the conversion wraps: the low 32 bits

    macs = batch * lin * (lout + 1)
    for beta, ell in SETTINGS:
        ksk, lwe = words(lin * ell * (lout + 1), p), words(batch * (lin + 1), p)
        out = torch.zeros(batch * (lout + 1), dtype=dt, device="cuda")
        for name, pl, vpm in (("prime", plan, VALU_PER_MAC[w]), ("native", nplan, NATIVE_VALU_PER_MAC[w])):
            ms = [timed(torch, lambda: pl.keyswitch_batch(out, lwe, ksk, lin, lout, beta, ell)) for _ in range(3)]
            best, m = min(ms), macs * ell
            print(json.dumps({"call": name, "w": w, "lin": lin, "lout": lout, "base_log": beta, "levels": ell, "batch": batch,
                              "ms": [round(x, 4) for x in ms], "spread": round(max(ms) / best - 1, 4), "gmac_per_s": round(m / best / 1e6, 2),
                              "valu_per_mac": round(vpm, 3), "valu_bound_ms": round(m * vpm / LANE_OPS_PER_S * 1e3, 4),
                              "valu_fraction": round(m * vpm / LANE_OPS_PER_S * 1e3 / best, 4)}), flush=True)
    if w != 64:
        return 0
    # the combined call against its two halves: prime64, n = 1024, k = 1, L = 630, bootstrap base_log 8 levels 3, keyswitch (4, 3)
    n, k, L, beta, ell, ks_beta, ks_ell = 1024, 1, 630, 8, 3, 4, 3
    bsk = words(L * (k + 1) * ell * (k + 1) * n, p)      # any canonical words time as a key does
    lut, ksk = words((k + 1) * n, p), words(k * n * ks_ell * (L + 1), p)
    for b in (64, 1024):
        ct = words(b * (k * n + 1), p)
        mid, res = torch.zeros(b * (L + 1), dtype=dt, device="cuda"), torch.zeros_like(ct)
        ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, b), dtype=torch.uint8, device="cuda")
        calls = {"keyswitch": lambda: plan.keyswitch_batch(mid, ct, ksk, k * n, L, ks_beta, ks_ell),
                 "bootstrap": lambda: plan.bootstrap_batch(res, mid, lut, bsk, L, k, beta, ell, workspace=ws),
                 "combined": lambda: plan.keyswitch_bootstrap_batch(res, ct, ksk, ks_beta, ks_ell, lut, bsk, L, k, beta, ell, workspace=ws)}
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, fn in calls.items():
                ms[name].append(round(timed(torch, fn), 4))
        print(json.dumps({"share": True, "n": n, "k": k, "lwe_dim": L, "batch": b, **{name + "_ms": v for name, v in ms.items()},
                          "combined_over_halves": round(min(ms["combined"]) / (min(ms["keyswitch"]) + min(ms["bootstrap"])), 5),
                          "keyswitch_share": round(min(ms["keyswitch"]) / min(ms["combined"]), 5)}), flush=True)
    return 0


def table(rows, shares, notes):
    out = ["LWE keyswitch mod p (cntt_prime*_keyswitch_batch) against cntt_native_keyswitch_batch of the same word width and shape, same box,",
           "same process; device-resident, best of three event-timed windows.  valu%: time at the VALU issue bound (VALU instructions per",
           "multiply-accumulate from the disassembly; every instruction at full rate, 1024 SIMDs x 32 lanes x 2.4 GHz) over the measured time.",
           "MACs per output word = Lin * levels.  spread: max / min - 1 of the three windows.", ""]
    out.append("%-6s %3s %5s %5s %4s %3s %6s %10s %7s %9s %9s %6s" % ("call", "w", "Lin", "Lout", "beta", "l", "batch", "ms", "spread", "GMAC/s",
                                                                   "VALU/MAC", "valu%"))
    for r in rows:
        out.append("%-6s %3d %5d %5d %4d %3d %6d %10.4f %6.1f%% %9.1f %9.2f %5.1f%%" % (
            r["call"], r["w"], r["lin"], r["lout"], r["base_log"], r["levels"], r["batch"], min(r["ms"]), 100 * r["spread"], r["gmac_per_s"],
            r["valu_per_mac"], 100 * r["valu_fraction"]))
    out.append("")
    for i in range(0, len(rows) - 1, 2):
        a, b = rows[i], rows[i + 1]
        if a["call"] == "prime" and b["call"] == "native":
            out.append("prime / native, u%d base_log %d levels %d: %.3f" % (a["w"], a["base_log"], a["levels"], min(a["ms"]) / min(b["ms"])))
    out.append("")
    for s in shares:
        out.append("cntt_prime64_keyswitch_bootstrap_batch, n = %d k = %d L = %d batch %d: keyswitch %.4f ms + bootstrap %.3f ms, combined %.3f ms "
                   "(%.4f of the two halves; the keyswitch is %.3f %% of it)" % (
                       s["n"], s["k"], s["lwe_dim"], s["batch"], min(s["keyswitch_ms"]), min(s["bootstrap_ms"]), min(s["combined_ms"]),
                       s["combined_over_halves"], 100 * s["keyswitch_share"]))
    return "\n".join(out + [""] + notes) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, metavar="W")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_prime_keyswitch.txt"))
    ap.add_argument("--words", default="32,64")
    ap.add_argument("--lin", type=int, default=2048)
    ap.add_argument("--lout", type=int, default=742)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--timeout", type=int, default=400)
    args = ap.parse_args()
    if args.one:
        return one(args.one, args.batch, args.lin, args.lout)
    rows, shares, notes = [], [], ["before: " + "; ".join(smi())]
    rc = 0
    for w in [int(x) for x in args.words.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(w), "--lin", str(args.lin),
               "--lout", str(args.lout), "--batch", str(args.batch)]
        p = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, text=True)
        for line in p.stdout:
            print(line, end="", flush=True)
            try:
                d = json.loads(line)
            except ValueError:
                continue
            (shares if d.get("share") else rows).append(d)
        rc = p.wait()
        if rc != 0:   # a failed, faulted or timed-out width ends the sweep: nothing more runs on the GPU
            notes.append("stopped at w = %d: exit %d" % (w, rc))
            break
    notes.append("after: " + "; ".join(smi()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(table(rows, shares, notes))
    return rc


if __name__ == "__main__":
    sys.exit(main())
