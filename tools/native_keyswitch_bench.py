#!/usr/bin/env python3
"""Timing of the LWE keyswitch (include/cntt_keyswitch.h) on device-resident data.  Per shape: time per call (three repetitions of a
warmed-up, event-timed window; their spread is the run-to-run noise), multiply-accumulates per second, the fraction of the VALU issue
bound implied by the instructions per multiply-accumulate counted in the disassembly of the built kernel, and the key bytes actually
read, ceil(batch / tile) * |ksk|, against 8 TB/s.  Then the share of the keyswitch in cntt_native_keyswitch_bootstrap_batch, the
bootstrap timed by the method of tools/native_pbs_bench.py in the same process.  One fresh process per word width under `timeout`;
the driver prints one JSON line per shape, the GPU clock / power read before and after (rocm-smi, read-only), and writes the table.
    python tools/native_keyswitch_bench.py [--out profiles/r10_native_keyswitch.txt] [--words 32,64] [--batches 1,64,1024,16384]
    python tools/native_keyswitch_bench.py --one W        (all shapes of one word width, this process; JSON lines on stdout)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Counted in the disassembly of native_keyswitch_kernel's main loop (hipcc -O3, gfx950; two key rows per trip):
#   u32   131 instructions for 64 multiply-accumulates, 103 of them VALU: 64 v_mul_lo_u32, 34 v_add3_u32, 4 v_lshl_add_u64 (addresses)
#   u64   199 for 64, 169 VALU: 64 v_mad_u64_u32, 64 v_mul_lo_u32, 32 v_add3_u32, 8 v_lshl_add_u64
#   u128  473 for 32, 381 VALU: 128 v_mad_u64_u32, 128 v_add_co / v_addc_co, 100 v_mov_b32
VALU_PER_MAC = {32: 103 / 64, 64: 169 / 64, 128: 381 / 32}
TILE_B = {32: 64, 64: 64, 128: 32}
# the issue bound: every VALU instruction at full rate, 32 lanes per cycle per SIMD, 4 SIMDs x 256 CUs at 2.4 GHz.  The 32-bit
# multiplies may take more than one pass; the fraction below then reads low by that factor, which is the point of recording it.
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
HBM_BYTES_PER_S = 8e12


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def timed(torch, fn, min_s=0.3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 0
    while time.perf_counter() - t0 < 0.1:   # warm-up and rep count
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


def one(w, batches, lins, louts, gadgets):
    sys.path.insert(0, ROOT)
    import torch

    from concrete_ntt_amd import native32, native64
    plan = {32: native32.Plan32, 64: native64.Plan32}[w].try_new(1024)
    dt = torch.int64 if w == 64 else torch.int32
    lo, hi = -(1 << (w - 1)), (1 << (w - 1)) - 1
    g = torch.Generator(device="cuda").manual_seed(w)
    for lin in lins:
        for lout in louts:
            for beta, ell in gadgets:
                ksk = torch.randint(lo, hi, (lin * ell * (lout + 1),), dtype=dt, device="cuda", generator=g)
                for batch in batches:
                    lwe = torch.randint(lo, hi, (batch * (lin + 1),), dtype=dt, device="cuda", generator=g)
                    out = torch.zeros(batch * (lout + 1), dtype=dt, device="cuda")
                    ms = [timed(torch, lambda: plan.keyswitch_batch(out, lwe, ksk, lin, lout, beta, ell)) for _ in range(3)]
                    best = min(ms)
                    macs = batch * lin * ell * (lout + 1)
                    key_read = -(-batch // TILE_B[w]) * ksk.numel() * (w // 8)
                    print(json.dumps({
                        "w": w, "lin": lin, "lout": lout, "base_log": beta, "levels": ell, "batch": batch,
                        "ms": [round(x, 4) for x in ms], "spread": round(max(ms) / best - 1, 4),
                        "gmac_per_s": round(macs / best / 1e6, 2),
                        "valu_bound_ms": round(macs * VALU_PER_MAC[w] / LANE_OPS_PER_S * 1e3, 4),
                        "valu_fraction": round(macs * VALU_PER_MAC[w] / LANE_OPS_PER_S * 1e3 / best, 4),
                        "key_mb": round(ksk.numel() * (w // 8) / 1e6, 2), "key_read_mb": round(key_read / 1e6, 1),
                        "key_bound_ms": round(key_read / HBM_BYTES_PER_S * 1e3, 4),
                        "key_fraction": round(key_read / HBM_BYTES_PER_S * 1e3 / best, 4)}), flush=True)
    if w != 64:
        return 0
    # the share of the keyswitch in the combined call: native64, n = 1024, k = 1, L = 630, bootstrap base_log 8 levels 3, keyswitch (4, 3)
    n, k, L, beta, ell, ks_beta, ks_ell = 1024, 1, 630, 8, 3, 4, 3
    J, O = (k + 1) * ell, k + 1
    kr = [torch.empty(L * J * O * n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    chunk = max(1, L // 8)
    for i in range(0, L, chunk):   # the key in pieces: the coefficient form of all of it need not exist at once
        c = min(chunk, L - i)
        keyw = torch.randint(lo, hi, (c * J * O * n,), dtype=dt, device="cuda", generator=g)
        plan.fwd_batch(keyw, [p[i * J * O * n:(i + c) * J * O * n] for p in kr])
    del keyw
    lut = torch.randint(lo, hi, (O * n,), dtype=dt, device="cuda", generator=g)
    ksk = torch.randint(lo, hi, (k * n * ks_ell * (L + 1),), dtype=dt, device="cuda", generator=g)
    for batch in (64, 1024):
        ct = torch.randint(lo, hi, (batch * (k * n + 1),), dtype=dt, device="cuda", generator=g)
        mid = torch.zeros(batch * (L + 1), dtype=dt, device="cuda")
        out = torch.zeros_like(ct)
        ws = torch.zeros(plan.ks_pbs_workspace_bytes(L, k, ell, batch), dtype=torch.uint8, device="cuda")
        calls = {"keyswitch": lambda: plan.keyswitch_batch(mid, ct, ksk, k * n, L, ks_beta, ks_ell),
                 "bootstrap": lambda: plan.bootstrap_batch(out, mid, lut, kr, L, k, beta, ell, workspace=ws),
                 "combined": lambda: plan.keyswitch_bootstrap_batch(out, ct, ksk, ks_beta, ks_ell, lut, kr, L, k, beta, ell, workspace=ws)}
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, fn in calls.items():
                ms[name].append(round(timed(torch, fn), 4))
        print(json.dumps({"share": True, "n": n, "k": k, "lwe_dim": L, "batch": batch, **{name + "_ms": v for name, v in ms.items()},
                          "keyswitch_share": round(min(ms["keyswitch"]) / min(ms["combined"]), 5)}), flush=True)
    return 0


def table(rows, shares, notes):
    out = ["LWE keyswitch (cntt_native_keyswitch_batch), device-resident, best of three event-timed windows per shape.",
           "valu%%: time at the VALU issue bound (VALU instructions per multiply-accumulate from the disassembly: u32 %.2f, u64 %.2f; every"
           % (VALU_PER_MAC[32], VALU_PER_MAC[64]),
           "instruction at full rate, 1024 SIMDs x 32 lanes x 2.4 GHz) over the measured time.  key%: ceil(batch / tile) * |ksk| at 8 TB/s over",
           "the measured time (tile = 64 batch elements).  spread: max / min - 1 of the three windows.", ""]
    out.append("%3s %5s %5s %4s %3s %6s %10s %7s %9s %6s %9s %6s" % ("w", "Lin", "Lout", "beta", "l", "batch", "ms", "spread", "GMAC/s", "valu%",
                                                                   "key MB rd", "key%"))
    for r in rows:
        out.append("%3d %5d %5d %4d %3d %6d %10.4f %6.1f%% %9.1f %5.1f%% %9.1f %5.1f%%" % (
            r["w"], r["lin"], r["lout"], r["base_log"], r["levels"], r["batch"], min(r["ms"]), 100 * r["spread"], r["gmac_per_s"],
            100 * r["valu_fraction"], r["key_read_mb"], 100 * r["key_fraction"]))
    out.append("")
    for s in shares:
        out.append("share in cntt_native_keyswitch_bootstrap_batch, native64 n = %d k = %d L = %d batch %d: keyswitch %.4f ms, bootstrap %.3f ms, "
                   "combined %.3f ms -> %.3f %%" % (s["n"], s["k"], s["lwe_dim"], s["batch"], min(s["keyswitch_ms"]), min(s["bootstrap_ms"]),
                                                    min(s["combined_ms"]), 100 * s["keyswitch_share"]))
    return "\n".join(out + [""] + notes) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", type=int, metavar="W")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_native_keyswitch.txt"))
    ap.add_argument("--words", default="32,64")
    ap.add_argument("--lins", default="1024,2048")
    ap.add_argument("--louts", default="630,750")
    ap.add_argument("--gadgets", default="3x5,4x3")
    ap.add_argument("--batches", default="1,64,1024,16384")
    ap.add_argument("--timeout", type=int, default=500)
    args = ap.parse_args()
    ints = lambda s: [int(x) for x in s.split(",")]
    gadgets = [tuple(int(x) for x in g.split("x")) for g in args.gadgets.split(",")]
    if args.one:
        return one(args.one, ints(args.batches), ints(args.lins), ints(args.louts), gadgets)
    rows, shares, notes = [], [], ["before: " + "; ".join(smi())]
    rc = 0
    for w in ints(args.words):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(w), "--lins", args.lins,
               "--louts", args.louts, "--gadgets", args.gadgets, "--batches", args.batches]
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
