#!/usr/bin/env python3
"""A/B timing of the native external product (include/cntt_ext.h) on device-resident data, three paths per shape:
    fused      cntt_native_external_product_batch, fused kernel (native_ext.hpp)
    composed   the same call with the testing switch native_ext = 0 (split + one mul_accumulate chain per prime + CRT)
    naive      J x O negacyclic_polymul_batch calls (key words tiled over the batch) + a wrapping add per product
All three outputs are compared word for word once per shape.  HBM fraction: the algorithmic bytes (J + O) n w per element over the
time, against 8 TB/s.  Every shape runs in a fresh process under `timeout`; the driver prints one JSON line per shape and the GPU
clock / power read before and after (rocm-smi, read-only).
    python tools/native_ext_bench.py [--kinds native64,native_binary64] [--sizes 1024,2048,4096] [--terms 1,2,4,8] [--outs 1,2]
                                     [--batch 16384]
    python tools/native_ext_bench.py --one KIND N J O BATCH        (one shape, this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_BPS = 8e12


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def one(kind, n, J, O, batch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native64, native_binary64
    cls = {"native64": native64.Plan32, "native_binary64": native_binary64.Plan32}[kind]
    plan = cls.try_new(n)
    assert plan.max_terms() >= J
    g = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * J + O)
    lo, hi = -(1 << 63), (1 << 63) - 1
    terms = torch.randint(lo, hi, (batch * J * n,), dtype=torch.int64, device="cuda", generator=g)
    if plan.BINARY:
        keyw = torch.randint(0, 2, (J * O * n,), dtype=torch.int64, device="cuda", generator=g)
    else:
        keyw = torch.randint(lo, hi, (J * O * n,), dtype=torch.int64, device="cuda", generator=g)
    kr = [torch.empty(J * O * n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(keyw, kr, binary=plan.BINARY)
    out = torch.zeros(batch * O * n, dtype=torch.int64, device="cuda")
    # naive path operands: term j of every element contiguous, key[j][o] tiled over the batch
    tj = terms.view(batch, J, n).transpose(0, 1).contiguous()
    tiles = [keyw.view(J, O, n)[j, o].repeat(batch) for j in range(J) for o in range(O)]
    prod = torch.empty(batch * n, dtype=torch.int64, device="cuda")
    outs_n = [torch.zeros(batch, n, dtype=torch.int64, device="cuda") for _ in range(O)]

    def fused():
        plan.external_product_batch(out, terms, kr, J, O)

    def composed():
        cntt.debug_set("native_ext", 0)
        plan.external_product_batch(out, terms, kr, J, O)
        cntt.debug_set("native_ext", -1)

    def naive():
        for o in range(O):
            outs_n[o].zero_()
            for j in range(J):
                plan.negacyclic_polymul_batch(prod, tj[j], tiles[j * O + o])
                outs_n[o].add_(prod.view(batch, n))   # int64 add: wraps modulo 2^64

    def timed(fn, min_s=0.4):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 0
        while time.perf_counter() - t0 < 0.2:   # warm-up and rep count
            fn()
            reps += 1
            torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / reps
        reps = max(3, int(min_s / per))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # outputs first: the three paths must agree word for word
    fused()
    torch.cuda.synchronize()
    a = out.clone()
    composed()
    torch.cuda.synchronize()
    b = out.clone()
    naive()
    torch.cuda.synchronize()
    c = torch.stack(outs_n, 1).reshape(-1)
    identical = bool(torch.equal(a, b) and torch.equal(a, c))
    res = {"kind": kind, "n": n, "J": J, "O": O, "batch": batch, "identical": identical}
    algo = (J + O) * n * 8 * batch
    # alternate the paths twice; keep the faster of each pair
    ms = {"fused": [], "composed": [], "naive": []}
    for _ in range(2):
        for name, fn in (("fused", fused), ("composed", composed), ("naive", naive)):
            ms[name].append(timed(fn))
    for name in ms:
        t = min(ms[name])
        res[name + "_ms"] = round(t, 4)
        res[name + "_ns_per_elem"] = round(t * 1e6 / batch, 1)
        res[name + "_hbm_frac"] = round(algo / (t * 1e-3) / HBM_BPS, 4)
    res["fused_vs_composed"] = round(min(ms["composed"]) / min(ms["fused"]), 3)
    res["fused_vs_naive"] = round(min(ms["naive"]) / min(ms["fused"]), 3)
    print(json.dumps(res), flush=True)
    return 0 if identical else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=5, metavar=("KIND", "N", "J", "O", "BATCH"))
    ap.add_argument("--kinds", default="native64,native_binary64")
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--terms", default="1,2,4,8")
    ap.add_argument("--outs", default="1,2")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.one:
        k, n, J, O, B = args.one
        return one(k, int(n), int(J), int(O), int(B))
    print(json.dumps({"smi_before": smi()}), flush=True)
    for kind in args.kinds.split(","):
        for n in [int(x) for x in args.sizes.split(",")]:
            for J in [int(x) for x in args.terms.split(",")]:
                for O in [int(x) for x in args.outs.split(",")]:
                    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", kind, str(n),
                           str(J), str(O), str(args.batch)]
                    r = subprocess.run(cmd, cwd=ROOT)
                    if r.returncode != 0:   # a failed, faulted or timed-out shape ends the sweep: nothing more runs on the GPU
                        print(json.dumps({"stopped": cmd[6:], "exit": r.returncode}), flush=True)
                        print(json.dumps({"smi_after": smi()}), flush=True)
                        return r.returncode
    print(json.dumps({"smi_after": smi()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
