#!/usr/bin/env python3
"""A/B timing of the external product on undecomposed polynomials (include/cntt_gadget.h) on device-resident data, in one process
per shape:
    fused      cntt_native_external_product_decomposed_batch with the testing switch native_gadget = 1: fused kernel (native_gadget.hpp)
    split      cntt_native_gadget_decompose_batch, then cntt_native_external_product_batch on its output, then the addend
               (three repetitions: their spread is the run-to-run noise the fused time is judged against)
    off        the same call with native_gadget = 0 (the library's default: it composes the two calls of `split` itself)
Mode CMUX, nout = npolys, addend = polys (the blind-rotation update).  The outputs are compared word for word once per shape.
Every shape runs in a fresh process under `timeout`; the driver prints one JSON line per shape and the GPU clock / power read
before and after (rocm-smi, read-only).
    python tools/native_gadget_bench.py [--kinds native64,native_binary64] [--sizes 1024,2048,4096] [--batch 16384]
    python tools/native_gadget_bench.py --one KIND N NPOLYS LEVELS BASE_LOG BATCH        (one shape, this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 1, 23), (2, 2, 15), (2, 3, 8), (3, 2, 12), (4, 1, 22)]   # (npolys, levels, base_log)


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def one(kind, n, npolys, levels, beta, batch):
    sys.path.insert(0, ROOT)
    import torch

    import concrete_ntt_amd as cntt
    from concrete_ntt_amd import native64, native_binary64
    plan = {"native64": native64.Plan32, "native_binary64": native_binary64.Plan32}[kind].try_new(n)
    J, O = npolys * levels, npolys
    assert plan.max_terms() >= J
    g = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * J + beta)
    lo, hi = -(1 << 63), (1 << 63) - 1
    polys = torch.randint(lo, hi, (batch * npolys * n,), dtype=torch.int64, device="cuda", generator=g)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=g)
    keyw = torch.randint(0, 2, (J * O * n,), dtype=torch.int64, device="cuda", generator=g) if plan.BINARY else \
        torch.randint(lo, hi, (J * O * n,), dtype=torch.int64, device="cuda", generator=g)
    kr = [torch.empty(J * O * n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(keyw, kr, binary=plan.BINARY)
    out = torch.zeros(batch * O * n, dtype=torch.int64, device="cuda")
    terms = torch.empty(batch * J * n, dtype=torch.int64, device="cuda")

    def call():
        plan.external_product_decomposed_batch(out, polys, kr, beta, levels, O, rot=rot, mode="cmux", addend=polys)

    def fused():
        cntt.debug_set("native_gadget", 1)
        call()
        cntt.debug_set("native_gadget", -1)

    def split():
        plan.gadget_decompose_batch(terms, polys, beta, levels, rot=rot, mode="cmux")
        plan.external_product_batch(out, terms, kr, J, O)
        out.add_(polys)   # int64 add: wraps modulo 2^64

    def off():
        cntt.debug_set("native_gadget", 0)
        call()
        cntt.debug_set("native_gadget", -1)

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

    outs = []
    for fn in (fused, split, off):
        fn()
        torch.cuda.synchronize()
        outs.append(out.clone())
    identical = bool(torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]))
    res = {"kind": kind, "n": n, "npolys": npolys, "levels": levels, "base_log": beta, "batch": batch, "identical": identical}
    ms = {"fused": [], "split": [], "off": []}
    for _ in range(3):
        for name, fn in (("fused", fused), ("split", split), ("off", off)):
            ms[name].append(round(timed(fn), 4))
    res.update({name + "_ms": ms[name] for name in ms})
    res["split_spread"] = round(max(ms["split"]) / min(ms["split"]) - 1, 4)
    res["fused_vs_split"] = round(min(ms["split"]) / min(ms["fused"]), 3)
    print(json.dumps(res), flush=True)
    return 0 if identical else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=6, metavar=("KIND", "N", "NPOLYS", "LEVELS", "BASE_LOG", "BATCH"))
    ap.add_argument("--kinds", default="native64,native_binary64")
    ap.add_argument("--sizes", default="1024,2048,4096")
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--timeout", type=int, default=240)
    args = ap.parse_args()
    if args.one:
        k, *rest = args.one
        return one(k, *[int(x) for x in rest])
    print(json.dumps({"smi_before": smi()}), flush=True)
    for kind in args.kinds.split(","):
        for n in [int(x) for x in args.sizes.split(",")]:
            for npolys, levels, beta in SHAPES:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", kind, str(n),
                       str(npolys), str(levels), str(beta), str(args.batch)]
                r = subprocess.run(cmd, cwd=ROOT)
                if r.returncode != 0:   # a failed, faulted or timed-out shape ends the sweep: nothing more runs on the GPU
                    print(json.dumps({"stopped": cmd[6:], "exit": r.returncode}), flush=True)
                    print(json.dumps({"smi_after": smi()}), flush=True)
                    return r.returncode
    print(json.dumps({"smi_after": smi()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
