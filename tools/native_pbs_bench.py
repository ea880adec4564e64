#!/usr/bin/env python3
"""Timing of the programmable bootstrap (include/cntt_pbs.h) on device-resident data, in one process per shape:
    one_call   cntt_native_bootstrap_batch with a caller workspace: modulus switch, set-up, L iterations in place, extraction
    loop       the caller-side loop over the public calls of cntt_gadget.h: L times cntt_native_external_product_decomposed_batch with
               mode CMUX and addend = polys on two buffers that swap.  Its modulus switch, accumulator set-up and sample extraction are
               LEFT OUT of the timed region (the library offered nothing for them), so `loop` does strictly less work than `one_call`.
    ends       the three end kernels alone: modulus switch + blind rotation with lwe_dim = 0 (the set-up) + extraction
Three repetitions each, interleaved: the spread of `loop` is the run-to-run noise `one_call` is judged against.  Once per shape the
accumulator of cntt_native_blind_rotate_batch is compared word for word with the loop's.  k = 1.  Every shape runs in a fresh process
under `timeout`; the driver prints one JSON line per shape and the GPU clock / power read before and after (rocm-smi, read-only).
    python tools/native_pbs_bench.py [--kinds native64,native32] [--sizes 1024,2048] [--levels 2,3,4] [--batches 64,1024,16384] [--lwe-dim 700]
    python tools/native_pbs_bench.py --one KIND N LEVELS BASE_LOG LWE_DIM BATCH        (one shape, this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_LOG = {64: {2: 15, 3: 8, 4: 6}, 32: {2: 8, 3: 6, 4: 4}}   # by word width and levels


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def one(kind, n, levels, beta, L, batch):
    sys.path.insert(0, ROOT)
    import torch

    from concrete_ntt_amd import native32, native64
    plan = {"native64": native64.Plan32, "native32": native32.Plan32}[kind].try_new(n)
    k, w = 1, 8 * plan.WORD
    dt = torch.int64 if w == 64 else torch.int32
    lo, hi = -(1 << (w - 1)), (1 << (w - 1)) - 1
    J, O = (k + 1) * levels, k + 1
    assert plan.max_terms() >= J
    g = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * J + beta)
    lwe = torch.randint(lo, hi, (batch * (L + 1),), dtype=dt, device="cuda", generator=g)
    lut = torch.randint(lo, hi, (O * n,), dtype=dt, device="cuda", generator=g)
    kr = [torch.empty(L * J * O * n, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    chunk = max(1, L // 8)
    for i in range(0, L, chunk):   # the key in pieces: the coefficient form of all of it need not exist at once
        c = min(chunk, L - i)
        keyw = torch.randint(lo, hi, (c * J * O * n,), dtype=dt, device="cuda", generator=g)
        plan.fwd_batch(keyw, [p[i * J * O * n:(i + c) * J * O * n] for p in kr])
    del keyw
    ws = torch.zeros(plan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros(batch * (k * n + 1), dtype=dt, device="cuda")
    rot_t = torch.zeros((L + 1) * batch, dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe, L)
    bufs = [torch.zeros(batch * O * n, dtype=dt, device="cuda") for _ in range(2)]
    acc = torch.zeros_like(bufs[0])
    no_key = [torch.empty(0, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    slice_ = J * O * n
    keys = [[p[i * slice_:(i + 1) * slice_] for p in kr] for i in range(L)]
    rots = [rot_t[i * batch:(i + 1) * batch] for i in range(L + 1)]

    def one_call():
        plan.bootstrap_batch(out, lwe, lut, kr, L, k, beta, levels, workspace=ws)

    def loop():
        a, b = bufs
        for i in range(L):
            plan.external_product_decomposed_batch(b, a, keys[i], beta, levels, O, rot=rots[i], mode="cmux", addend=a)
            a, b = b, a
        return a

    def ends():
        plan.lwe_modswitch_batch(rot_t, lwe, L)
        plan.blind_rotate_batch(acc, lut, rots[L], no_key, 0, k, beta, levels, workspace=ws)
        plan.sample_extract_batch(out, acc, k, 0)

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
        reps = max(2, int(min_s / per))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # the same words: blind_rotate_batch against the loop started from the same set-up
    plan.blind_rotate_batch(acc, lut, rot_t, kr, L, k, beta, levels, workspace=ws)
    plan.gadget_decompose_batch(bufs[0], lut.repeat(batch), w, 1, rot=rots[L], mode="rotate")   # X^a lut: the one full-width digit
    identical = bool(torch.equal(loop(), acc))
    res = {"kind": kind, "n": n, "k": k, "levels": levels, "base_log": beta, "lwe_dim": L, "batch": batch, "identical": identical}
    ms = {"one_call": [], "loop": [], "ends": []}
    for _ in range(3):
        for name, fn in (("one_call", one_call), ("loop", loop), ("ends", ends)):
            ms[name].append(round(timed(fn), 4))
    res.update({name + "_ms": ms[name] for name in ms})
    res["loop_spread"] = round(max(ms["loop"]) / min(ms["loop"]) - 1, 4)
    res["one_call_vs_loop"] = round(min(ms["loop"]) / min(ms["one_call"]), 4)   # > 1: the one call is faster
    res["ends_share"] = round(min(ms["ends"]) / min(ms["one_call"]), 5)
    print(json.dumps(res), flush=True)
    return 0 if identical else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=6, metavar=("KIND", "N", "LEVELS", "BASE_LOG", "LWE_DIM", "BATCH"))
    ap.add_argument("--kinds", default="native64,native32")
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--levels", default="2,3,4")
    ap.add_argument("--batches", default="64,1024,16384")
    ap.add_argument("--lwe-dim", type=int, default=700)
    ap.add_argument("--timeout", type=int, default=400)
    args = ap.parse_args()
    if args.one:
        k, *rest = args.one
        return one(k, *[int(x) for x in rest])
    print(json.dumps({"smi_before": smi()}), flush=True)
    for kind in args.kinds.split(","):
        for n in [int(x) for x in args.sizes.split(",")]:
            for levels in [int(x) for x in args.levels.split(",")]:
                for batch in [int(x) for x in args.batches.split(",")]:
                    beta = BASE_LOG[64 if kind == "native64" else 32][levels]
                    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", kind, str(n),
                           str(levels), str(beta), str(args.lwe_dim), str(batch)]
                    r = subprocess.run(cmd, cwd=ROOT)
                    if r.returncode != 0:   # a failed, faulted or timed-out shape ends the sweep: nothing more runs on the GPU
                        print(json.dumps({"stopped": cmd[6:], "exit": r.returncode}), flush=True)
                        print(json.dumps({"smi_after": smi()}), flush=True)
                        return r.returncode
    print(json.dumps({"smi_after": smi()}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
