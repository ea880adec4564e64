#!/usr/bin/env python3
"""Timing of the prime plans' programmable bootstrap (include/cntt_prime_pbs.h) on device-resident data, one process per shape:
    one_call   cntt_prime64_bootstrap_batch with a caller workspace: modulus switch, set-up, L iterations in place, extraction
    loop       the caller-side loop over the public calls in the same process: L times cntt_prime64_gadget_decompose_batch (CMUX) and
               cntt_prime64_external_product_batch (accumulate) on one buffer.  Its modulus switch, set-up and extraction are LEFT OUT of
               the timed region, so `loop` does strictly less work than `one_call`.
    gadget     L calls of the decomposition alone (CMUX): the share of prime_gadget_kernel in the loop
    native64   cntt_native_bootstrap_batch (native64 Plan32: five 30-bit transforms, split and CRT) at the same (n, k, L, levels), for context
Three repetitions each, interleaved: the spread of `loop` is the run-to-run noise `one_call` is judged against.  Once per shape the
accumulator of cntt_prime64_blind_rotate_batch is compared word for word with the loop's.  k = 1.  Every shape runs in a fresh process
under `timeout`; the driver writes one JSON line per shape and the GPU clock / power read before and after (rocm-smi, read-only) to
profiles/r12_prime_pbs.txt.
    python tools/prime_pbs_bench.py [--primes 4611686018427322369,18446744069414584321] [--sizes 1024] [--levels 2,3] [--batches 64,1024]
                                    [--lwe-dim 128] [--out profiles/r12_prime_pbs.txt]
    python tools/prime_pbs_bench.py --one P N LEVELS BASE_LOG LWE_DIM BATCH        (one shape, this process)"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE_LOG = {2: 15, 3: 8, 4: 6}   # by levels (as tools/native_pbs_bench.py for 64-bit words)
HEAD = """r12: programmable bootstrap of the prime plans (cntt_prime64_bootstrap_batch) against the caller-side loop and the native64 bootstrap
====================================================================================================================================

Tool:      tools/prime_pbs_bench.py (one process per shape under a time limit; three warmed-up, event-timed windows per variant,
           interleaved, on device-resident data; clock and power read through rocm-smi before and after the sweep).  k = 1.
Columns:   one_call / loop / gadget / native64 in ms per call (three windows each); one_call_vs_loop > 1: the one call is faster than
           the loop of public calls (which leaves its modulus switch, set-up and extraction untimed); gadget_share = the decomposition
           kernel's part of the loop; prime_vs_native64 > 1: the prime bootstrap is faster than cntt_native_bootstrap_batch.
"""


def smi():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=30)
        keep = [ln.strip() for ln in r.stdout.splitlines() if "sclk" in ln or "mclk" in ln or "Power" in ln]
        return keep[:6]
    except Exception as e:  # no rocm-smi: record why
        return ["rocm-smi unavailable: %s" % e]


def one(p, n, levels, beta, L, batch):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from concrete_ntt_amd import native64, prime64
    plan = prime64.Plan.try_new(n, p)
    k = 1
    J, O = (k + 1) * levels, k + 1
    rng = np.random.default_rng(1000 * n + 10 * J + beta)

    def words(count):
        return torch.from_numpy(rng.integers(0, p, size=count, dtype=np.uint64).view(np.int64)).cuda()

    lwe, lut, bsk = words(batch * (L + 1)), words(O * n), words(L * J * O * n)   # any canonical words time the same
    ws = torch.zeros(plan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")
    out = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
    rot_t = torch.zeros((L + 1) * batch, dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe, L)
    acc = torch.zeros(batch * O * n, dtype=torch.int64, device="cuda")
    buf = torch.zeros_like(acc)
    terms = torch.zeros(batch * J * n, dtype=torch.int64, device="cuda")
    slice_ = J * O * n
    keys = [bsk[i * slice_:(i + 1) * slice_] for i in range(L)]
    rots = [rot_t[i * batch:(i + 1) * batch] for i in range(L + 1)]

    nplan = native64.Plan32.try_new(n)
    g = torch.Generator(device="cuda").manual_seed(7)
    nkr = [torch.randint(0, 1 << 29, (L * J * O * n,), dtype=torch.int32, device="cuda", generator=g) for _ in range(nplan.NPRIMES)]
    nws = torch.zeros(nplan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")

    def one_call():
        plan.bootstrap_batch(out, lwe, lut, bsk, L, k, beta, levels, workspace=ws)

    def loop():
        for i in range(L):
            plan.gadget_decompose_batch(terms, buf, beta, levels, rot=rots[i], mode="cmux")
            plan.external_product_batch(buf, terms, keys[i], J, O, accumulate=True)

    def gadget():
        for i in range(L):
            plan.gadget_decompose_batch(terms, buf, beta, levels, rot=rots[i], mode="cmux")

    def native():
        nplan.bootstrap_batch(out, lwe, lut, nkr, L, k, beta, levels, workspace=nws)

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
    plan.blind_rotate_batch(acc, lut, rot_t, bsk, L, k, beta, levels, workspace=ws)
    plan.gadget_decompose_batch(buf, lut.repeat(batch), p.bit_length(), 1, rot=rots[L], mode="rotate")   # X^a lut: the one full-width digit
    loop()
    torch.cuda.synchronize()
    identical = bool(torch.equal(buf, acc))
    res = {"p": p, "n": n, "k": k, "levels": levels, "base_log": beta, "lwe_dim": L, "batch": batch, "identical": identical}
    ms = {"one_call": [], "loop": [], "gadget": [], "native64": []}
    for _ in range(3):
        for name, fn in (("one_call", one_call), ("loop", loop), ("gadget", gadget), ("native64", native)):
            ms[name].append(round(timed(fn), 4))
    res.update({name + "_ms": ms[name] for name in ms})
    res["loop_spread"] = round(max(ms["loop"]) / min(ms["loop"]) - 1, 4)
    res["one_call_vs_loop"] = round(min(ms["loop"]) / min(ms["one_call"]), 4)
    res["gadget_share"] = round(min(ms["gadget"]) / min(ms["loop"]), 4)
    res["prime_vs_native64"] = round(min(ms["native64"]) / min(ms["one_call"]), 4)
    print(json.dumps(res), flush=True)
    return 0 if identical else 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=6, metavar=("P", "N", "LEVELS", "BASE_LOG", "LWE_DIM", "BATCH"))
    ap.add_argument("--primes", default="4611686018427322369,18446744069414584321")
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--levels", default="2,3")
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--lwe-dim", type=int, default=128)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_prime_pbs.txt"))
    args = ap.parse_args()
    if args.one:
        return one(*[int(x) for x in args.one])
    lines = [json.dumps({"smi_before": smi()})]
    rc = 0
    for p in [int(x) for x in args.primes.split(",")]:
        for n in [int(x) for x in args.sizes.split(",")]:
            for levels in [int(x) for x in args.levels.split(",")]:
                for batch in [int(x) for x in args.batches.split(",")]:
                    if rc:
                        continue
                    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", str(p), str(n),
                           str(levels), str(BASE_LOG[levels]), str(args.lwe_dim), str(batch)]
                    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
                    lines += [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                    if r.returncode != 0:   # a failed, faulted or timed-out shape ends the sweep: nothing more runs on the GPU
                        lines.append(json.dumps({"stopped": cmd[6:], "exit": r.returncode, "stderr": r.stderr[-400:]}))
                        rc = r.returncode
    lines.append(json.dumps({"smi_after": smi()}))
    text = HEAD + "\nMeasured on one MI355X:\n" + "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
