#!/usr/bin/env python3
"""Timing of the native plans' multi-bit bootstrap (include/cntt_multibit.h) against the classic one, on device-resident data, all
shapes in ONE process:
    classic        cntt_native_bootstrap_batch with a caller workspace (the baseline; its windows' spread is the run-to-run noise)
    g1/g2/g3/g4    cntt_native_multibit_bootstrap_batch with grouping 1 ... 4 at the same (n, k, L, base_log, levels, batch)
    kernel         cntt_native_multibit_accumulate_batch alone at the bootstrap's (nterms, nout), all residue planes in its one launch:
                   ms per launch and its share of one group step (the step = the bootstrap's time / groups)
A warm-up call, then `--reps` event-timed windows per variant, interleaved.  native64 Plan32, k = 1.  Keys are random canonical residues:
they time the same as real ones.  There is no dispatch between the two calls -- they take different keys -- so the record reports both,
the losing shapes included.  One line per shape is appended to --out as soon as it is measured.
    python tools/native_multibit_bench.py [--sizes 1024,2048] [--settings 22x1,11x2] [--batches 1,16,256,4096] [--lwe-dim 720] [--reps 2]
                                          [--out profiles/r18_native_multibit.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMES32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801]   # the residue primes of native64 Plan32
GROUPINGS = (1, 2, 3, 4)

HEAD = """r18: multi-bit bootstrap of the native plans (cntt_native_multibit_bootstrap_batch, g = 1 ... 4) against cntt_native_bootstrap_batch
=================================================================================================================================

Tool:      tools/native_multibit_bench.py (one process; a warm-up call, then event-timed windows per variant, interleaved, on
           device-resident data with a caller workspace).  native64 Plan32, k = 1, L = %d.
Columns:   classic / g1 ... g4: ms per bootstrap call, every window listed (the spread of `classic` is the noise); best = the fastest
           variant by the minimum of its windows; kernel_ms[g] = one launch of the accumulate kernel alone (five planes);
           kernel_share[g] = kernel_ms / (bootstrap ms / groups).
           A group step is 2 * 5 + 4 = 14 launches against 2 per mask word of the classic call.  No dispatch between the calls: they take
           different keys.
Not here:  the lazy four-product sum against a mont_mul-per-term form of the kernel -- that variant was not built, so there is no A/B.
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--settings", default="22x1,11x2")
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--lwe-dim", type=int, default=720)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_native_multibit.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from concrete_ntt_amd import native64
    L, k = a.lwe_dim, 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(HEAD % L)
        f.write("Device:    %s\n\n" % torch.cuda.get_device_name(0))
    rng = np.random.default_rng(18)

    def words(count):
        return torch.from_numpy(rng.integers(0, 2 ** 63, size=count, dtype=np.int64)).cuda()

    def planes(count):
        return [torch.from_numpy(rng.integers(0, p, size=count, dtype=np.uint32).view(np.int32)).cuda() for p in PRIMES32]

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for n in (int(x) for x in a.sizes.split(",")):
        plan = native64.Plan32.try_new(n)
        for beta, levels in (tuple(int(y) for y in x.split("x")) for x in a.settings.split(",")):
            J, O = (k + 1) * levels, k + 1
            keys = {0: planes(L * J * O * n)}
            for g in GROUPINGS:
                keys[g] = planes(((L // g) * J * O << g) * n)
            lut = words(O * n)
            for batch in (int(x) for x in a.batches.split(",")):
                lwe = words(batch * (L + 1))
                ws = torch.zeros(plan.multibit_pbs_workspace_bytes(L, k, levels, 1, batch), dtype=torch.uint8, device="cuda")
                out = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
                calls = {"classic": lambda: plan.bootstrap_batch(out, lwe, lut, keys[0], L, k, beta, levels, workspace=ws)}
                for g in GROUPINGS:
                    calls["g%d" % g] = (lambda g=g: plan.multibit_bootstrap_batch(out, lwe, lut, keys[g], L, k, beta, levels, g, workspace=ws))
                for fn in calls.values():
                    fn()
                torch.cuda.synchronize()
                ms = {name: [] for name in calls}
                for _ in range(a.reps):
                    for name, fn in calls.items():
                        ms[name].append(round(timed(fn), 3))
                row = {"n": n, "base_log": beta, "levels": levels, "batch": batch, "ms": ms,
                       "best": min(ms, key=lambda name: min(ms[name])), "kernel_ms": {}, "kernel_share": {}}
                terms, acc = planes(batch * J * n), planes(batch * O * n)
                for g in GROUPINGS:
                    rows = torch.from_numpy(rng.integers(0, 2 * n, size=g * batch, dtype=np.uint32).view(np.int32)).cuda()
                    grp = [x[:(J * O << g) * n] for x in keys[g]]
                    plan.multibit_accumulate_batch(acc, terms, rows, grp, J, O, g)
                    t = timed(lambda: [plan.multibit_accumulate_batch(acc, terms, rows, grp, J, O, g) for _ in range(20)]) / 20
                    row["kernel_ms"][g] = round(t, 4)
                    row["kernel_share"][g] = round(t / (min(ms["g%d" % g]) / (L // g)), 3)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
