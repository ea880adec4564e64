#!/usr/bin/env python3
"""Timing of the prime plans' multi-bit bootstrap (include/cntt_prime_multibit.h) against the classic one, on device-resident data, all
shapes in ONE process:
    classic    cntt_prime64_bootstrap_batch with a caller workspace (the baseline; its windows' spread is the run-to-run noise)
    g2/g3/g4   cntt_prime64_multibit_bootstrap_batch with grouping 2, 3, 4 at the same (n, k, L, base_log, levels, batch)
    kernel     cntt_prime64_multibit_accumulate_batch alone at the bootstrap's (nterms, nout): ms per launch, its share of one group step
               (the step = the bootstrap's time / groups) and its fraction of the HBM roofline on (nterms + nout) * n words per element
A warm-up call, then `--reps` event-timed windows per variant, interleaved.  k = 1, p = 4611686018427322369.  Keys are random canonical
words: they time the same as real ones.  One line per shape is appended to --out as soon as it is measured.
    python tools/prime_multibit_bench.py [--sizes 1024,2048] [--settings 22x1,11x2] [--batches 1,16,256,4096] [--lwe-dim 720] [--reps 2]
                                         [--out profiles/r17_prime_multibit.txt]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4611686018427322369
HBM_BYTES_PER_S = 8.0e12   # MI355X peak

HEAD = """r17: multi-bit bootstrap of the prime plans (cntt_prime64_multibit_bootstrap_batch, g = 2, 3, 4) against cntt_prime64_bootstrap_batch
=================================================================================================================================

Tool:      tools/prime_multibit_bench.py (one process; a warm-up call, then event-timed windows per variant, interleaved, on
           device-resident data with a caller workspace).  p = 4611686018427322369, k = 1, L = %d.
Columns:   classic / g2 / g3 / g4: ms per bootstrap call, every window listed; best = the fastest variant by the minimum of its windows;
           kernel_ms[g] = one launch of the accumulate kernel alone; kernel_share[g] = kernel_ms / (bootstrap ms / groups);
           roofline[g] = (nterms + nout) * n * 8 bytes * batch / kernel_ms against %.1f TB/s.
           The table placement is L2 gathers (no LDS variant was built, so there is no A/B for it).
"""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--settings", default="22x1,11x2")
    ap.add_argument("--batches", default="1,16,256,4096")
    ap.add_argument("--lwe-dim", type=int, default=720)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_prime_multibit.txt"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from concrete_ntt_amd import prime64
    L, k = a.lwe_dim, 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(HEAD % (L, HBM_BYTES_PER_S / 1e12))
        f.write("Device:    %s\n\n" % torch.cuda.get_device_name(0))
    rng = np.random.default_rng(17)

    def words(count):
        return torch.from_numpy(rng.integers(0, P, size=count, dtype=np.uint64).view(np.int64)).cuda()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    for n in (int(x) for x in a.sizes.split(",")):
        plan = prime64.Plan.try_new(n, P)
        for beta, levels in (tuple(int(y) for y in x.split("x")) for x in a.settings.split(",")):
            J, O = (k + 1) * levels, k + 1
            keys = {0: words(L * J * O * n)}
            for g in (2, 3, 4):
                keys[g] = words(((L // g) * J * O << g) * n)
            lut = words(O * n)
            for batch in (int(x) for x in a.batches.split(",")):
                lwe = words(batch * (L + 1))
                ws = torch.zeros(plan.pbs_workspace_bytes(L, k, levels, batch), dtype=torch.uint8, device="cuda")
                out = torch.zeros(batch * (k * n + 1), dtype=torch.int64, device="cuda")
                calls = {"classic": lambda: plan.bootstrap_batch(out, lwe, lut, keys[0], L, k, beta, levels, workspace=ws)}
                for g in (2, 3, 4):
                    calls["g%d" % g] = (lambda g=g: plan.multibit_bootstrap_batch(out, lwe, lut, keys[g], L, k, beta, levels, g, workspace=ws))
                for fn in calls.values():
                    fn()
                torch.cuda.synchronize()
                ms = {name: [] for name in calls}
                for _ in range(a.reps):
                    for name, fn in calls.items():
                        ms[name].append(round(timed(fn), 3))
                row = {"n": n, "base_log": beta, "levels": levels, "batch": batch, "ms": ms,
                       "best": min(ms, key=lambda name: min(ms[name])), "kernel_ms": {}, "kernel_share": {}, "roofline": {}}
                terms, acc = words(batch * J * n), torch.zeros(batch * O * n, dtype=torch.int64, device="cuda")
                for g in (2, 3, 4):
                    rows = torch.from_numpy(rng.integers(0, 2 * n, size=g * batch, dtype=np.uint32).view(np.int32)).cuda()
                    grp = keys[g][:(J * O << g) * n]
                    plan.multibit_accumulate_batch(acc, terms, rows, grp, J, O, g)
                    t = timed(lambda: [plan.multibit_accumulate_batch(acc, terms, rows, grp, J, O, g) for _ in range(20)]) / 20
                    row["kernel_ms"][g] = round(t, 4)
                    row["kernel_share"][g] = round(t / (min(ms["g%d" % g]) / (L // g)), 3)
                    row["roofline"][g] = round((J + O) * n * 8 * batch / (t * 1e-3) / HBM_BYTES_PER_S, 4)
                with open(a.out, "a") as f:
                    f.write(json.dumps(row) + "\n")
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
