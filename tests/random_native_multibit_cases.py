"""Case generator of the `nativemultibit` family: the native plans' multi-bit blind rotation (include/cntt_multibit.h).  As
tests/random_prime_multibit_cases.py: a case draws from random.Random("nativemultibit/%d" % seed) and from nothing else -- no GPU, no
plan, no state of the library -- and no seed is rejected; coupled parameters are drawn in an order that satisfies them (the kind first,
then base_log, then levels <= w / base_log; L = groups * g).  tests/test_gpu_random_native_multibit.py runs seeds 0 .. SEEDS - 1;
tests/test_random_native_multibit_cases.py asserts, without a GPU, the corners they reach."""
import random

SEEDS = 32
KINDS = ["native32_plan32", "native64_plan32", "native128_plan32", "native_binary32_plan32", "native_binary64_plan32",
         "native_binary128_plan32"]
WBITS = {"native32_plan32": 32, "native64_plan32": 64, "native128_plan32": 128, "native_binary32_plan32": 32,
         "native_binary64_plan32": 64, "native_binary128_plan32": 128}
SIZES = [32, 64]
LAZY = 4                      # the kernel's chunk: J on both sides of it and ragged against it
CAP = 60000                   # row operations of the ring model: batch * groups * 2^g * J * (k + 1) * n


def case_nativemultibit(seed):
    rng = random.Random("nativemultibit/%d" % seed)
    kind = KINDS[seed % 6]
    j = seed // 6                                # 0 .. 5 within each kind (the last two kinds: 0 .. 4)
    g = (seed + j) % 4 + 1                       # every grouping on every kind
    w = WBITS[kind]
    n = SIZES[0] if j == 0 else rng.choice(SIZES)
    sel = j % 4                                  # the digit class
    if sel == 1:                                 # base_log * levels = w: no rounding
        levels = rng.choice([2, 4])
        base_log = w // levels
    elif sel == 3:                               # one wide level
        base_log, levels = rng.randint(w // 2, w), 1
    else:
        base_log = rng.randint(1, w // 3)
        levels = rng.randint(2, 3)
    k = 2 if j % 3 == 2 else 1                   # nout = 3 and J = 3 * levels: ragged against the chunk of four
    groups, batch = rng.randint(1, 2), rng.randint(1, 3)

    def cost():
        return batch * groups * (1 << g) * (k + 1) * levels * (k + 1) * n
    if cost() > CAP:
        batch = 1
    if cost() > CAP:
        groups = 1
    return {"family": "nativemultibit", "seed": seed, "kind": kind, "w": w, "n": n, "k": k, "g": g, "groups": groups,
            "lwe_dim": groups * g, "base_log": base_log, "levels": levels, "batch": batch, "per_element": bool(rng.randrange(2)),
            "workspace": bool(rng.randrange(2)), "data_seed": rng.getrandbits(32)}


def rot_of(case):
    """rot_t of the case, (L + 1) * batch exponents below 2n: uniform, except that with g >= 2 element 0 of the first two mask rows is
    2n - 1, so that a subset sum wraps 2n by construction and not by luck"""
    rng = random.Random("nativemultibit/rot/%d" % case["data_seed"])
    n, L, batch = case["n"], case["lwe_dim"], case["batch"]
    rot = [rng.randrange(2 * n) for _ in range((L + 1) * batch)]
    if case["g"] >= 2:
        rot[0] = rot[batch] = 2 * n - 1
    return rot


def wraps(case):
    """True when some group of some element has exponents whose plain sum reaches 2n"""
    n, g, batch = case["n"], case["g"], case["batch"]
    rot = rot_of(case)
    return any(sum(rot[(r * g + i) * batch + b] for i in range(g)) >= 2 * n for r in range(case["groups"]) for b in range(batch))
