"""Case generator of the `primemultibit` family: the prime plans' multi-bit blind rotation (include/cntt_prime_multibit.h).  As
tests/random_prime_pack_cases.py, whose prime search it shares: a case draws from random.Random("primemultibit/%d" % seed) and from
nothing else -- no GPU, no plan, no state of the library -- and no seed is rejected; coupled parameters are drawn in an order that
satisfies them (the prime first, then base_log, then levels <= W / base_log; L = groups * g).  tests/test_gpu_random_prime_multibit.py
runs seeds 0 .. SEEDS - 1; tests/test_random_prime_multibit_cases.py asserts, without a GPU, the corners they reach."""
import random

import random_prime_keyswitch_cases as pk          # _prime: the shared prime search of random_cases

SEEDS = 32
MIN_N = {32: 32, 64: 16}      # the smallest transform size of each width
SIZES = [16, 32, 64]
CAP = 100000                  # row operations of the ring model: batch * groups * 2^g * J * (k + 1) * n


def case_primemultibit(seed):
    rng = random.Random("primemultibit/%d" % seed)
    bits = (32, 64)[seed % 2]
    j = seed // 2                                # 0 .. 15 within each width
    g = j % 4 + 1                                # every grouping, four times per width
    sel = j // 4                                 # the digit class, once with every grouping
    sizes = [n for n in SIZES if n >= MIN_N[bits]]
    n = sizes[0] if j % 8 == 6 else rng.choice(sizes)
    lo_bits = max(n.bit_length() + 2, 12)
    if j % 8 == 3:                               # the reference's strict range: one bit below the word
        p = pk._prime(rng, n, bits - 1, bits - 1)
    else:
        p = pk._prime(rng, n, bits if j == 7 else max(lo_bits, bits // 2 + 1) if j % 2 else lo_bits, bits)
    W = p.bit_length()
    if sel == 1:                                 # base_log * levels = W
        base_log = rng.choice([b for b in range(1, W + 1) if W % b == 0 and W // b <= 6])
        levels = W // base_log
    elif sel == 3:                               # one wide level
        base_log, levels = rng.randint(max(1, W // 2), W), 1
    else:
        base_log = rng.randint(1, W)
        levels = rng.randint(1, min(4, W // base_log))
    k = 4 if j % 8 == 2 else rng.randint(1, 2)   # nout = k + 1 = 5: past the fused chains' four outputs
    groups, batch = rng.randint(1, 2), rng.randint(1, 3)

    # the cap shrinks the case: the batch first, then the groups, then the levels (base_log * levels <= W stays true)
    def cost():
        return batch * groups * (1 << g) * (k + 1) * levels * (k + 1) * n
    if cost() > CAP:
        batch = 1
    if cost() > CAP:
        groups = 1
    while cost() > CAP and levels > 1:
        levels -= 1
    return {"family": "primemultibit", "seed": seed, "bits": bits, "p": p, "n": n, "k": k, "g": g, "groups": groups, "lwe_dim": groups * g,
            "base_log": base_log, "levels": levels, "batch": batch, "per_element": bool(rng.randrange(2)), "workspace": bool(rng.randrange(2)),
            "data_seed": rng.getrandbits(32)}


def rot_of(case):
    """rot_t of the case, (L + 1) * batch exponents below 2n: uniform, except that element 0 of every odd seed's first two mask rows is
    2n - 1, so that with g >= 2 a subset sum wraps 2n by construction and not by luck"""
    rng = random.Random("primemultibit/rot/%d" % case["data_seed"])
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
