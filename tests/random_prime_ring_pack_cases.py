"""Case generator of the `primeringpack` family: the prime plans' ring packing (include/cntt_prime_ring_pack.h).  As
tests/random_prime_automorphism_cases.py, whose prime search it shares: a case draws from random.Random("primeringpack/%d" % seed) and
from nothing else -- no GPU, no plan, no state of the library -- and no seed is rejected.  tests/test_gpu_random_prime_ring_pack.py
runs seeds 0 .. SEEDS - 1; tests/test_random_prime_ring_pack_cases.py asserts, without a GPU, the corners they reach."""
import random

import random_prime_keyswitch_cases as pk          # _prime: the shared prime search of random_cases

SEEDS = 32
MIN_N = {32: 32, 64: 16}      # the smallest transform size of each width
SIZES = [16, 32, 64, 128, 256]
CAP = 3 * 10 ** 6             # integer products of the model of one tree node: batch * k * levels * (k + 1) * n * n


def case_primeringpack(seed):
    rng = random.Random("primeringpack/%d" % seed)
    bits = (32, 64)[seed % 2]
    j = seed // 2                                # 0 .. 15 within each width
    sel = j % 4                                  # the digit class
    sizes = [n for n in SIZES if n >= MIN_N[bits]]
    n = sizes[-1] if j % 8 == 5 else sizes[0] if j % 8 == 6 else rng.choice(sizes)
    logn = n.bit_length() - 1
    lo_bits = 33 if bits == 64 else max(n.bit_length() + 2, 12)   # a 64-bit case has a modulus only a 64-bit plan takes
    p = pk._prime(rng, n, bits if j == 7 else max(lo_bits, bits // 2 + 1) if j % 2 else lo_bits, bits)
    W = p.bit_length()
    if sel == 1:                                 # base_log * levels = W: no rounding
        base_log = rng.choice([b for b in range(1, W + 1) if W % b == 0 and W // b <= 8])
        levels = W // base_log
    elif sel == 3:                               # many levels
        levels = rng.randint(min(5, W), min(W, 9))
        base_log = rng.randint(1, W // levels)
    else:
        base_log = rng.randint(1, W)
        levels = rng.randint(1, min(4, W // base_log))
    k = 0 if j == 8 else 4 if j % 8 == 2 else rng.randint(1, 3)
    m = 1 if j % 8 == 1 else n if j % 8 == 3 else 2 if j == 4 else 1 << rng.randint(0, logn)
    shift = (0, n - 1, n, 2 * n - 1)[j // 4 % 4] if j % 4 == 0 else rng.randrange(2 * n)
    t = 2 * rng.randrange(n) + 1
    batch = rng.randint(1, 3)

    # the cap shrinks the case: the batch first, then the dimension
    def cost():
        return batch * k * levels * (k + 1) * n * n
    if cost() > CAP:
        batch = 1
    while cost() > CAP and k > 1:
        k -= 1
    return {"family": "primeringpack", "seed": seed, "bits": bits, "p": p, "n": n, "k": k, "lwe_count": m, "shift": shift, "t": t,
            "base_log": base_log, "levels": levels, "batch": batch, "workspace": bool(rng.randrange(2)), "data_seed": rng.getrandbits(32)}
