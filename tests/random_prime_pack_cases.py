"""Case generator of the `primepack` family: the prime plans' LWE-to-GLWE packing keyswitch (include/cntt_prime_pack.h).  As
tests/random_prime_keyswitch_cases.py, whose prime search it shares: a case draws from random.Random("primepack/%d" % seed) and from
nothing else -- no GPU, no plan, no state of the library -- and no seed is rejected.  tests/test_gpu_random_prime_pack.py runs seeds
0 .. SEEDS - 1; tests/test_random_prime_pack_cases.py asserts, without a GPU, the corners they reach."""
import random

import random_prime_keyswitch_cases as pk          # _prime: the shared prime search of random_cases

SEEDS = 32
PACK_TERMS = 64               # CNTT_PRIME_PACK_TERMS (cntt_prime_pack.h)
TT, TI = 64, 32               # prime_pack.hpp: ciphertexts x mask words of one workgroup's tile
MIN_N = {32: 32, 64: 16}      # the smallest transform size of each width
SIZES = [16, 32, 64, 128, 256]
CAP = 4 * 10 ** 6             # integer products of the model: batch * m * lin * levels * (k + 1) * n


def chunk(levels):
    """C of the header, before the cap at Lin"""
    return max(1, PACK_TERMS // levels)


def case_primepack(seed):
    rng = random.Random("primepack/%d" % seed)
    bits = (32, 64)[seed % 2]
    j = seed // 2                                # 0 .. 15 within each width
    sel = j % 4                                  # the digit class
    wide = sel == 1 and (j // 4) % 2 == 1        # wide digits: 30 bits and up, on 64-bit words above 31 (full words: no cap as in the keyswitch)
    mpick = (j + j // 5) % 5                     # 1 / inside / TT - 1 / TT + 1 / n
    sizes = [n for n in SIZES if n >= MIN_N[bits]]
    n = sizes[-1] if j % 8 == 5 else sizes[0] if j % 8 == 6 else rng.choice(sizes)
    if mpick in (2, 3):                          # the tile edge along t needs two tiles
        n = max(n, 2 * TT)
    lo_bits = max(n.bit_length() + 2, 12)
    p = pk._prime(rng, n, bits if j == 7 else max(lo_bits, 32 if bits == 64 else 30) if wide else max(lo_bits, bits // 2 + 1) if j % 2 else lo_bits,
                  bits)
    W = p.bit_length()
    if wide:
        base_log = rng.randint(32 if bits == 64 else 30, W if bits == 64 else min(31, W))
        levels = rng.randint(1, W // base_log)
    elif sel == 1:                               # base_log * levels = W
        base_log = rng.choice([b for b in range(1, W + 1) if W % b == 0])
        levels = W // base_log
    elif sel == 3:                               # many levels: few words per chunk
        levels = rng.randint(min(9, W), W)
        base_log = rng.randint(1, W // levels)
    else:
        base_log = rng.randint(1, W)
        levels = rng.randint(1, min(8, W // base_log))
    k = 5 if j % 8 == 2 else rng.randint(1, 4)
    m = (1, rng.randint(2, n - 1), TT - 1, TT + 1, n)[mpick]
    C = chunk(levels)
    lin = (rng.randint(1, 3), TI + rng.randint(-1, 2), C + rng.randint(1, 3), 2 * C + rng.randint(-1, 3))[rng.randrange(4)]
    if j == 8:                                   # seeds 16 and 17: one of each width
        lin = 0
    batch = rng.randint(1, 3)

    # the cap shrinks the case: the batch first, then lin (down to one mask word), then m
    def cost():
        return batch * m * lin * levels * (k + 1) * n
    if cost() > CAP:
        batch = 1
    if cost() > CAP:
        lin = max(1, CAP // (m * levels * (k + 1) * n))
    if cost() > CAP:
        m = max(1, CAP // (lin * levels * (k + 1) * n))
    return {"family": "primepack", "seed": seed, "bits": bits, "p": p, "n": n, "k": k, "m": m, "lin": lin, "base_log": base_log,
            "levels": levels, "batch": batch, "workspace": bool(rng.randrange(2)), "data_seed": rng.getrandbits(32)}
