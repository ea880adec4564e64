"""Case generator of the `primeks` family: the prime plans' LWE keyswitch (include/cntt_prime_keyswitch.h).  As tests/random_cases.py,
whose prime search it shares: a case draws from random.Random("primeks/%d" % seed) and from nothing else -- no GPU, no plan, no state of
the library -- and no seed is rejected.  tests/test_gpu_random_prime_keyswitch.py runs seeds 0 .. SEEDS - 1 and asserts, without a GPU,
the corners they reach."""
import random

import random_cases as rc

SEEDS = 32
KS_ROWS = 128                 # prime_keyswitch.hpp: PKS_ROWS
TILE_B, TILE_C = 32, 128      # prime_keyswitch.hpp: 4 * TB batch elements x 64 * TC columns of one workgroup
PLAN_N = {32: 32, 64: 16}     # the smallest transform size of each width: the keyswitch takes only p from the plan
CAP = 10 ** 6                 # integer products of the model: batch * lin * levels * (lout + 1)


def chunk_words(base_log, levels):
    """mask words per chunk of the kernel: min(KS_ROWS, 2^(32 - base_log)) rows, rounded down to whole words"""
    return min(KS_ROWS, 1 << (32 - base_log)) // levels


def _prime(rng, n, lo_bits, bits):
    for _ in range(rc.REDRAWS):
        nbits = rng.randint(lo_bits, bits)
        p = rc._search(n, rng.randrange(1 << (nbits - 1), 1 << nbits))      # the largest prime = 1 mod 2n below the draw
        if p is not None and p.bit_length() == nbits:
            return p
    return rc._search(n, (1 << bits) - 1)        # the largest such prime of the word: always there, and of `bits` bits


def case_primeks(seed):
    rng = random.Random("primeks/%d" % seed)
    bits = (32, 64)[seed % 2]
    n = PLAN_N[bits]
    sel = seed % 8 // 2                          # 0 .. 3 within each width
    wide = sel == 1 and (seed // 8) % 2 == 1     # the widest digits, which need W >= 30
    # the bit length first -- uniformly in 12 .. bits, every other time in the upper half of the word, for the widest digits 30 and up,
    # seeds 14 and 30 the whole 32-bit word (seeds 7 and 23 happen to draw the whole 64-bit word) -- then a prime = 1 mod 2n of that length
    p = _prime(rng, n, bits if seed % 16 == 14 else 30 if wide else bits // 2 + 1 if (seed // 2) % 2 else 12, bits)
    W = p.bit_length()
    # the digits, in an order that keeps base_log <= 31 and base_log * levels <= W
    if wide:                                     # the lazy sums fold after 4 or 2 rows
        base_log = rng.randint(30, min(31, W))
        levels = rng.randint(1, W // base_log)
    elif sel == 1:                               # base_log * levels = W
        base_log = rng.choice([b for b in range(1, min(31, W) + 1) if W % b == 0])
        levels = W // base_log
    elif sel == 3:                               # many levels: few words per chunk
        levels = rng.randint(min(9, W), W)
        base_log = rng.randint(1, W // levels)
    else:
        base_log = rng.randint(1, min(31, W))
        levels = rng.randint(1, min(8, W // base_log))
    kc = chunk_words(base_log, levels)
    lin = rng.randint(0, 3) * kc + rng.randint(0, kc)
    if seed % 17 == 0:                           # seeds 0 and 17: one of each width
        lin = 0
    lout = rng.randint(0, 2 * TILE_C + 49)
    if seed % 17 == 5:                           # seeds 5 and 22
        lout = 0
    batch = rng.randint(1, 2 * TILE_B + 3)
    pad = rng.randint(1, 7) if rng.randrange(2) else 0

    # the cap: the batch shrinks first (down to one element past the tile where it was above it), then lin
    def cost():
        return batch * lin * levels * (lout + 1)
    if cost() > CAP:
        floor = TILE_B + 1 if batch > TILE_B else 1
        batch = max(floor, min(batch, CAP // max(1, lin * levels * (lout + 1))))
    if cost() > CAP:
        lin = CAP // (batch * levels * (lout + 1))
    return {"family": "primeks", "seed": seed, "bits": bits, "p": p, "base_log": base_log, "levels": levels, "lin": lin, "lout": lout,
            "pad": pad, "batch": batch, "data_seed": rng.getrandbits(32)}
