"""Seeded case generators for the random sweep over the external-product, gadget, bootstrap and keyswitch calls
(tests/test_gpu_random_fhe.py, tools/soak_random.py; the corners the first SEEDS seeds must reach: tests/test_random_cases.py).

    case(family, seed) -> dict

draws from random.Random("%s/%d" % (family, seed)) and from nothing else: no GPU, no plan, no state of the library.  Every case is
valid by construction -- coupled parameters are drawn in an order that satisfies the coupling, every redraw loop is bounded and ends in
a fallback that is valid, and a shape whose CPU model would cost too much shrinks (lin, batch) instead of being rejected -- so a
(family, seed) never yields "no case".  A few parameters are stratified by the seed itself (kind = seed mod 10 and the like), the way
tests/test_gpu_random.py does it, so that a short prefix of the seeds reaches every kind, size and class.

The only thing read from outside is the CPU oracle's prime search, for the primepbs family."""
import random

SEEDS = 32            # seeds per family the test suite runs; tools/soak_random.py continues from here
FAMILIES = ("ext", "gadget", "nativepbs", "keyswitch", "pack", "primepbs")

KINDS = ["native32_plan32", "native64_plan32", "native128_plan32", "native_binary32_plan32", "native_binary64_plan32",
         "native_binary128_plan32", "native32_plan52", "native64_plan52", "native_binary32_plan52", "native_binary64_plan52"]
FUSED_KINDS = ["native32_plan32", "native64_plan32", "native_binary32_plan32", "native_binary64_plan32"]     # the fused gadget kernel
FUSED_N = [32, 64, 128, 256, 512, 1024, 2048, 4096]
BIG_N = [8192, 16384]
WORD_KIND = {32: "native32_plan32", 64: "native64_plan32", 128: "native128_plan32"}
MODES = ["plain", "rotate", "cmux"]
PACK_TERMS = 64       # CNTT_PACK_TERMS (cntt_pack.h)
KS_ROWS = 128         # digit rows per chunk of the keyswitch kernel (native_keyswitch.hpp)
KS_TILE_B = {32: 64, 64: 64, 128: 32}
PACK_TI = {32: 32, 64: 32, 128: 16}

# cntt_native_max_terms() restated on Python ints (csrc/host_native.hip, native_max_terms_of; tests/test_random_cases.py compares the
# two): the primes of the plans and, per kind, (number of primes, 52-bit primes, prime indices of the top mixed-radix group)
PRIMES32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801, 1068433409, 1068564481, 1069219841, 1071513601, 1073479681]
PRIMES52 = [1125899881086977, 1125899885412353, 1125899886395393, 1125899899174913, 1125899902124033, 1125899903107073]
KIND_INFO = {"native32_plan32": (3, False, (2,)), "native64_plan32": (5, False, (3, 4)), "native128_plan32": (10, False, (8, 9)),
             "native_binary32_plan32": (2, False, (1,)), "native_binary64_plan32": (3, False, (2,)),
             "native_binary128_plan32": (5, False, (3, 4)), "native32_plan52": (2, True, (1,)), "native64_plan52": (3, True, (2,)),
             "native_binary32_plan52": (1, True, (0,)), "native_binary64_plan52": (2, True, (1,))}
ACC_FRAC_BITS = 27

# cost caps of the CPU models, in big-integer multiply-adds (keyswitch, pack at w = 128) or wrapping numpy ones (pack at w = 32 / 64)
KEYSWITCH_CAP = 2 * 10 ** 6
PACK_CAP = {32: 10 ** 8, 64: 10 ** 8, 128: 8 * 10 ** 6}
SCHOOLBOOK_MAX_N = 64
# levels: most cases stay at a handful (what bootstraps use); one in four of the gadget, bootstrap and packing cases may take many narrow
# digits: up to WIDE_LEVELS, the gadget family as many as keep its key within WIDE_KEY_WORDS coefficients (128 at small sizes)
WIDE_LEVELS = 32
WIDE_KEY_WORDS = 1 << 19


def wbits(kind):
    return 128 if "128" in kind else 64 if "64" in kind else 32


def is_binary(kind):
    return "binary" in kind


def max_terms(kind, n):
    nprimes, is52, top = KIND_INFO[kind]
    primes = (PRIMES52 if is52 else PRIMES32)[:nprimes]
    M = Mpre = 1
    for i, q in enumerate(primes):
        M *= q
        if i not in top:
            Mpre *= q
    lim = min((M - Mpre) >> 1, ((M + Mpre) >> 1) - 1)
    if not is52:
        lim = min(lim, (M - 1) >> 1, (M * ((1 << ACC_FRAC_BITS) - 3 * nprimes)) >> (ACC_FRAC_BITS + 1))
    A = (1 << wbits(kind)) - 1
    return max(1, min(lim // (n * (A if is_binary(kind) else A * A)), (1 << 63) - 1))


def _rng(family, seed):
    return random.Random("%s/%d" % (family, seed))


def special_words(rng, w, count):
    """word values: three in four uniform, the rest 0, 1, 2^w - 1 and 2^(w-1)"""
    edge = [0, 1, (1 << w) - 1, 1 << (w - 1)]
    return [edge[rng.randrange(4)] if rng.randrange(4) == 0 else rng.getrandbits(w) for _ in range(count)]


def _digit_pair(rng, w, max_base_log, max_levels, full):
    """(base_log, levels) with base_log * levels <= w, base_log <= max_base_log, levels <= max_levels (>= 1); full: base_log * levels
    = w where such a pair exists under the two caps.  levels first, then base_log from what it leaves: no redraw."""
    max_levels = max(1, min(max_levels, w))
    if full:
        pairs = [(b, w // b) for b in range(1, min(max_base_log, w) + 1) if w % b == 0 and w // b <= max_levels]
        if pairs:
            return pairs[rng.randrange(len(pairs))]
    levels = rng.randint(1, max_levels)                      # max_levels <= w: w // levels >= 1
    base_log = rng.randint(1, min(max_base_log, w // levels))
    return base_log, levels


def rot_values(rng, n, batch):
    fixed = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    return [fixed[rng.randrange(6)] if rng.randrange(3) == 0 else rng.randrange(2 * n) for _ in range(batch)]


def _ragged(rng, n):
    """a batch around the 4096 / n elements one workgroup of the fused kernels holds"""
    full = max(1, 4096 // n)
    return max(1, full + rng.randint(-2, 3)) if rng.randrange(3) else rng.randint(1, 2 * full + 1)


# -- ext: cntt_native_external_product_batch ---------------------------------------------------------------------------------------------
def case_ext(seed):
    rng = _rng("ext", seed)
    kind = KINDS[seed % 10]
    big = seed % 4 == 3
    n = BIG_N[(seed // 4) % 2] if big else FUSED_N[((seed // 4) * 3 + seed % 4) % 8]
    nterms = min(rng.randint(1, 9), max_terms(kind, n))
    nout = 5 if seed % 8 == 5 else rng.randint(1, 5)
    batch = 1 if big else _ragged(rng, n)
    return {"family": "ext", "seed": seed, "kind": kind, "n": n, "nterms": nterms, "nout": nout, "batch": batch,
            "accumulate": bool(rng.randrange(2)), "switch": rng.randrange(2), "data_seed": rng.getrandbits(32)}


# -- gadget: gadget_decompose_batch and external_product_decomposed_batch ----------------------------------------------------------------
def case_gadget(seed):
    rng = _rng("gadget", seed)
    kind = KINDS[seed % 10]
    big = seed % 8 == 7
    n = BIG_N[(seed // 8) % 2] if big else FUSED_N[(seed // 2) % 8]
    w = wbits(kind)
    fused = kind in FUSED_KINDS and n <= 4096
    npolys = min(rng.randint(1, 4), max_terms(kind, n))
    nout = rng.randint(1, 4)
    # levels: up to 8; one case in four as many as the word and max_terms allow while the key stays within WIDE_KEY_WORDS coefficients
    cap = max(8, WIDE_KEY_WORDS // (npolys * nout * n)) if rng.randrange(4) == 0 else 8
    base_log, levels = _digit_pair(rng, w, 31 if fused else w, min(max_terms(kind, n) // npolys, cap), full=rng.randrange(4) == 0 or seed % 4 == 1)
    batch = 1 if big else min(_ragged(rng, n), max(1, 16384 // (npolys * n)))          # the model walks every coefficient
    mode = MODES[rng.randrange(3)]
    return {"family": "gadget", "seed": seed, "kind": kind, "n": n, "npolys": npolys, "base_log": base_log, "levels": levels,
            "nout": nout, "mode": mode, "rot": rot_values(rng, n, batch), "batch": batch, "fused": fused,
            "addend": [None, "out", "third"][rng.randrange(3)], "data_seed": rng.getrandbits(32)}


# -- nativepbs: modulus switch, sample extraction, blind rotation, bootstrap on the native plans -------------------------------------------
def case_nativepbs(seed):
    rng = _rng("nativepbs", seed)
    w = (32, 64, 128)[seed % 3]
    n = (32, 64, 256, 1024)[(seed // 3) % 4]
    kind = WORD_KIND[w]
    k = rng.randint(1, 3)
    cap = WIDE_LEVELS if rng.randrange(4) == 0 else 4          # levels: up to 4; one case in four up to WIDE_LEVELS
    base_log, levels = _digit_pair(rng, w, w, min(max_terms(kind, n) // (k + 1), cap), full=rng.randrange(4) == 0)
    L = rng.randint(0, 6)
    batch = 33 if seed % 8 == 2 else rng.randint(1, 40)
    return {"family": "nativepbs", "seed": seed, "w": w, "kind": kind, "n": n, "k": k, "L": L, "base_log": base_log, "levels": levels,
            "batch": batch, "per_element": bool(rng.randrange(2)), "workspace": bool(rng.randrange(2)), "index": rng.randrange(n),
            "data_seed": rng.getrandbits(32)}


# -- keyswitch: keyswitch_batch -------------------------------------------------------------------------------------------------------------
def case_keyswitch(seed):
    rng = _rng("keyswitch", seed)
    w = (32, 64, 128)[seed % 3]
    tile = KS_TILE_B[w]
    sel = seed % 12 // 3                      # 0 .. 3 within each width
    if sel == 3 or (w == 128 and sel == 2):    # one in four: levels > 16; w = 128 also reaches levels >= 64
        lo = 64 if (w == 128 and sel == 2) else 17
        levels = rng.randint(lo, w)
        base_log = rng.randint(1, w // levels)
    elif sel == 1:                             # base_log * levels = w, or base_log = 31 (alternating)
        if (seed // 12) % 2:
            base_log, levels = 31, rng.randint(1, w // 31)
        else:
            base_log, levels = _digit_pair(rng, w, 31, 16, full=True)
    else:
        base_log, levels = _digit_pair(rng, w, 31, 16, full=False)
    kc = KS_ROWS // levels
    lin = rng.randint(0, 3) * kc + rng.randint(0, kc)
    if seed % 12 == 0:
        lin = 0
    lout = rng.randint(0, 2 * 128 + 49)
    if seed % 12 == 6:
        lout = 0
    batch = rng.randint(1, 2 * tile + 3)
    pad = rng.randint(0, 7) if rng.randrange(2) else 0
    # the cap: batch first (down to one element past the tile where it was above it), then lin
    def cost():
        return batch * lin * levels * (lout + 1)
    if cost() > KEYSWITCH_CAP:
        floor = tile + 1 if batch > tile else 1
        batch = max(floor, min(batch, KEYSWITCH_CAP // max(1, lin * levels * (lout + 1))))
    if cost() > KEYSWITCH_CAP:
        lin = KEYSWITCH_CAP // (batch * levels * (lout + 1))
    return {"family": "keyswitch", "seed": seed, "w": w, "base_log": base_log, "levels": levels, "lin": lin, "lout": lout, "pad": pad,
            "batch": batch, "data_seed": rng.getrandbits(32)}


# -- pack: pack_keyswitch_batch -------------------------------------------------------------------------------------------------------------
def case_pack(seed):
    rng = _rng("pack", seed)
    w = (32, 64, 128)[seed % 3]
    kind = WORD_KIND[w]
    sel = seed % 12 // 3
    n = 32 << rng.randrange(6)                             # 32 .. 1024
    k = rng.randint(1, 2)
    m = n if sel == 0 else rng.randint(1, min(n, 63)) if sel == 1 else rng.randint(1, n)
    mt = max_terms(kind, n)
    if sel == 2:                                            # a digit wider than 32 bits
        levels = rng.randint(1, min(mt, w // 32 - 1)) if w > 32 else 1
        base_log = rng.randint(32, w // levels)
    else:
        cap = WIDE_LEVELS if rng.randrange(4) == 0 else 8  # levels: up to 8; one case in four up to WIDE_LEVELS
        base_log, levels = _digit_pair(rng, w, w, min(mt, cap), full=rng.randrange(4) == 0)
    C = max(1, min(mt, PACK_TERMS) // levels)
    ti = PACK_TI[w]
    pick = rng.randrange(4) if sel != 3 else 2
    lin = (rng.randint(0, 3), ti + rng.randint(-1, 2), C + rng.randint(1, 3), 2 * C + rng.randint(-1, 3))[pick]
    batch = rng.randint(1, 3)
    def cost():
        return batch * m * lin * levels * (k + 1) * n
    # the cap: the batch first, then m where the case does not pin it (down to one ciphertext), then lin
    if cost() > PACK_CAP[w]:
        batch = 1
    if cost() > PACK_CAP[w] and sel != 0:
        m = max(1, min(m, PACK_CAP[w] // (lin * levels * (k + 1) * n)))
    if cost() > PACK_CAP[w]:
        lin = PACK_CAP[w] // (m * levels * (k + 1) * n)
    return {"family": "pack", "seed": seed, "w": w, "kind": kind, "n": n, "k": k, "m": m, "lin": lin, "base_log": base_log,
            "levels": levels, "batch": batch, "workspace": bool(rng.randrange(2)), "C": C, "data_seed": rng.getrandbits(32)}


# -- primepbs: the six cntt_prime{32,64}_* bootstrap calls ---------------------------------------------------------------------------------
# (name, word bits, lowest value, one past the highest, a prime of the class = 1 mod 2048 as the fallback)
PRIME_CLASSES = [("lazy", 64, 1 << 51, 1 << 62, 4611686018427322369),
                 ("above_pow2", 64, 1 << 51, 1 << 62, 2305843009214414849),
                 ("strict", 64, 1 << 62, 1 << 63, 9223372036853661697),
                 ("montgomery", 64, 1 << 63, (1 << 64) - (1 << 32), 9224497936763846657),
                 ("solinas", 64, (1 << 64) - (1 << 32), 1 << 64, 18446744069414584321),
                 ("fp50", 64, 1 << 40, 1 << 50, 1125899904679937),
                 ("fp51", 64, 1 << 50, 1 << 51, 2251799813554177),
                 ("lazy", 32, 1 << 20, 1 << 30, 1062862849),
                 ("above_pow2", 32, 1 << 20, 1 << 30, 536903681),
                 ("strict", 32, 1 << 30, 1 << 31, 2147352577),
                 ("top", 32, 1 << 31, 1 << 32, 4293918721)]
REDRAWS = 8


def above_pow2(p):
    """just above a power of two: within 1 / 64 of it"""
    top = 1 << (p.bit_length() - 1)
    return p - top <= top >> 6


def _search(n, hi):
    from oracle import pyoracle
    p = pyoracle.largest_prime_in_arithmetic_progression64(2 * n, 1, 0, hi)
    return p if p is not None and p > 2 * n else None


def _class_prime(rng, n, cls):
    name, bits, lo, end, fallback = cls
    for _ in range(REDRAWS):
        if name == "above_pow2":
            top = 1 << (rng.randint(lo.bit_length(), end.bit_length() - 1) - 1)
            hi = top + rng.randint(1, max(4 * n, top >> 6))
            p = _search(n, hi)
            if p is not None and p > top and above_pow2(p):
                return p
        else:
            p = _search(n, rng.randrange(lo, end))
            if p is not None and lo <= p < end:
                return p
    return fallback


def _uniform_prime(rng, n, bits):
    lo_bits = max(n.bit_length() + 2, 12)
    for _ in range(REDRAWS):
        nbits = rng.randint(lo_bits, bits)          # the bit length first, uniformly; then a prime of that length
        p = _search(n, rng.randrange(1 << (nbits - 1), 1 << nbits))
        if p is not None and p.bit_length() == nbits:
            return p
    return _search(n, (1 << bits) - 1)              # the largest prime = 1 mod 2n of the word: always there


def case_primepbs(seed):
    rng = _rng("primepbs", seed)
    cls = PRIME_CLASSES[(seed // 3) % len(PRIME_CLASSES)] if seed % 3 == 0 else None
    bits = cls[1] if cls else (64, 32)[rng.randrange(2)]
    n = ({64: 16, 32: 32}[bits], 64, 1024)[rng.randrange(3)]
    p = _class_prime(rng, n, cls) if cls else _uniform_prime(rng, n, bits)
    W = p.bit_length()
    if seed % 8 == 0:
        base_log, levels = W, 1
    elif seed % 8 == 4:
        pairs = [(b, W // b) for b in range(1, W + 1) if W % b == 0 and 2 <= W // b <= 8]
        base_log, levels = pairs[(seed // 8) % len(pairs)] if pairs else (W, 1)          # W prime: only (W, 1) and (1, W)
    else:
        cap = WIDE_LEVELS if rng.randrange(4) == 0 else 8          # levels: up to 8; one case in four up to WIDE_LEVELS
        base_log, levels = _digit_pair(rng, W, W, cap, full=False)
    return {"family": "primepbs", "seed": seed, "bits": bits, "p": p, "W": W, "cls": cls[0] if cls else None, "n": n, "k": rng.randint(1, 4),
            "L": rng.randint(0, 5), "base_log": base_log, "levels": levels, "batch": 33 if seed % 8 == 3 else rng.randint(1, 40),
            "per_element": bool(rng.randrange(2)), "workspace": bool(rng.randrange(2)), "index": rng.randrange(n),
            "mode": MODES[rng.randrange(3)], "npolys": rng.randint(1, 3), "data_seed": rng.getrandbits(32)}


_CASES = {"ext": case_ext, "gadget": case_gadget, "nativepbs": case_nativepbs, "keyswitch": case_keyswitch, "pack": case_pack,
          "primepbs": case_primepbs}


def case(family, seed):
    return _CASES[family](seed)


# -- "the big-integer model applies", decided per prime on the CPU --------------------------------------------------------------------------
PROBE_PRODUCTS = 1 << 16


def model_applies(oracle, p, bits):
    """True when the oracle's fwd / mul_accumulate / inv composition under the bootstrap's key convention (key = n^-1 fwd(key)) equals
    the exact negacyclic product mod p on a fixed probe: the smallest plan of the word type (n = 16 / 32, so every prime a plan accepts
    can be probed), PROBE_PRODUCTS / n + 8 terms into one accumulator -- some 65 700 pointwise products.  The first 8 left operands are
    dense (all p - 1, then the oracle's uniform words), the others monomials c X^i with uniform c (their transforms are as good as
    uniform, and the exact product is a signed shift); the right operands are uniform, two of them all p - 1 and all (p + 1) / 2.  The reference's Barrett product wraps for some primes above 2^B / 3, up
    to 7e-4 of the products: the probe sees such a prime with all but negligible probability, and a prime it passes has a wrap rate low
    enough for the sweep's few thousand products per case.  Primes the probe fails are compared with the per-iteration public calls."""
    import numpy as np
    n, dense = 16 if bits == 64 else 32, 8
    monomials = PROBE_PRODUCTS // n
    terms = monomials + dense
    if (p - 1) % (2 * n):
        return False
    plan = oracle.Plan.try_new(n, p, bits)
    if plan is None:
        return False
    dt = np.uint64 if bits == 64 else np.uint32
    a = np.zeros(terms * n, dtype=dt)
    a[:dense * n] = oracle.fill_uniform(dense * n, p, 1, bits)
    a[:2 * n] = p - 1
    coef = [int(v) for v in oracle.fill_uniform(monomials, p, 3, bits)]
    for j, cj in enumerate(coef):
        a[(dense + j) * n + j % n] = cj
    b = oracle.fill_uniform(terms * n, p, 2, bits).astype(dt)
    b[:n] = p - 1
    b[2 * n:3 * n] = (p + 1) // 2
    bi = [int(v) for v in b]
    want = [0] * n
    for j in range(terms):
        y = bi[j * n:(j + 1) * n]
        if j < dense:
            x = [int(v) for v in a[j * n:(j + 1) * n]]
            for i in range(n):
                for l in range(n):
                    want[(i + l) % n] += x[i] * y[l] if i + l < n else -x[i] * y[l]
        else:
            i, cj = (j - dense) % n, coef[j - dense]
            for l in range(n):
                want[(i + l) % n] += cj * y[l] if i + l < n else -cj * y[l]
    acc = np.zeros(n, dtype=dt)
    for j in range(terms):
        x, y = a[j * n:(j + 1) * n].copy(), b[j * n:(j + 1) * n].copy()
        plan.fwd(x)
        plan.fwd(y)
        plan.normalize(y)
        plan.mul_accumulate(acc, x, y)
    plan.inv(acc)
    return [int(v) for v in acc] == [v % p for v in want]
