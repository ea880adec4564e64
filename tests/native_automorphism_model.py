"""The plain-int model of include/cntt_automorphism.h on lists of Python ints mod 2^w: the automorphism sigma_t in gather form and as the
scatter that defines it, the slot permutation of a residue plane, the Galois keyswitch and the trace with the digits of cntt_gadget.h
(restated here, not imported from the code under test), automorphism keys with or without noise, the phase, and the header's workspace
formulas and grid rule.  tests/test_native_automorphism_model.py checks these against each other, against the CPU oracle's transforms and
against the header's phase statements.  No GPU needed; not a test module."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_automorphism.h")
LDS_BYTES = 64 << 10                  # native_automorphism.hpp: the largest polynomial the kernels stage through LDS


def up(x):
    return (x + 255) // 256 * 256


def autoks_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word)


def trace_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word) + up(batch * (k + 1) * n * word)


def grid(polys, logn, word):
    """the rule cntt_native_automorphism_grid exports: one workgroup per polynomial up to 8 per CU of a 256-CU part, fewer where the
    staged polynomial (up to 64 KiB) limits residency at 160 KiB of LDS per CU"""
    size = word << logn
    per_cu = min(8, max(1, (160 << 10) // size)) if 0 < size <= LDS_BYTES else 8
    return max(1, min(polys, per_cu * 256))


def trace_exponents(n, steps):
    return [(n >> r) + 1 for r in range(steps)]


# -- the ring -------------------------------------------------------------------------------------------------------------------------
def digits(x, w, beta, ell):
    """the signed digits of cntt_gadget.h, the sequential rule: round to a multiple of 2^s (ties up), then base-B digits in [-B/2, B/2)
    with carries, d_1 (most significant) first"""
    s = w - beta * ell
    state = x if s == 0 else ((x + (1 << (s - 1))) % (1 << w)) >> s
    B, out = 1 << beta, []
    for _ in range(ell):
        d = state % B
        state >>= beta
        if d >= B // 2:
            d -= B
            state += 1
        out.append(d)
    return out[::-1]


def negacyclic(a, b, w):
    """the schoolbook product in Z/2^w[X]/(X^n + 1)"""
    n, M = len(a), 1 << w
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < n:
                    out[i + j] += x * y
                else:
                    out[i + j - n] -= x * y
    return [v % M for v in out]


# -- the automorphism -----------------------------------------------------------------------------------------------------------------
def autom_scatter(f, t, w):
    """the definition: X^i -> (-1)^floor(i t / n) X^(i t mod n)"""
    n, M = len(f), 1 << w
    out = [0] * n
    for i, x in enumerate(f):
        e = i * t % (2 * n)
        out[e % n] = (-x) % M if e >= n else x % M
    return out


def autom_gather(f, t, w):
    """the header's gather form: out[j] = +-f[j tinv mod 2n]"""
    n, M = len(f), 1 << w
    tinv = pow(t, -1, 2 * n)
    out = []
    for j in range(n):
        u = j * tinv % (2 * n)
        out.append((-f[u % n]) % M if u >= n else f[u % n] % M)
    return out


def autom_gather_np(f, t):
    """autom_gather on a numpy array of u32 / u64 words (any leading shape, polynomials along the last axis)"""
    n = f.shape[-1]
    u = np.arange(n, dtype=np.int64) * pow(t, -1, 2 * n) % (2 * n)
    x = f[..., u % n]
    with np.errstate(over="ignore"):
        return np.where(u >= n, (f.dtype.type(0) - x).astype(f.dtype), x)


def bitrev(x, logn):
    return int(format(x, "0%db" % logn)[::-1], 2) if logn else 0


def ntt_permutation(t, n):
    """src[c] = c' with 2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n, as an index array: out_plane = in_plane[src]"""
    logn = n.bit_length() - 1
    c = np.arange(n, dtype=np.int64)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(logn):
        rev |= ((c >> b) & 1) << (logn - 1 - b)
    e = t * (2 * rev + 1) % (2 * n)
    return rev[(e - 1) // 2]                      # bitrev is an involution


# -- keys and phases ------------------------------------------------------------------------------------------------------------------
def automorphism_key(rng, w, S, t, n, beta, ell, noise=0):
    """AK for sigma_t, coefficient domain: row (r, l) = uniform mask polynomials, body = sum_q A_q (*) S_q + e + sigma_t(S_r) 2^(w - beta l).
    S: k polynomials of ints; rng: random.Random.  -> k * ell * (k + 1) * n ints"""
    M, k, key = 1 << w, len(S), []
    for r in range(k):
        rot = autom_gather([s % M for s in S[r]], t, w)
        for l in range(1, ell + 1):
            body = [rng.randint(-noise, noise) if noise else 0 for _ in range(n)]
            for q in range(k):
                a = [rng.randrange(M) for _ in range(n)]
                key += a
                body = [x + y for x, y in zip(body, negacyclic(a, [s % M for s in S[q]], w))]
            key += [(x + y * (1 << (w - beta * l))) % M for x, y in zip(body, rot)]
    return key


def trace_keys(rng, w, S, steps, n, beta, ell, noise=0):
    return [v for t in trace_exponents(n, steps) for v in automorphism_key(rng, w, S, t, n, beta, ell, noise)]


def phase(ct, S, w):
    """body - sum_q mask_q (*) S_q mod 2^w of one ciphertext of (k + 1) * n ints"""
    k, M = len(S), 1 << w
    n = len(ct) // (k + 1)
    out = list(ct[k * n:])
    for q in range(k):
        out = [(x - y) % M for x, y in zip(out, negacyclic(ct[q * n:(q + 1) * n], [s % M for s in S[q]], w))]
    return out


# -- calls 3 and 4 --------------------------------------------------------------------------------------------------------------------
def model_autoks(ct, key, w, t, k, n, beta, ell, add_input):
    """The header's formula for one ciphertext: ct (k + 1) * n ints, key k * ell * (k + 1) polynomials in the coefficient domain."""
    M = 1 << w
    out = [[0] * n for _ in range(k + 1)]
    out[k] = autom_gather(ct[k * n:], t, w)
    if add_input:
        out = [[x + y for x, y in zip(row, ct[q * n:(q + 1) * n])] for q, row in enumerate(out)]
    for r in range(k):
        dig = [digits(x, w, beta, ell) for x in autom_gather(ct[r * n:(r + 1) * n], t, w)]
        for l in range(ell):
            D = [d[l] % M for d in dig]
            for q in range(k + 1):
                base = ((r * ell + l) * (k + 1) + q) * n
                out[q] = [x - y for x, y in zip(out[q], negacyclic(D, key[base:base + n], w))]
    return [v % M for row in out for v in row]


def model_trace(ct, keys, w, steps, k, n, beta, ell):
    per = k * ell * (k + 1) * n
    cur = list(ct)
    for r, t in enumerate(trace_exponents(n, steps)):
        cur = model_autoks(cur, keys[r * per:(r + 1) * per], w, t, k, n, beta, ell, True)
    return cur
