"""The plain-int model of include/cntt_prime_automorphism.h: the automorphism sigma_t in gather form and as the scatter that defines it,
the NTT-slot permutation, the Galois keyswitch and the trace with the digits of tests/test_prime_pbs_model.py (as
tests/prime_pack_model.py uses them), automorphism keys with or without noise, the phase, and the header's workspace formulas.
tests/test_prime_automorphism_model.py checks these against each other, against the CPU oracle's transform and against the header's
phase statements.  No GPU needed; not a test module."""
import os

import numpy as np

from prime_pack_model import negacyclic
from test_prime_pbs_model import signed_digits, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_automorphism.h")
LDS_BYTES = 64 << 10                  # prime_automorphism.hpp: the largest polynomial the kernels stage through LDS


def up(x):
    return (x + 255) // 256 * 256


def autoks_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word)


def trace_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word) + up(batch * (k + 1) * n * word)


def trace_exponents(n, steps):
    return [(n >> r) + 1 for r in range(steps)]


# -- the automorphism ---------------------------------------------------------------------------------------------------------------
def autom_scatter(f, t, p):
    """the definition: X^i -> (-1)^floor(i t / n) X^(i t mod n)"""
    n = len(f)
    out = [0] * n
    for i, x in enumerate(f):
        e = i * t % (2 * n)
        out[e % n] = (-x) % p if e >= n else x % p
    return out


def autom_gather(f, t, p):
    """the header's gather form: out[j] = +-f[j tinv mod 2n]"""
    n = len(f)
    tinv = pow(t, -1, 2 * n)
    out = []
    for j in range(n):
        u = j * tinv % (2 * n)
        x = f[u % n]
        out.append((p - x) % p if u >= n and x else x)
    return out


def autom_gather_np(f, t, p):
    """autom_gather on a numpy array of canonical words (any leading shape, polynomials along the last axis)"""
    n = f.shape[-1]
    u = np.arange(n, dtype=np.int64) * pow(t, -1, 2 * n) % (2 * n)
    x = f[..., u % n]
    return np.where((u >= n) & (x != 0), f.dtype.type(p) - x, x)


def bitrev(x, logn):
    return int(format(x, "0%db" % logn)[::-1], 2) if logn else 0


def ntt_permutation(t, n):
    """src[c] = c' with 2 bitrev(c') + 1 = t (2 bitrev(c) + 1) mod 2n, as an index array: out_ntt = in_ntt[src]"""
    logn = n.bit_length() - 1
    c = np.arange(n, dtype=np.int64)
    rev = np.zeros(n, dtype=np.int64)
    for b in range(logn):
        rev |= ((c >> b) & 1) << (logn - 1 - b)
    e = t * (2 * rev + 1) % (2 * n)
    inv = np.empty(n, dtype=np.int64)
    inv[rev] = c                                  # bitrev is an involution: inv == rev, spelled out
    return inv[(e - 1) // 2]


# -- keys and phases ----------------------------------------------------------------------------------------------------------------
def automorphism_key(rng, p, S, t, n, beta, ell, noise=0):
    """AK for sigma_t, coefficient domain: row (r, l) = uniform mask polynomials, body = sum_q A_q (*) S_q + e + sigma_t(S_r) 2^(W - beta l).
    S: k polynomials of ints; rng: random.Random.  -> k * ell * (k + 1) * n ints"""
    W, k, key = wbits(p), len(S), []
    for r in range(k):
        rot = autom_gather(S[r], t, p)
        for l in range(1, ell + 1):
            body = [rng.randint(-noise, noise) if noise else 0 for _ in range(n)]
            for q in range(k):
                a = [rng.randrange(p) for _ in range(n)]
                key += a
                body = [x + y for x, y in zip(body, negacyclic(a, S[q], n))]
            key += [(x + y * (1 << (W - beta * l))) % p for x, y in zip(body, rot)]
    return key


def trace_keys(rng, p, S, steps, n, beta, ell, noise=0):
    return [w for t in trace_exponents(n, steps) for w in automorphism_key(rng, p, S, t, n, beta, ell, noise)]


def phase(ct, S, p):
    """body - sum_q mask_q (*) S_q mod p of one ciphertext of (k + 1) * n ints"""
    k = len(S)
    n = len(ct) // (k + 1)
    out = list(ct[k * n:])
    for q in range(k):
        out = [x - y for x, y in zip(out, negacyclic(ct[q * n:(q + 1) * n], S[q], n))]
    return [x % p for x in out]


# -- calls 3 and 4 ------------------------------------------------------------------------------------------------------------------
def model_autoks(ct, key, p, t, k, n, beta, ell, add_input):
    """The header's formula for one ciphertext: ct (k + 1) * n ints, key k * ell * (k + 1) polynomials in the coefficient domain."""
    out = [[0] * n for _ in range(k + 1)]
    out[k] = autom_gather(ct[k * n:], t, p)
    if add_input:
        out = [[x + y for x, y in zip(row, ct[q * n:(q + 1) * n])] for q, row in enumerate(out)]
    for r in range(k):
        dig = [signed_digits(x, p, beta, ell) for x in autom_gather(ct[r * n:(r + 1) * n], t, p)]
        for l in range(ell):
            D = [d[l] for d in dig]
            for q in range(k + 1):
                base = ((r * ell + l) * (k + 1) + q) * n
                out[q] = [x - y for x, y in zip(out[q], negacyclic(D, key[base:base + n], n))]
    return [v % p for row in out for v in row]


def model_autoks_batch(cts, key, p, t, k, n, beta, ell, add_input, batch):
    per = (k + 1) * n
    return [w for b in range(batch) for w in model_autoks(cts[b * per:(b + 1) * per], key, p, t, k, n, beta, ell, add_input)]


def model_trace(ct, keys, p, steps, k, n, beta, ell):
    per = k * ell * (k + 1) * n
    cur = list(ct)
    for r, t in enumerate(trace_exponents(n, steps)):
        cur = model_autoks(cur, keys[r * per:(r + 1) * per], p, t, k, n, beta, ell, True)
    return cur
