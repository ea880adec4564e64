"""The plain-int model of include/cntt_prime_pack.h -- digits of tests/test_prime_pbs_model.py, transpose, negacyclic sums mod p -- in
the matrix form the GPU tests compare the device with and, naively, as the header's formula to the letter; the header's chunk C; a
noise-free key; and csrc/prime_pack.hpp's negated digits restated on tb-bit words.  tests/test_prime_pack_abi.py checks these
against each other and against the header's phase identity.  No GPU needed; not a test module."""
import os
import re

import numpy as np

from test_prime_pbs_model import signed_digits, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_pack.h")
PACK_TERMS = int(re.search(r"#define\s+CNTT_PRIME_PACK_TERMS\s+(\d+)", open(HEADER).read()).group(1))
TT, TI = 64, 32                      # prime_pack.hpp: ciphertexts x mask words of one workgroup's tile

PG64 = 9224497936763846657          # 64-bit Montgomery class: p >= 2^63 and not 2^64 - c
P31 = 2147352577                    # 32-bit strict range


def C(levels):
    """the chunk of mask words of one external product (cntt_prime_pack.h), before the cap at Lin"""
    return max(1, PACK_TERMS // levels)


def workspace_bytes(n, word, lin, levels, batch):
    """the header's formula: up(batch * C * levels * n * sizeof(T)), C capped at Lin"""
    return (batch * min(C(levels), lin) * levels * n * word + 255) // 256 * 256


def negacyclic(a, b, n):
    """a (*) b in Z[X]/(X^n + 1), Python ints"""
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < n:
                    out[i + j] += x * y
                else:
                    out[i + j - n] -= x * y
    return out


def model_pack_literal(lwe, key, p, lin, m, k, n, beta, ell):
    """The header's formula to the letter for one batch element.  lwe: m * (lin + 1) ints; key: lin * ell * (k + 1) polynomials of n
    ints (coefficient domain), K[r][q] at (r * (k + 1) + q) * n -> (k + 1) * n ints."""
    out = [[0] * n for _ in range(k + 1)]
    for t in range(m):
        out[k][t] = lwe[t * (lin + 1) + lin]
    for i in range(lin):
        dig = [signed_digits(lwe[t * (lin + 1) + i], p, beta, ell) for t in range(m)]
        for l in range(ell):
            D = [dig[t][l] for t in range(m)] + [0] * (n - m)              # the transpose: coefficient t from ciphertext t
            for q in range(k + 1):
                base = ((i * ell + l) * (k + 1) + q) * n
                for c, v in enumerate(negacyclic(D, key[base:base + n], n)):
                    out[q][c] -= v
    return [v % p for row in out for v in row]


def _digit_rows(cts, p, lin, m, beta, ell):
    return [[d for i in range(lin) for d in signed_digits(int(cts[t * (lin + 1) + i]), p, beta, ell)] for t in range(m)]


def model_pack_batch(lwe, key, p, lin, m, k, n, beta, ell, batch):
    """The same words as one matrix product per batch element: row t of D K is sum_r d_r(lwe_t) K[r], the output is the body polynomial
    minus sum_t X^t (row t), all mod p.  Exact integer arithmetic: where |digit| * rows * 2^32 stays below 2^62 the product runs in
    int64 on the two 32-bit halves of the key words, otherwise on Python ints; either way reduced once at the end."""
    rows = lin * ell
    half = 1 << (beta - 1)
    small = rows and half * rows < (1 << 30)
    if rows:
        if small:
            K64 = np.array(key, dtype=np.uint64).reshape(rows, (k + 1) * n)
            Klo, Khi = (K64 & np.uint64(0xFFFFFFFF)).astype(np.int64), (K64 >> np.uint64(32)).astype(np.int64)
        else:
            Kobj = np.array([int(x) for x in key], dtype=object).reshape(rows, (k + 1) * n)
    out = []
    for g in range(batch):
        cts = lwe[g * m * (lin + 1):(g + 1) * m * (lin + 1)]
        acc = np.zeros((k + 1, n), dtype=object)
        if rows:
            D = _digit_rows(cts, p, lin, m, beta, ell)
            if small:
                D = np.array(D, dtype=np.int64)
                A = D.dot(Klo).astype(object) + D.dot(Khi).astype(object) * (1 << 32)
            else:
                A = np.array(D, dtype=object).dot(Kobj)
            A = A.reshape(m, k + 1, n)
            for t in range(m):                                             # acc -= X^t A[t]
                acc[:, t:] -= A[t][:, :n - t]
                if t:
                    acc[:, :t] += A[t][:, n - t:]
        acc[k, :m] += np.array([int(cts[t * (lin + 1) + lin]) for t in range(m)], dtype=object)
        out += [int(x) % p for x in acc.reshape(-1)]
    return out


def noise_free_key(rng, p, s_in, S, k, n, beta, ell, noise=0):
    """row (i, l): uniform mask polynomials, body = sum_q A_q (*) S_q + e + s_in[i] 2^(W - beta l) at coefficient 0; rng: random.Random"""
    W, key = wbits(p), []
    for i in range(len(s_in)):
        for l in range(1, ell + 1):
            body = [rng.randint(-noise, noise) if noise else 0 for _ in range(n)]
            for q in range(k):
                a = [rng.randrange(p) for _ in range(n)]
                key += a
                body = [(x + y) % p for x, y in zip(body, negacyclic(a, S[q], n))]
            body[0] = (body[0] + s_in[i] * (1 << (W - beta * l))) % p
            key += [x % p for x in body]
    return key


def gadget_offset(p, beta, ell):
    """off of csrc/prime_pbs.hpp: 2^(s-1) + sum_{l >= 2} (B/2) 2^(W - beta l)"""
    W = wbits(p)
    s = W - beta * ell
    return ((1 << (s - 1)) if s else 0) + sum(1 << (W - beta * l + beta - 1) for l in range(2, ell + 1))


def kernel_negated_digits(x, p, beta, ell, tb):
    """prime_pack_decompose_kernel restated on tb-bit words: the canonical x read back from LDS, the lift, y = x' + off mod 2^tb, the
    top digit by an arithmetic shift when y is negative and a logical one otherwise, and the two selects that store -d mod p."""
    M, W = 1 << tb, wbits(p)
    sh1, off = W - beta, gadget_offset(p, beta, ell)
    mask, half = (1 << beta) - 1, 1 << (beta - 1)
    hi = x >= (p - x) % M
    y = (x + off - (p if hi else 0)) % M
    neg = hi and (y >> (tb - 1)) == 1
    d1 = (-((y - M) >> sh1)) % M if neg else y >> sh1          # Python's >> on a negative int floors, as the arithmetic shift does
    out = [d1 if neg or d1 == 0 else (p - d1) % M]
    sh = sh1
    for _ in range(1, ell):
        sh -= beta
        e = (y >> sh) & mask
        out.append(half - e if e <= half else (p - e + half) % M)
    return out
