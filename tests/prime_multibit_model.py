"""The plain-int model of include/cntt_prime_multibit.h: the transformed monomial in closed form, the subset-sum exponents, the
pointwise bundle step in the NTT domain (what prime_multibit_accumulate_kernel computes), and the group step and the whole rotation in
the ring with exact negacyclic products.  Digits, source polynomials, modulus switch and extraction are those of
tests/test_prime_pbs_model.py, imported and not restated.  tests/test_prime_multibit_model.py checks this file against its
specification on the CPU; the GPU tests compare the kernels with it."""
import numpy as np

from test_prime_pbs_model import model_terms_element, source, wbits

PG64 = 9224497936763846657          # 64-bit Montgomery class
P51 = 2251799813554177
P31 = 2147352577                    # 32-bit strict range
PW63 = 8717305756806021121          # strict range, the reference's Barrett product wraps
PW31 = 2088517633


def bitrev(c, logn):
    return int(format(c, "0%db" % logn)[::-1], 2) if logn else 0


def monomial_ntt(e, psi, n, p):
    """fwd(X^e) in closed form: psi^(e (2 bitrev(c) + 1) mod 2n), psi the plan's primitive 2n-th root"""
    logn = n.bit_length() - 1
    return [pow(psi, (e * (2 * bitrev(c, logn) + 1)) % (2 * n), p) for c in range(n)]


def subset_exponents(a, n):
    """a: the g exponents of one element -> e_t for t < 2^g; bit i of t (least significant first) selects a[i]"""
    return [sum(x for i, x in enumerate(a) if (t >> i) & 1) % (2 * n) for t in range(1 << len(a))]


def mb_offset(r, t, j, o, g, J, k):
    """polynomial index of key[r][t][j][o] in bsk_mb"""
    return ((r * (1 << g) + t) * J + j) * (k + 1) + o


def model_accumulate(terms, key, rot_rows, psi, n, p, nterms, nout, g, batch):
    """terms: batch*nterms*n ints, key: 2^g*nterms*nout*n ints, rot_rows: g*batch ints -> batch*nout*n ints (lists or arrays of
    Python ints).  Object arrays: every product is exact."""
    T = np.array(terms, dtype=object).reshape(batch, nterms, n)
    K = np.array(key, dtype=object).reshape(1 << g, nterms, nout, n)
    out = np.zeros((batch, nout, n), dtype=object)
    mono = {}
    for b in range(batch):
        es = subset_exponents([int(rot_rows[i * batch + b]) % (2 * n) for i in range(g)], n)
        for t, e in enumerate(es):
            if e not in mono:
                mono[e] = np.array(monomial_ntt(e, psi, n, p), dtype=object)
            for o in range(nout):
                s = np.zeros(n, dtype=object)
                for j in range(nterms):
                    s = (s + T[b, j] * K[t, j, o]) % p
                out[b, o] = (out[b, o] + mono[e] * s) % p
    return [int(x) for x in out.reshape(-1)]


def negacyclic_fast(a, b, p):
    """exact product in Z_p[X]/(X^n + 1): the words of test_prime_pbs_model.negacyclic, row by row on object arrays"""
    n = len(a)
    bo = np.array([int(x) for x in b], dtype=object)
    wide = np.zeros(2 * n, dtype=object)
    for i, x in enumerate(a):
        if x:
            wide[i:i + n] += int(x) * bo
    return [int(v) % p for v in (wide[:n] - wide[n:])]


def model_group_step(elem, a, keys, p, beta, ell):
    """elem: k + 1 lists of n ints; a: the group's g exponents; keys[t][j][o]: coefficient-domain key polynomials (lists of n ints)
    -> sum_t X^(e_t) ExtProd(keys[t], elem), k + 1 lists"""
    n, npolys = len(elem[0]), len(elem)
    terms = model_terms_element(elem, 0, p, beta, ell, mode="plain")
    out = [[0] * n for _ in range(npolys)]
    for t, e in enumerate(subset_exponents(a, n)):
        for o in range(npolys):
            s = [0] * n
            for j, d in enumerate(terms):
                s = [(x + y) % p for x, y in zip(s, negacyclic_fast(d, keys[t][j][o], p))]
            out[o] = [(x + y) % p for x, y in zip(out[o], source(s, e, p, "rotate"))]
    return out


def model_multibit_rotate(lut, rot_t, key, p, n, L, k, beta, ell, g, batch, per_element=False):
    """lut: (k + 1) * n ints (or batch times that); rot_t: (L + 1) * batch; key: bsk_mb in the COEFFICIENT domain, flat, laid out by
    mb_offset -> batch * (k + 1) * n ints"""
    J = (k + 1) * ell
    out = []
    for b in range(batch):
        base = b * (k + 1) * n if per_element else 0
        acc = [source(lut[base + q * n:base + (q + 1) * n], int(rot_t[L * batch + b]), p, "rotate") for q in range(k + 1)]
        for r in range(L // g):
            keys = [[[key[mb_offset(r, t, j, o, g, J, k) * n:][:n] for o in range(k + 1)] for j in range(J)] for t in range(1 << g)]
            acc = model_group_step(acc, [int(rot_t[(r * g + i) * batch + b]) for i in range(g)], keys, p, beta, ell)
        for q in range(k + 1):
            out += acc[q]
    return out


def trivial_ggsw(bit, p, n, k, beta, ell):
    """the noiseless GGSW ciphertext of `bit` with zero masks: row (q, l) is bit * 2^(W - beta l) on coefficient 0 of polynomial q;
    [j][o] -> n ints"""
    W = wbits(p)
    rows = []
    for q in range(k + 1):
        for l in range(1, ell + 1):
            row = [[0] * n for _ in range(k + 1)]
            row[q][0] = bit * pow(2, W - beta * l, p) % p
            rows.append(row)
    return rows


def flatten_keys(keys):
    """keys[r][t][j][o][c] -> the flat bsk_mb order"""
    return [c for grp in keys for pat in grp for row in pat for poly in row for c in poly]
