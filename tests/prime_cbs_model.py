"""The plain-int model of include/cntt_prime_cbs.h on top of tests/test_prime_pbs_model.py and tests/prime_cmux_model.py: the key
generators (bootstrapping key and the k + 1 functional packing keys, coefficient domain, optional noise), the three steps of the
convention, the keyswitch half on its own in the NTT domain, and the header's workspace formula, slab rule and grid rule.
tests/test_prime_cbs_model.py checks these against the header's statements.  No GPU needed; not a test module."""
import os

from prime_automorphism_model import up
from prime_cmux_model import ggsw
from test_prime_pbs_model import model_extract, model_terms_element, ms, negacyclic, signed_digits, source, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_cbs.h")


def ceil_div(a, b):
    return -(-a // b)


# -- the workspace formula, the slab rule, the grid rule --------------------------------------------------------------------------------
def shape(n, word, k, R, E):
    """(cols, tiles, rows, S) of the header"""
    cols = ceil_div((k + 1) * n, 256 * 16 // word)
    tiles = ceil_div(E, 8)
    s0 = max(1, min(ceil_div(R, 64), 2048 // ((k + 1) * cols * max(tiles, 1))))
    rows = ceil_div(R, s0)
    return cols, tiles, rows, ceil_div(R, rows)


def cbs_workspace_bytes(n, word, L, k, pbs_levels, Lk, Lc, batch):
    E, R = batch * Lc, (k * n + 1) * Lk
    S = shape(n, word, k, R, E)[3]
    ct = (k + 1) * n * word
    return up((L + 1) * E * 4) + up(E * ct) + up(E * ct * pbs_levels) + up(E * ct) + up(E * R * 4) + up(S * (k + 1) * E * ct)


def grid(items, logn, word):
    """the rule cntt_prime_cbs_grid exports: one workgroup per work item up to 8 per CU of a 256-CU part"""
    return max(1, min(items, 8 * 256))


# -- constants --------------------------------------------------------------------------------------------------------------------------
def G(p, cbs_beta, l):
    return (1 << (wbits(p) - cbs_beta * l)) % p


def H(p, cbs_beta, l):
    return G(p, cbs_beta, l) * ((p + 1) // 2) % p


def Q4(p):
    return (p + 2) // 4


# -- keys, coefficient domain -------------------------------------------------------------------------------------------------------------
def flatten(S):
    """s_in of the header: the GLWE key polynomials back to back"""
    return [c for poly in S for c in poly]


def glwe_encrypt(rng, p, S, msg, n, noise=0):
    """(k + 1) n ints: uniform masks, body = sum_r A_r (*) S_r + msg + e"""
    body = [(m + (rng.randint(-noise, noise) if noise else 0)) % p for m in msg]
    row = []
    for Sr in S:
        a = [rng.randrange(p) for _ in range(n)]
        body = [(x + y) % p for x, y in zip(body, negacyclic(a, [s % p for s in Sr], p))]
        row += a
    return row + body


def bsk(rng, p, s_lwe, S, n, beta, ell, noise=0):
    """the bootstrapping key of cntt_prime_pbs.h: one GGSW(s_lwe[i]) per LWE mask word"""
    return [w for s in s_lwe for w in ggsw(rng, p, S, s, n, beta, ell, noise)]


def fpksk(rng, p, S, n, ks_beta, Lk, noise=0):
    """the k + 1 functional keys F_0 .. F_k of the header under the output key S, which is also the key s_in flattens: row (i, j) of F_q
    encrypts the polynomial s_in[i] M_q 2^(W - ks_beta j) for i < Lin and -M_q 2^(W - ks_beta j) for i = Lin; M_q = -S_q, M_k = 1"""
    W, k = wbits(p), len(S)
    s_in = flatten(S)
    out = []
    for q in range(k + 1):
        Mq = [1] + [0] * (n - 1) if q == k else [-c for c in S[q]]
        for i in range(k * n + 1):
            f = s_in[i] if i < k * n else -1
            for j in range(1, Lk + 1):
                out += glwe_encrypt(rng, p, S, [(f * m << (W - ks_beta * j)) % p for m in Mq], n, noise)
    return out


# -- the three steps ----------------------------------------------------------------------------------------------------------------------
def model_blind_rotate(lut, rot, bsk_rows, p, k, n, beta, ell):
    """cntt_prime_pbs.h: acc = X^rot[L] lut, then acc += ExtProd(bsk_i, X^rot[i] acc - acc); lut, acc: k + 1 lists"""
    L = len(rot) - 1
    acc = [source(f, rot[L], p, "rotate") for f in lut]
    per = (k + 1) * ell * (k + 1) * n
    for i in range(L):
        terms = model_terms_element(acc, rot[i], p, beta, ell, "cmux")
        key = bsk_rows[i * per:(i + 1) * per]
        for j, t in enumerate(terms):
            for o in range(k + 1):
                base = (j * (k + 1) + o) * n
                acc[o] = [(x + y) % p for x, y in zip(acc[o], negacyclic(t, key[base:base + n], p))]
    return acc


def model_u(lwe, bsk_rows, p, L, k, n, pbs_beta, pbs_ell, cbs_beta, l):
    """steps 1 and 2 for one element and one level: the Lin + 1 words of u[b][l]"""
    logn = n.bit_length() - 1
    x = list(lwe)
    x[L] = (x[L] + Q4(p)) % p
    rot = [ms(w, p, logn) for w in x[:L]] + [(2 * n - ms(x[L], p, logn)) % (2 * n)]
    h = H(p, cbs_beta, l)
    lut = [[0] * n for _ in range(k)] + [[(p - h) % p] * n]
    u = model_extract(model_blind_rotate(lut, rot, bsk_rows, p, k, n, pbs_beta, pbs_ell), 0, p)
    u[k * n] = (u[k * n] + h) % p
    return u


def model_keyswitch_rows(u, F_ntt, p, k, n, ks_beta, Lk):
    """step 3 for one u: the (k + 1) (k + 1) polynomials out[q][o] = -sum_{i,j} d_{i,j} F_q[(i Lk + j - 1) (k + 1) + o] slot by slot.  F_ntt: the
    k + 1 keys in the NTT domain (any words: the statement is slot-wise arithmetic)"""
    dig = [d for x in u for d in signed_digits(x, p, ks_beta, Lk)]
    R, C = len(dig), (k + 1) * n
    out = []
    for q in range(k + 1):
        base = q * R * C
        acc = [0] * C
        for r, d in enumerate(dig):
            if d:
                row = F_ntt[base + r * C:base + (r + 1) * C]
                acc = [a + d * w for a, w in zip(acc, row)]
        out.append([(-a) % p for a in acc])
    return out


def selector_from_rows(rows_per_level, k, n):
    """rows_per_level[l - 1][q] = the (k + 1) n words of row (q, l) -> one selector in the layout of cntt_prime_cmux.h"""
    Lc = len(rows_per_level)
    return [w for q in range(k + 1) for l in range(Lc) for w in rows_per_level[l][q]]


def model_circuit_bootstrap(lwe, bsk_rows, F, p, L, k, n, pbs_beta, pbs_ell, ks_beta, Lk, cbs_beta, Lc):
    """one element, COEFFICIENT domain: F in the coefficient domain gives the selector in the coefficient domain (a constant digit times a
    polynomial is slot-wise in either domain), which prime_cmux_model.model_tree takes"""
    rows = [model_keyswitch_rows(model_u(lwe, bsk_rows, p, L, k, n, pbs_beta, pbs_ell, cbs_beta, l), F, p, k, n, ks_beta, Lk)
            for l in range(1, Lc + 1)]
    return selector_from_rows(rows, k, n)


def lwe_phase(u, s, p):
    return (u[-1] - sum(a * b for a, b in zip(u, s))) % p


def lwe_encrypt(rng, p, s, msg, noise=0):
    a = [rng.randrange(p) for _ in s]
    return a + [(sum(x * y for x, y in zip(a, s)) + msg + (rng.randint(-noise, noise) if noise else 0)) % p]
