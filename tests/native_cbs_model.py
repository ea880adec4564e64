"""The plain-int model of include/cntt_cbs.h on top of tests/native_cmux_model.py: the key generators (bootstrapping key and the k + 1
functional packing keys, plain words in the coefficient domain, optional noise), steps 1 - 3 of the convention up to the selector words,
the public packing recipe of cntt_pack.h on the ciphertext (u, 0), and the header's workspace formula, slab rule and grid rule.
tests/test_native_cbs_model.py checks these against the header's statements.  No GPU needed; not a test module."""
import os

from native_cmux_model import digits, ggsw, negacyclic, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_cbs.h")


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
    return (up((L + 1) * E * 4) + up(E * ct) + up(E * ct * pbs_levels) + up(E * ct) + up(E * R * 4) + up(S * (k + 1) * E * ct)
            + up((k + 1) * E * ct))


def grid(items, logn, word):
    """the rule cntt_native_cbs_grid exports: one workgroup per work item up to 8 per CU of a 256-CU part"""
    return max(1, min(items, 8 * 256))


# -- constants --------------------------------------------------------------------------------------------------------------------------
def G(w, cbs_beta, l):
    return 1 << (w - cbs_beta * l)


def H(w, cbs_beta, l):
    return 1 << (w - cbs_beta * l - 1)


def ms(x, w, logn):
    """cntt_pbs.h"""
    return (((x >> (w - logn - 2)) + 1) >> 1) % (2 << logn)


# -- keys, coefficient domain -------------------------------------------------------------------------------------------------------------
def flatten(S):
    """s_in of the header: the GLWE key polynomials back to back"""
    return [c for poly in S for c in poly]


def glwe_encrypt(rng, w, S, msg, n, noise=0):
    """(k + 1) n ints: uniform masks, body = sum_r A_r (*) S_r + msg + e"""
    M = 1 << w
    body = [(m + (rng.randint(-noise, noise) if noise else 0)) % M for m in msg]
    row = []
    for Sr in S:
        a = [rng.randrange(M) for _ in range(n)]
        body = [(x + y) % M for x, y in zip(body, negacyclic(a, [s % M for s in Sr], w))]
        row += a
    return row + body


def bsk(rng, w, s_lwe, S, n, beta, ell, noise=0):
    """the bootstrapping key of cntt_pbs.h: one GGSW(s_lwe[i]) per LWE mask word"""
    return [x for s in s_lwe for x in ggsw(rng, w, S, s, n, beta, ell, noise)]


def fpksk(rng, w, S, n, ks_beta, Lk, noise=0):
    """the k + 1 functional keys F_0 .. F_k of the header under the output key S, which is also the key s_in flattens: row (i, j) of F_q
    encrypts the polynomial s_in[i] M_q 2^(w - ks_beta j) for i < Lin and -M_q 2^(w - ks_beta j) for i = Lin; M_q = -S_q, M_k = 1"""
    k, M = len(S), 1 << w
    s_in = flatten(S)
    out = []
    for q in range(k + 1):
        Mq = [1] + [0] * (n - 1) if q == k else [-c for c in S[q]]
        for i in range(k * n + 1):
            f = s_in[i] if i < k * n else -1
            for j in range(1, Lk + 1):
                out += glwe_encrypt(rng, w, S, [(f * m << (w - ks_beta * j)) % M for m in Mq], n, noise)
    return out


# -- steps 1 and 2 ------------------------------------------------------------------------------------------------------------------------
def rotate(f, a, w):
    """X^a f in Z/2^w[X]/(X^n + 1), a < 2n"""
    n, M = len(f), 1 << w
    g = [0] * n
    for i in range(n):
        t = (i - a) % (2 * n)
        g[i] = f[t % n] if t < n else (-f[t % n]) % M
    return g


def model_blind_rotate(lut, rot, bsk_rows, w, k, n, beta, ell):
    """cntt_pbs.h: acc = X^rot[L] lut, then acc += ExtProd(bsk_i, X^rot[i] acc - acc); lut, acc: k + 1 lists"""
    M, L = 1 << w, len(rot) - 1
    acc = [rotate(f, rot[L], w) for f in lut]
    per = (k + 1) * ell * (k + 1) * n
    for i in range(L):
        diff = [[(x - y) % M for x, y in zip(rotate(f, rot[i], w), f)] for f in acc]
        key = bsk_rows[i * per:(i + 1) * per]
        new = [list(f) for f in acc]
        for p, f in enumerate(diff):
            dig = [digits(x, w, beta, ell) for x in f]
            for l in range(ell):
                D = [d[l] % M for d in dig]
                for o in range(k + 1):
                    base = ((p * ell + l) * (k + 1) + o) * n
                    new[o] = [(x + y) % M for x, y in zip(new[o], negacyclic(D, key[base:base + n], w))]
        acc = new
    return acc


def model_extract(glwe, w):
    """sample extraction at index 0: k + 1 lists of n ints -> k n + 1 ints"""
    n, M, k = len(glwe[0]), 1 << w, len(glwe) - 1
    out = []
    for p in range(k):
        out += [glwe[p][0]] + [(-glwe[p][n - j]) % M for j in range(1, n)]
    return out + [glwe[k][0]]


def model_u(lwe, bsk_rows, w, L, k, n, pbs_beta, pbs_ell, cbs_beta, l):
    """steps 1 and 2 for one element and one level: the Lin + 1 words of u[b][l]"""
    M, logn = 1 << w, n.bit_length() - 1
    x = list(lwe)
    x[L] = (x[L] + (1 << (w - 2))) % M
    rot = [ms(v, w, logn) for v in x[:L]] + [(2 * n - ms(x[L], w, logn)) % (2 * n)]
    h = H(w, cbs_beta, l)
    lut = [[0] * n for _ in range(k)] + [[M - h] * n]
    u = model_extract(model_blind_rotate(lut, rot, bsk_rows, w, k, n, pbs_beta, pbs_ell), w)
    u[k * n] = (u[k * n] + h) % M
    return u


# -- step 3 -------------------------------------------------------------------------------------------------------------------------------
def model_keyswitch_rows(u, F, w, k, n, ks_beta, Lk):
    """step 3 for one u: the (k + 1) polynomials-of-(k + 1) n-words out[q] = -sum_{i,j} d_{i,j} F_q[(i Lk + j - 1) (k + 1) + o] mod 2^w"""
    M = 1 << w
    dig = [d for x in u for d in digits(x, w, ks_beta, Lk)]
    R, C = len(dig), (k + 1) * n
    out = []
    for q in range(k + 1):
        base = q * R * C
        acc = [0] * C
        for r, d in enumerate(dig):
            if d:
                row = F[base + r * C:base + (r + 1) * C]
                acc = [a + d * x for a, x in zip(acc, row)]
        out.append([(-a) % M for a in acc])
    return out


def model_pack_rows(u, F, w, k, n, ks_beta, Lk):
    """the formula of cntt_pack.h on the ciphertext (u, 0), lwe_dim_in = Lin + 1, lwe_count = 1, once per key F_q:
    glwe_out[p] = (the body polynomial, here 0, if p == k) - sum_{i,l} D_{i,l} (*) K[i levels + l - 1][p], D_{i,l} = the polynomial whose
    coefficient 0 is digit l of u[i] and whose other coefficients are 0 -- through the negacyclic product, as the public call runs it"""
    M, lin1 = 1 << w, len(u)
    out = []
    for q in range(k + 1):
        K = F[q * lin1 * Lk * (k + 1) * n:(q + 1) * lin1 * Lk * (k + 1) * n]
        g = [[0] * n for _ in range(k + 1)]
        for i, x in enumerate(u):
            for l, d in enumerate(digits(x, w, ks_beta, Lk)):
                D = [d % M] + [0] * (n - 1)
                for p in range(k + 1):
                    base = ((i * Lk + l) * (k + 1) + p) * n
                    g[p] = [(a - b) % M for a, b in zip(g[p], negacyclic(D, K[base:base + n], w))]
        out.append([v for poly in g for v in poly])
    return out


def selector_from_rows(rows_per_level, k, n):
    """rows_per_level[l - 1][q] = the (k + 1) n words of row (q, l) -> one selector in the layout of cntt_cmux.h"""
    Lc = len(rows_per_level)
    return [x for q in range(k + 1) for l in range(Lc) for x in rows_per_level[l][q]]


def model_circuit_bootstrap(lwe, bsk_rows, F, w, L, k, n, pbs_beta, pbs_ell, ks_beta, Lk, cbs_beta, Lc):
    """one element: the selector words of steps 1 - 3 (coefficient domain), which native_cmux_model.model_tree takes"""
    rows = [model_keyswitch_rows(model_u(lwe, bsk_rows, w, L, k, n, pbs_beta, pbs_ell, cbs_beta, l), F, w, k, n, ks_beta, Lk)
            for l in range(1, Lc + 1)]
    return selector_from_rows(rows, k, n)


def lwe_phase(u, s, w):
    return (u[-1] - sum(a * b for a, b in zip(u, s))) % (1 << w)


def lwe_encrypt(rng, w, s, msg, noise=0):
    M = 1 << w
    a = [rng.randrange(M) for _ in s]
    return a + [(sum(x * y for x, y in zip(a, s)) + msg + (rng.randint(-noise, noise) if noise else 0)) % M]
