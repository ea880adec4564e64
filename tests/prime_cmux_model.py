"""The plain-int model of include/cntt_prime_cmux.h on top of tests/test_prime_pbs_model.py: the CMux of two GLWE ciphertexts against a
GGSW selector (big-integer negacyclic products, the header's digits, not negated), the leaf stage of the tree on plain table
polynomials, the whole tree, noise-free and noisy selectors, and the header's workspace formulas and grid rule.
tests/test_prime_cmux_model.py checks these against the header's statements.  No GPU needed; not a test module."""
import os

from prime_automorphism_model import up
from test_prime_pbs_model import negacyclic, signed_digits, wbits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_cmux.h")


def cmux_workspace_bytes(n, word, k, levels, batch):
    return up(batch * (k + 1) * levels * n * word)


def cmux_tree_workspace_bytes(n, word, m, k, levels, batch):
    H, Q = m // 2, m // 4
    return (up(max(batch * H * levels, batch * Q * (k + 1) * levels) * n * word) + up(batch * H * (k + 1) * n * word)
            + up(batch * Q * (k + 1) * n * word))


def grid(polys, logn, word):
    """the rule cntt_prime_cmux_grid exports: one workgroup per polynomial up to 8 per CU of a 256-CU part; nothing is staged"""
    return max(1, min(polys, 8 * 256))


def selector_polys(k, ell):
    return (k + 1) * ell * (k + 1)


# -- call 1 -------------------------------------------------------------------------------------------------------------------------
def ext_product_into(out, polys, rows, p, k, n, beta, ell):
    """out[o] += sum over the polynomials f of `polys` and the levels l of d_l(f) (*) rows[(i ell + l - 1) (k + 1) + o]; out: k + 1 lists"""
    for i, f in enumerate(polys):
        dig = [signed_digits(x, p, beta, ell) for x in f]
        for l in range(ell):
            D = [d[l] % p for d in dig]
            for o in range(k + 1):
                base = ((i * ell + l) * (k + 1) + o) * n
                out[o] = [(x + y) % p for x, y in zip(out[o], negacyclic(D, rows[base:base + n], p))]
    return out


def model_cmux(c0, c1, sel, p, k, n, beta, ell):
    """c0 + ExtProd(sel, c1 - c0): ciphertexts of (k + 1) n ints, sel: (k + 1) ell (k + 1) coefficient-domain polynomials"""
    d = [[(y - x) % p for x, y in zip(c0[q * n:(q + 1) * n], c1[q * n:(q + 1) * n])] for q in range(k + 1)]
    out = ext_product_into([list(c0[q * n:(q + 1) * n]) for q in range(k + 1)], d, sel, p, k, n, beta, ell)
    return [w for row in out for w in row]


# -- call 2 -------------------------------------------------------------------------------------------------------------------------
def trivial(f, k, n):
    return [0] * (k * n) + list(f)


def model_leaf(f0, f1, sel, p, k, n, beta, ell):
    """stage 1 as the header defines it: zero masks, body f0, the digits of f1 - f0 against the BODY rows of the selector only"""
    out = [[0] * n for _ in range(k)] + [list(f0)]
    d = [(y - x) % p for x, y in zip(f0, f1)]
    out = ext_product_into(out, [d], sel[k * ell * (k + 1) * n:], p, k, n, beta, ell)
    return [w for row in out for w in row]


def stage_params(m):
    """[(h, selector index)] of the stages s = 1 .. log2 m"""
    depth = m.bit_length() - 1
    return [(m >> s, depth - s) for s in range(1, depth + 1)]


def model_tree(lut, sels, p, m, k, n, beta, ell):
    """lut: m lists of n ints; sels: log2 m selectors back to back, coefficient domain -> (k + 1) n ints"""
    per = selector_polys(k, ell) * n
    cur = list(lut)
    for s, (h, i) in enumerate(stage_params(m), 1):
        node = model_leaf if s == 1 else model_cmux
        cur = [node(cur[j], cur[j + h], sels[i * per:(i + 1) * per], p, k, n, beta, ell) for j in range(h)]
    return cur[0] if m > 1 else trivial(cur[0], k, n)


# -- selectors ------------------------------------------------------------------------------------------------------------------------
def ggsw(rng, p, S, bit, n, beta, ell, noise=0):
    """GGSW(bit) in the coefficient domain, the layout of one iteration's slice of bsk_ntt: row (q, l) = uniform masks A, body =
    sum_r A_r (*) S_r + e, plus bit * 2^(W - beta l) on polynomial q.  S: k polynomials of ints; rng: random.Random."""
    W, k, out = wbits(p), len(S), []
    for q in range(k + 1):
        for l in range(1, ell + 1):
            g = bit << (W - beta * l)
            body = [rng.randint(-noise, noise) if noise else 0 for _ in range(n)]
            row = []
            for r in range(k):
                a = [rng.randrange(p) for _ in range(n)]
                body = [(x + y) % p for x, y in zip(body, negacyclic(a, [s % p for s in S[r]], p))]
                row.append(a)
            row.append(body)
            row[q][0] = (row[q][0] + g) % p
            out += [w % p for poly in row for w in poly]
    return out


def phase(ct, S, p):
    """body - sum_q mask_q (*) S_q mod p of one ciphertext of (k + 1) n ints"""
    k = len(S)
    n = len(ct) // (k + 1)
    out = list(ct[k * n:])
    for q in range(k):
        out = [(x - y) % p for x, y in zip(out, negacyclic(ct[q * n:(q + 1) * n], [s % p for s in S[q]], p))]
    return out
