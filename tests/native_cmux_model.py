"""The plain-int model of include/cntt_cmux.h: the CMux of two GLWE ciphertexts over Z/2^w[X]/(X^n + 1) against a GGSW selector
(schoolbook negacyclic products mod 2^w, the digits of cntt_gadget.h), the leaf stage of the tree on plain table polynomials, the whole
tree, noise-free and noisy selectors, and the header's workspace formulas and grid rule.  tests/test_native_cmux_model.py checks these
against the header's statements.  No GPU needed; not a test module."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_cmux.h")


def up(x):
    return (x + 255) & ~255


def cmux_workspace_bytes(n, word, k, levels, batch):
    return up(batch * (k + 1) * levels * n * word)


def cmux_tree_workspace_bytes(n, word, m, k, levels, batch):
    H, Q = m // 2, m // 4
    return (up(max(batch * H * levels, batch * Q * (k + 1) * levels) * n * word) + up(batch * H * (k + 1) * n * word)
            + up(batch * Q * (k + 1) * n * word))


def grid(polys, logn, word):
    """the rule cntt_native_cmux_grid exports: one workgroup per polynomial up to 8 per CU of a 256-CU part; nothing is staged"""
    return max(1, min(polys, 8 * 256))


def selector_polys(k, ell):
    return (k + 1) * ell * (k + 1)


# -- the ring -------------------------------------------------------------------------------------------------------------------------
def digits(x, w, beta, ell):
    """the signed digits of cntt_native_gadget_decompose_batch, the sequential rule: round to a multiple of 2^s (ties up), then base-B
    digits in [-B/2, B/2) with carries, d_1 (most significant) first"""
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


def digits_by_offset(x, w, beta, ell):
    """the same digits the way the kernels take them (native_gadget.hpp): y = x + off, d_l = ((y >> (w - beta l)) & (B - 1)) - B / 2"""
    s = w - beta * ell
    off = (1 << (s - 1)) if s else 0
    for l in range(1, ell + 1):
        off += 1 << (w - beta * l + beta - 1)
    y = (x + off) % (1 << w)
    return [((y >> (w - beta * l)) & ((1 << beta) - 1)) - (1 << (beta - 1)) for l in range(1, ell + 1)]


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


# -- call 1 -------------------------------------------------------------------------------------------------------------------------
def ext_product_into(out, polys, rows, w, k, n, beta, ell):
    """out[o] += sum over the polynomials f of `polys` and the levels l of d_l(f) (*) rows[(i ell + l - 1) (k + 1) + o]; out: k + 1 lists"""
    M = 1 << w
    for i, f in enumerate(polys):
        dig = [digits(x, w, beta, ell) for x in f]
        for l in range(ell):
            D = [d[l] % M for d in dig]
            for o in range(k + 1):
                base = ((i * ell + l) * (k + 1) + o) * n
                out[o] = [(x + y) % M for x, y in zip(out[o], negacyclic(D, rows[base:base + n], w))]
    return out


def model_cmux(c0, c1, sel, w, k, n, beta, ell):
    """c0 + ExtProd(sel, c1 - c0): ciphertexts of (k + 1) n ints, sel: (k + 1) ell (k + 1) coefficient-domain polynomials"""
    M = 1 << w
    d = [[(y - x) % M for x, y in zip(c0[q * n:(q + 1) * n], c1[q * n:(q + 1) * n])] for q in range(k + 1)]
    out = ext_product_into([list(c0[q * n:(q + 1) * n]) for q in range(k + 1)], d, sel, w, k, n, beta, ell)
    return [v for row in out for v in row]


# -- call 2 -------------------------------------------------------------------------------------------------------------------------
def trivial(f, k, n):
    return [0] * (k * n) + list(f)


def model_leaf(f0, f1, sel, w, k, n, beta, ell):
    """stage 1 as the header defines it: zero masks, body f0, the digits of f1 - f0 against the BODY rows of the selector only"""
    out = [[0] * n for _ in range(k)] + [list(f0)]
    d = [(y - x) % (1 << w) for x, y in zip(f0, f1)]
    out = ext_product_into(out, [d], sel[k * ell * (k + 1) * n:], w, k, n, beta, ell)
    return [v for row in out for v in row]


def stage_params(m):
    """[(h, selector index)] of the stages s = 1 .. log2 m"""
    depth = m.bit_length() - 1
    return [(m >> s, depth - s) for s in range(1, depth + 1)]


def model_tree(lut, sels, w, m, k, n, beta, ell):
    """lut: m lists of n ints; sels: log2 m selectors back to back, coefficient domain -> (k + 1) n ints"""
    per = selector_polys(k, ell) * n
    cur = list(lut)
    for s, (h, i) in enumerate(stage_params(m), 1):
        node = model_leaf if s == 1 else model_cmux
        cur = [node(cur[j], cur[j + h], sels[i * per:(i + 1) * per], w, k, n, beta, ell) for j in range(h)]
    return cur[0] if m > 1 else trivial(cur[0], k, n)


# -- selectors ------------------------------------------------------------------------------------------------------------------------
def ggsw(rng, w, S, bit, n, beta, ell, noise=0):
    """GGSW(bit) in the coefficient domain, the layout of one iteration's slice of bsk_ntt: row (q, l) = uniform masks A, body =
    sum_r A_r (*) S_r + e, plus bit * 2^(w - beta l) on polynomial q.  S: k polynomials of ints; rng: random.Random."""
    M, k, out = 1 << w, len(S), []
    for q in range(k + 1):
        for l in range(1, ell + 1):
            g = bit << (w - beta * l)
            body = [rng.randint(-noise, noise) % M if noise else 0 for _ in range(n)]
            row = []
            for r in range(k):
                a = [rng.randrange(M) for _ in range(n)]
                body = [(x + y) % M for x, y in zip(body, negacyclic(a, [s % M for s in S[r]], w))]
                row.append(a)
            row.append(body)
            row[q][0] = (row[q][0] + g) % M
            out += [v for poly in row for v in poly]
    return out


def phase(ct, S, w):
    """body - sum_q mask_q (*) S_q mod 2^w of one ciphertext of (k + 1) n ints"""
    k, M = len(S), 1 << w
    n = len(ct) // (k + 1)
    out = list(ct[k * n:])
    for q in range(k):
        out = [(x - y) % M for x, y in zip(out, negacyclic(ct[q * n:(q + 1) * n], [s % M for s in S[q]], w))]
    return out
