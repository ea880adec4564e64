"""The plain-int model of include/cntt_multibit.h: the accumulate step per residue prime (the monomial identity and the subset-sum
exponents are those of tests/prime_multibit_model.py, imported and not restated) with the factor n^-1 the native call folds into its
table; the kernel's own arithmetic -- four products in one 64-bit sum, one Montgomery reduction, a 32-bit running sum -- restated; a
vectorised form of the per-prime step for large batches; and the group step and the rotation in the ring Z/2^w[X]/(X^n + 1) as the
schoolbook expression.  tests/test_native_multibit_model.py checks this file on the CPU; the GPU tests compare the kernels with it."""
import numpy as np

from prime_multibit_model import bitrev, mb_offset, model_accumulate, subset_exponents  # noqa: F401  (mb_offset: re-exported)

PRIMES32 = [1062862849, 1063059457, 1064697857, 1065484289, 1068236801, 1068433409, 1068564481, 1069219841, 1071513601, 1073479681]
# kind name -> (nprimes, word bits, binary)
KINDS = {"native32_plan32": (3, 32, False), "native64_plan32": (5, 64, False), "native128_plan32": (10, 128, False),
         "native_binary32_plan32": (2, 32, True), "native_binary64_plan32": (3, 64, True), "native_binary128_plan32": (5, 128, True)}
LAZY_TERMS = 4
R = 1 << 32


def model_accumulate_native(terms, key, rot_rows, psis, n, nterms, nout, g, batch):
    """terms[i], key[i]: plane i as flat lists of ints; psis[i]: the root of sub-plan i -> the nprimes output planes of
    cntt_native_multibit_accumulate_batch: n^-1 times the prime call's words"""
    out = []
    for i, psi in enumerate(psis):
        p = PRIMES32[i]
        ninv = pow(n, -1, p)
        out.append([x * ninv % p for x in model_accumulate(terms[i], key[i], rot_rows, psi, n, p, nterms, nout, g, batch)])
    return out


def redc(w, p):
    """the kernel's reduction: w < 2^32 p -> w 2^-32 mod p through (w + m p) / 2^32 < 2 p and one conditional subtraction"""
    assert 0 <= w < R * p
    m = (w % R) * (-pow(p, -1, R) % R) % R
    u = (w >> 32) + ((m * p) >> 32) + (1 if w % R else 0)
    assert u == (w + m * p) >> 32 and u < 2 * p < R
    return u - p if u >= p else u


def lazy_inner_sum(xs, ys, p):
    """sum_j xs[j] ys[j] 2^-32 mod p as the kernel forms it: chunks of four products in a 64-bit register (asserted not to wrap), one
    reduction per chunk, a 32-bit running sum with one conditional subtraction"""
    s = 0
    for j0 in range(0, len(xs), LAZY_TERMS):
        w = 0
        for x, y in zip(xs[j0:j0 + LAZY_TERMS], ys[j0:j0 + LAZY_TERMS]):
            w += x * y
            assert w < 1 << 64
        s += redc(w, p)
        assert s < R
        if s >= p:
            s -= p
    return s


def lazy_word(xs_by_pattern, ys_by_pattern, tab_words, p):
    """one output word as the kernel forms it: per pattern the lazy inner sum, a Montgomery product with the table word
    (+-psi^m n^-1 2^64), a canonical running sum"""
    acc = 0
    for xs, ys, tw in zip(xs_by_pattern, ys_by_pattern, tab_words):
        acc = (acc + redc(lazy_inner_sum(xs, ys, p) * tw, p)) % p
    return acc


def fast_accumulate_plane(terms, key, rot_rows, psi, n, p, nterms, nout, g, batch):
    """model_accumulate times n^-1 for ONE plane on uint64 arrays (p < 2^30: a product is below 2^60 and is reduced at once).
    terms: batch*nterms*n, key: 2^g*nterms*nout*n, any integer arrays -> uint32 array batch*nout*n"""
    logn = n.bit_length() - 1
    T = np.asarray(terms, dtype=np.uint64).reshape(batch, nterms, 1, n)
    K = np.asarray(key, dtype=np.uint64).reshape(1 << g, nterms, nout, n)
    P = np.uint64(p)
    idx = np.array([2 * bitrev(c, logn) + 1 for c in range(n)], dtype=np.uint64)
    ninv = pow(n, -1, p)
    table = np.array([pow(psi, m, p) * ninv % p for m in range(2 * n)], dtype=np.uint64)
    rows = np.asarray(rot_rows, dtype=np.uint64).reshape(g, batch) % np.uint64(2 * n)
    out = np.zeros((batch, nout, n), dtype=np.uint64)
    for t in range(1 << g):
        e = np.zeros(batch, dtype=np.uint64)
        for q in range(g):
            if (t >> q) & 1:
                e += rows[q]
        s = np.zeros((batch, nout, n), dtype=np.uint64)
        for j in range(nterms):
            s = (s + T[:, j] * K[t, j][None] % P) % P
        mono = table[(e[:, None] * idx[None, :]) % np.uint64(2 * n)]
        out = (out + s * mono[:, None, :] % P) % P
    return out.reshape(-1).astype(np.uint32)


# -- the ring Z/2^w[X]/(X^n + 1) ----------------------------------------------------------------------------------------------------------
def digits(x, w, beta, ell):
    """the signed digits of cntt_native_gadget_decompose_batch (the closed rule of tests/test_native_gadget_abi.py), d_1 first"""
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


def plain_terms(elem, w, beta, ell):
    """elem: npolys lists of n ints -> the npolys * ell CNTT_SRC_PLAIN term polynomials as words mod 2^w"""
    row = []
    for f in elem:
        ds = [digits(x, w, beta, ell) for x in f]
        row.extend([[d[l] % (1 << w) for d in ds] for l in range(ell)])
    return row


def negacyclic_int(a, b):
    """the exact integer product in Z[X]/(X^n + 1) on object arrays"""
    n = len(a)
    bo = np.array([int(x) for x in b], dtype=object)
    wide = np.zeros(2 * n, dtype=object)
    for i, x in enumerate(a):
        if x:
            wide[i:i + n] += int(x) * bo
    return wide[:n] - wide[n:]


def rotate(f, e, M):
    """X^e f in Z/M[X]/(X^n + 1), e < 2n"""
    n = len(f)
    g = [0] * n
    for i in range(n):
        t = (i - e) % (2 * n)
        g[i] = f[t % n] if t < n else (-f[t % n]) % M
    return g


def ring_group_step(terms, a, keys, w):
    """terms: J term polynomials (words mod 2^w); a: the group's g exponents; keys[t][j][o]: key polynomials as words
    -> sum_t X^(e_t) sum_j terms[j] (*) keys[t][j][o] mod 2^w: the schoolbook expression, nout lists"""
    n, M, nout = len(terms[0]), 1 << w, len(keys[0][0])
    out = [[0] * n for _ in range(nout)]
    for t, e in enumerate(subset_exponents(a, n)):
        for o in range(nout):
            s = np.zeros(n, dtype=object)
            for j, d in enumerate(terms):
                s = s + negacyclic_int(d, keys[t][j][o])
            out[o] = [(x + y) % M for x, y in zip(out[o], rotate([int(v) % M for v in s], e, M))]
    return out


def model_multibit_rotate(lut, rot_t, key, w, n, L, k, beta, ell, g, batch, per_element=False):
    """lut: (k + 1) * n ints (or batch times that); rot_t: (L + 1) * batch; key: bsk_mb in the COEFFICIENT domain as words, flat, laid
    out by mb_offset -> batch * (k + 1) * n ints"""
    J, M = (k + 1) * ell, 1 << w
    out = []
    for b in range(batch):
        base = b * (k + 1) * n if per_element else 0
        acc = [rotate(lut[base + q * n:base + (q + 1) * n], int(rot_t[L * batch + b]), M) for q in range(k + 1)]
        for r in range(L // g):
            keys = [[[key[mb_offset(r, t, j, o, g, J, k) * n:][:n] for o in range(k + 1)] for j in range(J)] for t in range(1 << g)]
            acc = ring_group_step(plain_terms(acc, w, beta, ell), [int(rot_t[(r * g + i) * batch + b]) for i in range(g)], keys, w)
        for q in range(k + 1):
            out += acc[q]
    return out
