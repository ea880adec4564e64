"""The plain-int model of include/cntt_prime_ring_pack.h on top of tests/prime_automorphism_model.py: the embedding of an LWE ciphertext
(the inverse of sample extraction at index 0), one node of the packing tree, the whole packing, LWE encryption under the flattened GLWE
key, numpy forms of the prefill for the GPU tests, and the header's workspace formulas and grid rule.
tests/test_prime_ring_pack_model.py checks these against the header's phase statements.  No GPU needed; not a test module."""
import os

import numpy as np

from prime_automorphism_model import autom_gather_np, model_autoks, model_trace, up
from test_prime_pbs_model import source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_ring_pack.h")
LDS_BYTES = 64 << 10                  # prime_ring_pack.hpp: the two staged polynomials together


def merge_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word)


def ring_pack_workspace_bytes(n, word, m, k, levels, batch):
    H, Q = max(m // 2, 1), max(m // 4, 1)
    return up(batch * H * k * levels * n * word) + up(batch * H * (k + 1) * n * word) + up(batch * Q * (k + 1) * n * word)


def grid(polys, logn, word):
    """the rule cntt_prime_ring_pack_grid exports: 8 workgroups per CU of a 256-CU part, fewer where 160 KiB hold fewer staged pairs"""
    pair = 2 * (word << logn)
    per_cu = min(8, max(1, (160 << 10) // pair)) if pair <= LDS_BYTES else 8
    return max(1, min(polys, per_cu * 256))


# -- call 1 -------------------------------------------------------------------------------------------------------------------------
def embed(lwe, p, k, n):
    """lwe: k n + 1 ints -> (k + 1) n ints"""
    out = []
    for q in range(k):
        out += [lwe[q * n]] + [(-lwe[q * n + n - i]) % p for i in range(1, n)]
    return out + [lwe[k * n]] + [0] * (n - 1)


def embed_np(lwe, p, k, n):
    """embed on a numpy array of canonical words, rows of k n + 1 words along the last axis"""
    lead = lwe.shape[:-1]
    out = np.zeros(lead + (k + 1, n), dtype=lwe.dtype)
    mask = lwe[..., :k * n].reshape(lead + (k, n))
    out[..., :k, 0] = mask[..., 0]
    rev = mask[..., :0:-1]
    out[..., :k, 1:] = np.where(rev != 0, lwe.dtype.type(p) - rev, rev)
    out[..., k, 0] = lwe[..., k * n]
    return out.reshape(lead + ((k + 1) * n,))


# -- call 2 -------------------------------------------------------------------------------------------------------------------------
def merge_parts(E, O, shift, p, k, n):
    """(a, d) = (E + X^shift O, E - X^shift O), ciphertexts of (k + 1) n ints"""
    a, d = [], []
    for q in range(k + 1):
        e, r = E[q * n:(q + 1) * n], source(O[q * n:(q + 1) * n], shift, p, "rotate")
        a += [(x + y) % p for x, y in zip(e, r)]
        d += [(x - y) % p for x, y in zip(e, r)]
    return a, d


def model_merge(E, O, key, p, shift, t, k, n, beta, ell):
    """a + AutoKS_t(d): the header's formula for one node; key: k * ell * (k + 1) coefficient-domain polynomials"""
    a, d = merge_parts(E, O, shift, p, k, n)
    return [(x + y) % p for x, y in zip(a, model_autoks(d, key, p, t, k, n, beta, ell, False))]


def rotate_np(f, shift, p):
    """X^shift f (CNTT_SRC_ROTATE) on a numpy array of canonical words, polynomials along the last axis"""
    n = f.shape[-1]
    r = (np.arange(n, dtype=np.int64) - shift) % (2 * n)
    x = f[..., r % n]
    return np.where((r >= n) & (x != 0), f.dtype.type(p) - x, x)


def merge_parts_np(E, O, shift, p):
    """(a, d) on numpy arrays of canonical words of any shape with polynomials along the last axis"""
    e, r = E.astype(object), rotate_np(O, shift, p).astype(object)
    return ((e + r) % p).astype(E.dtype), ((e - r) % p).astype(E.dtype)


def prefill_np(a, d, t, p, k, n):
    """the prefilled output of call 2 for ciphertext arrays a, d of shape (..., (k + 1) n): a with sigma_t(d body) added to the body"""
    out = a.reshape(a.shape[:-1] + (k + 1, n)).copy()
    body = autom_gather_np(d.reshape(out.shape)[..., k, :], t, p).astype(object)
    out[..., k, :] = ((out[..., k, :].astype(object) + body) % p).astype(a.dtype)
    return out.reshape(a.shape)


# -- call 3 -------------------------------------------------------------------------------------------------------------------------
def stage_params(n, m):
    """[(h, shift, t, key index)] of the stages s = 1 .. log2 m"""
    logn = n.bit_length() - 1
    return [(m >> s, n >> s, (1 << s) + 1, logn - s) for s in range(1, m.bit_length())]


def model_ring_pack(lwes, keys, p, m, k, n, beta, ell):
    """lwes: m lists of k n + 1 ints; keys: the log2 n trace keys back to back, coefficient domain -> (k + 1) n ints"""
    per = k * ell * (k + 1) * n
    cur = [embed(x, p, k, n) for x in lwes]
    for h, shift, t, r in stage_params(n, m):
        cur = [model_merge(cur[j], cur[j + h], keys[r * per:(r + 1) * per], p, shift, t, k, n, beta, ell) for j in range(h)]
    return model_trace(cur[0], keys, p, (n.bit_length() - 1) - (m.bit_length() - 1), k, n, beta, ell)


def lwe_encrypt(rng, p, S, phase, k, n):
    """an LWE ciphertext of k n + 1 ints under the flattened key s[q n + j] = S_q[j] whose phase body - <mask, s> is `phase`"""
    mask = [rng.randrange(p) for _ in range(k * n)]
    flat = [x for row in S for x in row]
    return mask + [(phase + sum(a * s for a, s in zip(mask, flat))) % p]
