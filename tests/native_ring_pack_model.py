"""The plain-int model of include/cntt_ring_pack.h on lists of Python ints mod 2^w (w = 32 / 64 / 128): the embedding of an LWE row, sample
extraction at index 0 (restated, to invert it), the rotation X^shift, one merge node by the header's formula, the whole pack as embed +
merges + trace, the headroom encoding and its decoding, and the header's workspace formulas and grid rule.  Built on
native_automorphism_model.py (digits, the Galois keyswitch, the trace, keys and phases).  tests/test_native_ring_pack_model.py checks
these against each other and against the header's statements on layout and factor.  No GPU needed; not a test module."""
import os

from native_automorphism_model import LDS_BYTES, model_autoks, model_trace, up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_ring_pack.h")


def merge_workspace_bytes(n, word, k, levels, batch):
    return up(batch * k * levels * n * word)


def ring_pack_workspace_bytes(n, word, m, k, levels, batch):
    h, q = max(m // 2, 1), max(m // 4, 1)
    return up(batch * h * k * levels * n * word) + up(batch * h * (k + 1) * n * word) + up(batch * q * (k + 1) * n * word)


def grid(polys, logn, word):
    """the rule cntt_native_ring_pack_grid exports: that of cntt_native_automorphism_grid with two staged polynomials"""
    size = (2 * word) << logn
    per_cu = min(8, max(1, (160 << 10) // size)) if 0 < size <= LDS_BYTES else 8
    return max(1, min(polys, per_cu * 256))


def stages(n, m):
    """[(s, h, shift, t, key index)] of the tree, then the number of trace steps"""
    logn, l = n.bit_length() - 1, m.bit_length() - 1
    return [(s, m >> s, n >> s, (1 << s) + 1, logn - s) for s in range(1, l + 1)], logn - l


# -- call 1 and its inverse -------------------------------------------------------------------------------------------------------------
def embed(lwe, w, k, n):
    """one LWE row of k n + 1 ints -> (k + 1) * n ints"""
    M = 1 << w
    out = []
    for q in range(k):
        out += [lwe[q * n] % M] + [(-lwe[q * n + n - i]) % M for i in range(1, n)]
    return out + [lwe[k * n] % M] + [0] * (n - 1)


def sample_extract0(glwe, w, k, n):
    """sample extraction at index 0, as cntt_pbs.h states it: mask word q n + j is glwe[q][0] for j = 0 and -glwe[q][n - j] beyond"""
    M = 1 << w
    out = []
    for q in range(k):
        f = glwe[q * n:(q + 1) * n]
        out += [f[0] % M] + [(-f[n - j]) % M for j in range(1, n)]
    return out + [glwe[k * n] % M]


def lwe_phase(lwe, S, w):
    """body - <mask, flattened key> mod 2^w"""
    flat = [s for row in S for s in row]
    return (lwe[-1] - sum(a * s for a, s in zip(lwe, flat))) % (1 << w)


# -- call 2 -----------------------------------------------------------------------------------------------------------------------------
def rotate(f, shift, w):
    """X^shift f: CNTT_SRC_ROTATE of cntt_gadget.h in gather form, 0 <= shift < 2n"""
    n, M = len(f), 1 << w
    out = []
    for i in range(n):
        r = (i - shift) % (2 * n)
        out.append((-f[r % n]) % M if r >= n else f[r % n] % M)
    return out


def merge(even, odd, key, w, shift, t, k, n, beta, ell):
    """glwe_out = a + AutoKS_t(d), a = E + X^shift O, d = E - X^shift O, polynomial by polynomial"""
    M = 1 << w
    a, d = [], []
    for q in range(k + 1):
        e, o = even[q * n:(q + 1) * n], rotate(odd[q * n:(q + 1) * n], shift, w)
        a += [(x + y) % M for x, y in zip(e, o)]
        d += [(x - y) % M for x, y in zip(e, o)]
    ks = model_autoks(d, key, w, t, k, n, beta, ell, False)
    return [(x + y) % M for x, y in zip(a, ks)]


# -- call 3 -----------------------------------------------------------------------------------------------------------------------------
def ring_pack(lwes, keys, w, k, n, beta, ell):
    """lwes: M rows; keys: all log2 n trace keys back to back, coefficient domain -> one ciphertext"""
    per = k * ell * (k + 1) * n
    cur = [embed(row, w, k, n) for row in lwes]
    tree, steps = stages(n, len(lwes))
    for _, h, shift, t, r in tree:
        cur = [merge(cur[j], cur[j + h], keys[r * per:(r + 1) * per], w, shift, t, k, n, beta, ell) for j in range(h)]
    return model_trace(cur[0], keys, w, steps, k, n, beta, ell)


# -- the headroom encoding ----------------------------------------------------------------------------------------------------------------
def encode(m, bits, w, n):
    """a message of `bits` bits at bit w - log2 n - bits: log2 n bits of headroom below it for the factor n"""
    return (m % (1 << bits)) << (w - (n.bit_length() - 1) - bits)


def decode(x, bits, w):
    """the top `bits` bits of a packed phase coefficient, rounded to nearest"""
    return (((x % (1 << w)) >> (w - bits - 1)) + 1 >> 1) % (1 << bits)
