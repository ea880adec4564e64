"""The plain-int model of include/cntt_manylut.h on top of tests/native_cbs_model.py: the coarse modulus switch, the interleaved table, the
extraction of several indices, the many-LUT bootstrap, the circuit bootstrap with one rotation per input bit built from
native_cbs_model's functions, and the header's workspace formula.  tests/test_native_manylut_model.py checks these against the header's
statements.  No GPU needed; not a test module."""
import os

from native_cbs_model import H, model_blind_rotate, model_keyswitch_rows, selector_from_rows, shape
from native_cmux_model import up

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_manylut.h")


def ms_coarse(x, w, logn, t):
    """ms_t(x) = 2^t ((((x >> (w - (logn - t) - 2)) + 1) >> 1) mod 2n'), n' = n / 2^t"""
    return ((((x >> (w - (logn - t) - 2)) + 1) >> 1) % (2 << (logn - t))) << t


def top32_ms_coarse(x, w, logn, t):
    """the kernel's form: the same rule on the top 32 bits of the word alone"""
    top = x >> (w - 32)
    return ((((top >> (32 - (logn - t) - 2)) + 1) >> 1) & ((2 << (logn - t)) - 1)) << t


def model_modswitch_coarse(lwe, L, batch, w, logn, t, add=0):
    """lwe: batch * (L + 1) ints -> rot_t, (L + 1) * batch ints, transposed, body row negated; add: added to the body first (wrapping)"""
    two_n = 2 << logn
    out = [0] * ((L + 1) * batch)
    for b in range(batch):
        for i in range(L + 1):
            x = lwe[b * (L + 1) + i]
            if i == L:
                x = (x + add) % (1 << w)
            m = ms_coarse(x, w, logn, t)
            out[i * batch + b] = (two_n - m) % two_n if i == L else m
    return out


def interleave(functions, n, t):
    """functions: 2^t lists of n' = n / 2^t ints -> the body polynomial v with v[m 2^t + h] = functions[h][m]"""
    return [functions[c & ((1 << t) - 1)][c >> t] for c in range(n)]


def model_extract(glwe, h, w):
    """sample extraction at the index h (cntt_pbs.h): k + 1 lists of n ints -> k n + 1 ints"""
    n, M, k = len(glwe[0]), 1 << w, len(glwe) - 1
    out = []
    for p in range(k):
        out += [glwe[p][h - j] if j <= h else (-glwe[p][h - j + n]) % M for j in range(n)]
    return out + [glwe[k][h]]


def model_extract_many(glwe, count, w):
    """glwe: k + 1 lists of n ints -> count * (k n + 1) ints, row h the extraction at the index h"""
    return [x for h in range(count) for x in model_extract(glwe, h, w)]


def model_bootstrap_manylut(lwe, lut, bsk_rows, w, L, k, n, beta, ell, t, count):
    """one element: the coarse switch, the unchanged blind rotation, the extraction of the indices 0 .. count - 1"""
    rot = model_modswitch_coarse(lwe, L, 1, w, n.bit_length() - 1, t)
    return model_extract_many(model_blind_rotate(lut, rot, bsk_rows, w, k, n, beta, ell), count, w)


def cbs_table(w, k, n, cbs_beta, Lc, t):
    """the shared table of the circuit bootstrap: zero masks, body v[m 2^t + h] = 2^w - H_(h+1) for h < Lc and 0 above"""
    mask = (1 << t) - 1
    body = [(1 << w) - H(w, cbs_beta, (c & mask) + 1) if (c & mask) < Lc else 0 for c in range(n)]
    return [[0] * n for _ in range(k)] + [body]


def model_u_manylut(lwe, bsk_rows, w, L, k, n, pbs_beta, pbs_ell, cbs_beta, Lc, t):
    """steps 1 and 2 for one element: [u[l] for l = 1 .. Lc], each Lin + 1 words, from ONE blind rotation"""
    M = 1 << w
    x = list(lwe)
    x[L] = (x[L] + (1 << (w - 2))) % M
    rows = model_bootstrap_manylut(x, cbs_table(w, k, n, cbs_beta, Lc, t), bsk_rows, w, L, k, n, pbs_beta, pbs_ell, t, Lc)
    lin = k * n
    us = []
    for l in range(1, Lc + 1):
        u = rows[(l - 1) * (lin + 1):l * (lin + 1)]
        u[lin] = (u[lin] + H(w, cbs_beta, l)) % M
        us.append(u)
    return us


def model_circuit_bootstrap_manylut(lwe, bsk_rows, F, w, L, k, n, pbs_beta, pbs_ell, ks_beta, Lk, cbs_beta, Lc, t):
    """one element: the selector words of steps 1 - 3 (coefficient domain), which native_cmux_model.model_tree takes"""
    us = model_u_manylut(lwe, bsk_rows, w, L, k, n, pbs_beta, pbs_ell, cbs_beta, Lc, t)
    return selector_from_rows([model_keyswitch_rows(u, F, w, k, n, ks_beta, Lk) for u in us], k, n)


def cbs_manylut_workspace_bytes(n, word, L, k, pbs_levels, Lk, Lc, batch):
    E, R = batch * Lc, (k * n + 1) * Lk
    S = shape(n, word, k, R, E)[3]
    ct = (k + 1) * n * word
    return (up((L + 1) * batch * 4) + up(ct) + up(batch * ct * pbs_levels) + up(batch * ct) + up(E * R * 4) + up(S * (k + 1) * E * ct)
            + up((k + 1) * E * ct))
