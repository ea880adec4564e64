"""The plain-int model of include/cntt_prime_manylut.h on top of tests/test_prime_pbs_model.py and tests/prime_cbs_model.py: the coarse
modulus switch, the interleaved table, the extraction of several indices, the many-LUT bootstrap, the circuit bootstrap with one rotation
per input bit built from prime_cbs_model's functions, and the header's workspace formula.  tests/test_prime_manylut_model.py checks these
against the header's statements.  No GPU needed; not a test module."""
import os

from prime_automorphism_model import up
from prime_cbs_model import H, Q4, model_blind_rotate, model_keyswitch_rows, selector_from_rows, shape
from test_prime_pbs_model import model_extract

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cntt_prime_manylut.h")


def ms_coarse(x, p, logn, t):
    """ms_t(x) = 2^t (floor((2 x 2n' + p) / (2 p)) mod 2n'), n' = n / 2^t"""
    two_np = 2 << (logn - t)
    return (((2 * x * two_np + p) // (2 * p)) % two_np) << t


def bit_serial_ms_coarse(x, p, logn, t, tb):
    """the kernel's form: prime_ms with logn + 2 - t doublings on tb-bit words and the mask 2n' - 1, then << t"""
    M, r, q = 1 << tb, x, 0
    for _ in range(logn + 2 - t):
        carry = r >> (tb - 1)
        r = (r << 1) % M
        q <<= 1
        if carry or r >= p:
            r = (r - p) % M
            q |= 1
    return (((q + 1) >> 1) & ((2 << (logn - t)) - 1)) << t


def model_modswitch_coarse(lwe, L, batch, p, logn, t, q4=0):
    """lwe: batch * (L + 1) ints -> rot_t, (L + 1) * batch ints, transposed, body row negated; q4: added to the body first"""
    two_n = 2 << logn
    out = [0] * ((L + 1) * batch)
    for b in range(batch):
        for i in range(L + 1):
            x = lwe[b * (L + 1) + i]
            if i == L:
                x = (x + q4) % p
            m = ms_coarse(x, p, logn, t)
            out[i * batch + b] = (two_n - m) % two_n if i == L else m
    return out


def interleave(functions, n, t):
    """functions: 2^t lists of n' = n / 2^t ints -> the body polynomial v with v[m 2^t + h] = functions[h][m]"""
    return [functions[c & ((1 << t) - 1)][c >> t] for c in range(n)]


def model_extract_many(glwe, count, p):
    """glwe: k + 1 lists of n ints -> count * (k n + 1) ints, row h the extraction at the index h"""
    return [w for h in range(count) for w in model_extract(glwe, h, p)]


def model_bootstrap_manylut(lwe, lut, bsk_rows, p, L, k, n, beta, ell, t, count):
    """one element: the coarse switch, the unchanged blind rotation, the extraction of the indices 0 .. count - 1"""
    logn = n.bit_length() - 1
    rot = model_modswitch_coarse(lwe, L, 1, p, logn, t)
    return model_extract_many(model_blind_rotate(lut, rot, bsk_rows, p, k, n, beta, ell), count, p)


def cbs_table(p, k, n, cbs_beta, Lc, t):
    """the shared table of the circuit bootstrap: zero masks, body v[m 2^t + h] = p - H_(h+1) for h < Lc and 0 above"""
    body = [(p - H(p, cbs_beta, (c & ((1 << t) - 1)) + 1)) % p if (c & ((1 << t) - 1)) < Lc else 0 for c in range(n)]
    return [[0] * n for _ in range(k)] + [body]


def model_u_manylut(lwe, bsk_rows, p, L, k, n, pbs_beta, pbs_ell, cbs_beta, Lc, t):
    """steps 1 and 2 for one element: [u[l] for l = 1 .. Lc], each Lin + 1 words, from ONE blind rotation"""
    x = list(lwe)
    x[L] = (x[L] + Q4(p)) % p
    rows = model_bootstrap_manylut(x, cbs_table(p, k, n, cbs_beta, Lc, t), bsk_rows, p, L, k, n, pbs_beta, pbs_ell, t, Lc)
    lin = k * n
    us = []
    for l in range(1, Lc + 1):
        u = rows[(l - 1) * (lin + 1):l * (lin + 1)]
        u[lin] = (u[lin] + H(p, cbs_beta, l)) % p
        us.append(u)
    return us


def model_circuit_bootstrap_manylut(lwe, bsk_rows, F, p, L, k, n, pbs_beta, pbs_ell, ks_beta, Lk, cbs_beta, Lc, t):
    """one element; F in the coefficient domain gives the selector in the coefficient domain, as prime_cbs_model.model_circuit_bootstrap"""
    us = model_u_manylut(lwe, bsk_rows, p, L, k, n, pbs_beta, pbs_ell, cbs_beta, Lc, t)
    return selector_from_rows([model_keyswitch_rows(u, F, p, k, n, ks_beta, Lk) for u in us], k, n)


def cbs_manylut_workspace_bytes(n, word, L, k, pbs_levels, Lk, Lc, batch):
    E, R = batch * Lc, (k * n + 1) * Lk
    S = shape(n, word, k, R, E)[3]
    ct = (k + 1) * n * word
    return up((L + 1) * batch * 4) + up(ct) + up(batch * ct * pbs_levels) + up(batch * ct) + up(E * R * 4) + up(S * (k + 1) * E * ct)
