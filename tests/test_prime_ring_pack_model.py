"""The model of tests/prime_ring_pack_model.py against its specification (include/cntt_prime_ring_pack.h), on the CPU: the embedding
inverts sample extraction at index 0; the packing on noise-free keys with no rounding leaves n * phase(lwe_j) at coefficient j n / M and 0
elsewhere, for every M; the numpy forms the GPU tests use equal the plain-int ones; and encrypted 3-bit messages survive a packing with
noisy keys at the parameters of the GPU test, which confirms its noise margin before any GPU run.  No GPU."""
import random

import numpy as np
import pytest

from prime_automorphism_model import automorphism_key, autom_gather, phase, trace_keys
from prime_ring_pack_model import (embed, embed_np, lwe_encrypt, merge_parts, merge_parts_np, model_merge, model_ring_pack, prefill_np, rotate_np,
                                   stage_params)
from test_prime_automorphism_model import binary_key
from test_prime_pbs_model import P30, P62, PM64, lift, model_extract, source, wbits


@pytest.mark.parametrize("p", [PM64, P30])
@pytest.mark.parametrize("k", [0, 1, 2])
def test_embedding_inverts_sample_extraction_at_index_0(p, k):
    n = 16
    rng = random.Random("ringpack/embed/%d/%d" % (p, k))
    lwe = [rng.randrange(p) for _ in range(k * n + 1)]
    lwe[1:4] = [0, p - 1, 0][:min(3, k * n)]                              # a zero stays zero under the sign
    g = embed(lwe, p, k, n)
    assert len(g) == (k + 1) * n and g[k * n + 1:] == [0] * (n - 1)
    assert model_extract([g[q * n:(q + 1) * n] for q in range(k + 1)], 0, p) == lwe
    dtype = np.uint64 if p >= 1 << 32 else np.uint32
    assert embed_np(np.array([lwe, lwe], dtype=dtype), p, k, n).tolist() == [g, g]
    # coefficient 0 of the phase of the embedding is the phase of the LWE ciphertext under the flattened key
    S = binary_key(rng, k, n)
    flat = [x for row in S for x in row]
    assert phase(g, S, p)[0] == (lwe[k * n] - sum(a * s for a, s in zip(lwe, flat))) % p


def test_stage_parameters_are_the_trace_keys():
    """stage s uses shift n / 2^s and t = 2^s + 1 = t_r with r = log2 n - s"""
    n = 16
    assert stage_params(n, 1) == [] and stage_params(n, 2) == [(1, 8, 3, 3)]
    assert stage_params(n, 16) == [(8, 8, 3, 3), (4, 4, 5, 2), (2, 2, 9, 1), (1, 1, 17, 0)]
    for h, shift, t, r in stage_params(1024, 1024):
        assert t == (1024 >> r) + 1 and shift * (t - 1) == 1024


@pytest.mark.parametrize("p,beta,ell", [(PM64, 16, 4), (P30, 10, 3)])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("m", [1, 2, 4, 16])
def test_packing_on_noise_free_keys_with_no_rounding(p, beta, ell, k, m):
    """base_log * levels = W: coefficient j n / M of the phase is exactly n * phase(lwe_j), every other coefficient is 0, for every M"""
    n = 16
    assert beta * ell == wbits(p)
    rng = random.Random("ringpack/pack/%d/%d/%d" % (p, k, m))
    S = binary_key(rng, k, n)
    keys = trace_keys(rng, p, S, 4, n, beta, ell)
    phases = [rng.randrange(p) for _ in range(m)]
    lwes = [lwe_encrypt(rng, p, S, x, k, n) for x in phases]
    out = model_ring_pack(lwes, keys, p, m, k, n, beta, ell)
    assert all(0 <= v < p for v in out)
    want = [0] * n
    for j, x in enumerate(phases):
        want[j * (n // m)] = n * x % p
    assert phase(out, S, p) == want, (k, m)


@pytest.mark.parametrize("p", [P62, P30])
def test_merge_phase_identity_and_numpy_forms(p):
    """phase(merge) = phase(E) + X^shift phase(O) + sigma_t(phase(E) - X^shift phase(O)) on a noise-free key with no rounding needed to
    state it: the digits reconstruct exactly when s = 0, so take W = base_log * levels via one level of W bits"""
    n, k = 16, 1
    W = wbits(p)
    rng = random.Random("ringpack/merge/%d" % p)
    S = binary_key(rng, k, n)
    dtype = np.uint64 if p >= 1 << 32 else np.uint32
    for shift, t in ((0, 3), (1, 5), (n // 2, 3), (n - 1, 2 * n - 1), (n, n + 1), (2 * n - 1, 9)):
        E = [rng.randrange(p) for _ in range((k + 1) * n)]
        O = [rng.randrange(p) for _ in range((k + 1) * n)]
        E[2], O[5], E[7] = 0, 0, p - 1
        key = automorphism_key(rng, p, S, t, n, W, 1)
        out = model_merge(E, O, key, p, shift, t, k, n, W, 1)
        pe, po = phase(E, S, p), source(phase(O, S, p), shift, p, "rotate")
        rot = autom_gather([(x - y) % p for x, y in zip(pe, po)], t, p)
        assert phase(out, S, p) == [(x + y + z) % p for x, y, z in zip(pe, po, rot)], (shift, t)
        a, d = merge_parts(E, O, shift, p, k, n)
        an, dn = (x.reshape(-1) for x in merge_parts_np(np.array(E, dtype=dtype).reshape(k + 1, n), np.array(O, dtype=dtype).reshape(k + 1, n), shift, p))
        assert an.tolist() == a and dn.tolist() == d
        assert rotate_np(np.array(O[:n], dtype=dtype), shift, p).tolist() == source(O[:n], shift, p, "rotate")
        pre = prefill_np(an, dn, t, p, k, n).tolist()
        assert pre[:k * n] == a[:k * n] and pre[k * n:] == [(x + y) % p for x, y in zip(a[k * n:], autom_gather(d[k * n:], t, p))]


def test_encrypted_messages_survive_a_packing_with_noisy_keys():
    """The parameters of the GPU test at a size the plain-int model affords: PM64, k = 1, binary key, M = 16, 3-bit messages at steps of
    floor(p / 8), LWE noise below 2^30, key noise |e| < 2^10, base_log 16, levels 4 (base_log * levels = 64), inputs scaled by n^-1.  n is 32
    here and 256 on the GPU.  Error bound: the packing is linear in the phase, so message j comes out with its own LWE noise; each of the
    log2 n keyswitches adds at most k n levels (B / 2) 2^10 per coefficient and every later step at most doubles what is there, so the sum
    stays below n log2 n k n levels (B / 2) 2^10 -- 2^44 at n = 256 with B = 2^16, far below the floor(p / 16) ~ 2^60 that half a message
    step allows."""
    p, n, k, beta, ell, m = PM64, 32, 1, 16, 4, 16
    rng = random.Random("ringpack/messages")
    S = binary_key(rng, k, n)
    keys = trace_keys(rng, p, S, 5, n, beta, ell, noise=(1 << 10) - 1)
    msgs = [rng.randrange(8) for _ in range(m)]
    n_inv = pow(n, -1, p)
    lwes = []
    for x in msgs:
        ct = lwe_encrypt(rng, p, S, (x * (p // 8) + rng.randint(-(1 << 30) + 1, (1 << 30) - 1)) % p, k, n)
        lwes.append([w * n_inv % p for w in ct])
    out = model_ring_pack(lwes, keys, p, m, k, n, beta, ell)
    ph = phase(out, S, p)
    dec = [(8 * x + p // 2) // p % 8 for x in ph]
    want = [0] * n
    for j, x in enumerate(msgs):
        want[j * (n // m)] = x
    assert dec == want and any(msgs)
    bound = n * 5 * k * n * ell * (1 << (beta - 1)) * (1 << 10) + (1 << 30)
    assert max(abs(lift((x - w * (p // 8)) % p, p)) for x, w in zip(ph, want)) < bound < 1 << 60
