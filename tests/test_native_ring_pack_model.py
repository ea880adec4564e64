"""The plain-int model of include/cntt_ring_pack.h (tests/native_ring_pack_model.py) against itself and against the header's statements:
the embedding inverts sample extraction and keeps the phase, a merge node is its formula and its phase statement, the pack is embed +
merges + trace, and on noise-free keys with base_log * levels = w coefficient j n / M of the packed phase is n * phase_j mod 2^w with every
other coefficient 0 -- the plaintext algebra checked on the CPU before any kernel, for w = 32 / 64 / 128 -- and the headroom encoding
decodes.  These pin the convention; they do not touch the library.  No GPU needed."""
import random

import pytest

from native_automorphism_model import autom_gather, automorphism_key, model_autoks, model_trace, phase, trace_keys
from native_ring_pack_model import decode, embed, encode, lwe_phase, merge, ring_pack, rotate, sample_extract0, stages

WIDTHS = [32, 64, 128]


def rnd_words(rnd, w, count):
    return [rnd.randrange(1 << w) for _ in range(count)]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_embedding_inverts_sample_extraction_and_keeps_the_phase(w, k):
    n = 16
    rnd = random.Random("embed/%d/%d" % (w, k))
    lwe = rnd_words(rnd, w, k * n + 1)
    g = embed(lwe, w, k, n)
    assert len(g) == (k + 1) * n and sample_extract0(g, w, k, n) == lwe
    assert g[k * n] == lwe[k * n] and g[k * n + 1:] == [0] * (n - 1)
    if k:
        assert g[0] == lwe[0] and g[1] == (-lwe[n - 1]) % (1 << w) and g[n - 1] == (-lwe[1]) % (1 << w)
    S = [[rnd.randrange(2) for _ in range(n)] for _ in range(k)]
    assert phase(g, S, w)[0] == lwe_phase(lwe, S, w)
    # and the other way round: extraction of a random ciphertext embeds back to its mask and its constant body coefficient
    ct = rnd_words(rnd, w, (k + 1) * n)
    back = embed(sample_extract0(ct, w, k, n), w, k, n)
    assert back[:k * n] == ct[:k * n] and back[k * n] == ct[k * n]


@pytest.mark.parametrize("w", WIDTHS)
def test_rotation_is_multiplication_by_a_monomial(w):
    n = 16
    rnd = random.Random("rot/%d" % w)
    f = rnd_words(rnd, w, n)
    assert rotate(f, 0, w) == f and rotate(f, n, w) == [(-x) % (1 << w) for x in f]
    assert rotate(rotate(f, 5, w), 2 * n - 5, w) == f
    assert rotate(f, 1, w) == [(-f[n - 1]) % (1 << w)] + f[:n - 1]


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("k", [0, 1, 2])
def test_merge_is_its_formula_and_its_phase_statement(w, k):
    """a + AutoKS_t(d) spelled out with the model of the Galois keyswitch; with a noise-free key and base_log * levels = w the phase is
    phase(E) + X^shift phase(O) + sigma_t(phase(E) - X^shift phase(O))"""
    n, beta, ell, M = 16, w // 4, 4, 1 << w
    rnd = random.Random("merge/%d/%d" % (w, k))
    S = [[rnd.randrange(2) for _ in range(n)] for _ in range(k)]
    for shift, t in ((0, 3), (1, n + 1), (n - 1, 2 * n - 1), (n, 3), (2 * n - 1, n + 1)):
        key = automorphism_key(rnd, w, S, t, n, beta, ell)
        E, O = rnd_words(rnd, w, (k + 1) * n), rnd_words(rnd, w, (k + 1) * n)
        got = merge(E, O, key, w, shift, t, k, n, beta, ell)
        rot = [v for q in range(k + 1) for v in rotate(O[q * n:(q + 1) * n], shift, w)]
        d = [(x - y) % M for x, y in zip(E, rot)]
        want = [(x + y + z) % M for x, y, z in zip(E, rot, model_autoks(d, key, w, t, k, n, beta, ell, False))]
        assert got == want
        pe, po = phase(E, S, w), rotate(phase(O, S, w), shift, w)
        sig = autom_gather([(x - y) % M for x, y in zip(pe, po)], t, w)
        assert phase(got, S, w) == [(x + y + z) % M for x, y, z in zip(pe, po, sig)], (shift, t)


def test_stages_are_those_of_the_header():
    assert stages(16, 1) == ([], 4)
    assert stages(16, 2) == ([(1, 1, 8, 3, 3)], 3)
    assert stages(16, 16) == ([(1, 8, 8, 3, 3), (2, 4, 4, 5, 2), (3, 2, 2, 9, 1), (4, 1, 1, 17, 0)], 0)
    for n in (16, 1024):
        for s, h, shift, t, r in stages(n, n)[0]:
            assert t == (n >> r) + 1 and shift == n >> s and h == n >> s      # stage s uses the trace key of round log2 n - s


@pytest.mark.parametrize("w", WIDTHS)
def test_pack_is_embed_merges_and_trace(w):
    n, k, beta, ell = 16, 1, 7, 2
    rnd = random.Random("pack-seq/%d" % w)
    S = [[rnd.randrange(2) for _ in range(n)]]
    keys = trace_keys(rnd, w, S, 4, n, beta, ell, noise=5)
    per = k * ell * (k + 1) * n
    lwes = [rnd_words(rnd, w, k * n + 1) for _ in range(4)]
    c = [embed(row, w, k, n) for row in lwes]
    c = [merge(c[0], c[2], keys[3 * per:4 * per], w, 8, 3, k, n, beta, ell), merge(c[1], c[3], keys[3 * per:4 * per], w, 8, 3, k, n, beta, ell)]
    c = merge(c[0], c[1], keys[2 * per:3 * per], w, 4, 5, k, n, beta, ell)
    assert ring_pack(lwes, keys, w, k, n, beta, ell) == model_trace(c, keys, w, 2, k, n, beta, ell)


@pytest.mark.parametrize("w,m,k", [(w, m, 1) for w in WIDTHS for m in (1, 2, 4, 16)] + [(32, 2, 2), (64, 16, 2)])
def test_layout_factor_and_junk_on_noise_free_keys(w, m, k):
    """base_log * levels = w: coefficient j n / M of the phase is n * phase_j mod 2^w and every other coefficient is 0 -- the junk
    coefficients of the embeddings are gone, for every M (k = 2 at the two ends only: the schoolbook model is slow)"""
    n, beta, ell, M = 16, w // 4, 4, 1 << w
    rnd = random.Random("pack-closed/%d/%d/%d" % (w, m, k))
    S = [[rnd.randrange(2) for _ in range(n)] for _ in range(k)]
    keys = trace_keys(rnd, w, S, 4, n, beta, ell)
    lwes = [rnd_words(rnd, w, k * n + 1) for _ in range(m)]
    ph = phase(ring_pack(lwes, keys, w, k, n, beta, ell), S, w)
    want = [0] * n
    for j, row in enumerate(lwes):
        want[j * n // m] = n * lwe_phase(row, S, w) % M
    assert ph == want


@pytest.mark.parametrize("w", WIDTHS)
def test_headroom_encoding_decodes_after_the_factor_n(w):
    """a 3-bit message at bit w - log2 n - 3 with noise below it comes out of n * phase at the top of the word"""
    n, bits = 16, 3
    rnd = random.Random("headroom/%d" % w)
    for m in range(8):
        for _ in range(4):
            e = rnd.randrange(-(1 << (w - 4 - bits - 2)) + 1, 1 << (w - 4 - bits - 2))      # n e stays below half a message step
            assert decode(n * (encode(m, bits, w, n) + e), bits, w) == m
    assert encode(5, 3, 64, 1024) == 5 << 51 and decode(5 << 61, 3, 64) == 5
    # without the headroom the factor destroys the message: the top log2 n bits are gone
    assert decode(n * (5 << (w - 3)), 3, w) != 5
    # and through the pack: noise-free keys, M = 4
    k, beta, ell, m4 = 1, w // 4, 4, [1, 7, 2, 4]
    S = [[rnd.randrange(2) for _ in range(n)]]
    keys = trace_keys(rnd, w, S, 4, n, beta, ell)
    lwes = []
    for m in m4:
        a = rnd_words(rnd, w, n)
        lwes.append(a + [(sum(x * s for x, s in zip(a, S[0])) + encode(m, bits, w, n) + rnd.randrange(-100, 101)) % (1 << w)])
    ph = phase(ring_pack(lwes, keys, w, k, n, beta, ell), S, w)
    assert [decode(ph[j * n // 4], bits, w) for j in range(4)] == m4
