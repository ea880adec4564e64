"""Seeded random sweep over the external-product, gadget, bootstrap and keyswitch calls (include/cntt_ext.h, cntt_gadget.h, cntt_pbs.h,
cntt_keyswitch.h, cntt_pack.h, cntt_prime_pbs.h) on the MI355X.  The cases come from tests/random_cases.py, whose first SEEDS seeds are
shown to reach the stated corners in tests/test_random_cases.py.  Bit-exact throughout: the reference is the plain-integer model of
the file that owns it or the CPU oracle, and where a library call serves as a second reference (the per-iteration public calls of the
blind rotations, the composition of the fused gadget call) the integer model is compared as well.  check(oracle, family, seed) runs
one case; tools/soak_random.py calls it for more seeds."""
import random

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import random_cases as rc
import test_gpu_native_external_product as tex
import test_gpu_native_gadget as tg
import test_gpu_native_keyswitch as tks
import test_gpu_native_pack as tpk
import test_gpu_native_pbs as tnp
import test_gpu_prime_pbs as tpp
import test_prime_pbs_model as pm
from concrete_ntt_amd import prime32, prime64

pytestmark = pytest.mark.gpu

ORACLE_WORDS = 1 << 19      # coefficients of oracle products one case replays through Python lists, about; fewer elements beyond that
MODEL_ELEMENTS = 6          # batch elements the slower integer models replay when the batch is larger: first, last, middle, random ones


def sample_elements(rng, batch, count=MODEL_ELEMENTS):
    if batch <= count:
        return list(range(batch))
    if count < 3:
        return sorted({0, batch - 1})[:count]
    return sorted({0, batch // 2, batch - 1} | {rng.randrange(batch) for _ in range(count - 3)})


def first_bad(got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return None if bad.size == 0 else (int(bad[0]), int(bad.size))


def chunks(flat, n):
    return [flat[i * n:(i + 1) * n] for i in range(len(flat) // n)]


# -- ext ------------------------------------------------------------------------------------------------------------------------------------
def check_ext(oracle, c):
    torch = tex._torch()
    kind, n, batch, J, O = c["kind"], c["n"], c["batch"], c["nterms"], c["nout"]
    plan = tex.KINDS[kind].try_new(n)
    assert plan is not None and J <= plan.max_terms(), c
    w, M = 8 * plan.WORD, 1 << (8 * plan.WORD)
    rng = random.Random(c["data_seed"])
    terms_i = rc.special_words(rng, w, batch * J * n)
    key_i = [rng.randrange(2) for _ in range(J * O * n)] if plan.BINARY else rc.special_words(rng, w, J * O * n)
    prior_i = rc.special_words(rng, w, batch * O * n)
    terms, keyw, prior = tg.to_array(plan, terms_i), tg.to_array(plan, key_i), tg.to_array(plan, prior_i)
    kr = tex.key_residues(torch, plan, keyw, J * O)
    want = tex.expected(oracle, kind, plan, terms, keyw, batch, J, O)
    if c["accumulate"]:
        want = tex.wadd(prior, want, plan.WORD)
    with cntt.debug_switches(native_ext=c["switch"]):
        got = tex.run_ext(torch, plan, prior, terms, kr, J, O, c["accumulate"])
    assert first_bad(got, want) is None, ("oracle", first_bad(got, want), c)
    if n <= rc.SCHOOLBOOK_MAX_N:
        T, K, G = chunks(terms_i, n), chunks(key_i, n), chunks(tg.to_ints(plan, got), n)
        for b in sample_elements(rng, batch, 3):
            for o in range(O):
                acc = prior_i[(b * O + o) * n:(b * O + o + 1) * n] if c["accumulate"] else [0] * n
                for j in range(J):
                    acc = [(x + y) % M for x, y in zip(acc, pm.negacyclic(T[b * J + j], K[j * O + o], M))]
                assert G[b * O + o] == acc, ("schoolbook", b, o, c)


# -- gadget ---------------------------------------------------------------------------------------------------------------------------------
def check_gadget(oracle, c):
    torch = tg._torch()
    kind, n, batch, npolys, beta, ell, nout, mode = (c[x] for x in ("kind", "n", "batch", "npolys", "base_log", "levels", "nout", "mode"))
    plan = tg.KINDS[kind].try_new(n)
    assert plan is not None and npolys * ell <= plan.max_terms(), c
    w, M = tg.wbits(plan), 1 << tg.wbits(plan)
    per = n * (2 if plan.WORD == 16 else 1)
    rng, nrng = random.Random(c["data_seed"]), np.random.default_rng(c["data_seed"])
    words = tg.sample_words(nrng, w, beta, ell, batch * npolys * n)          # the rounding ties of this (base_log, levels) among them
    polys = [[words[(b * npolys + q) * n:(b * npolys + q + 1) * n] for q in range(npolys)] for b in range(batch)]
    rot = c["rot"]
    polys_t, rot_t = tg.dev(torch, tg.to_array(plan, tg.flat(polys))), tg.dev(torch, np.array(rot, dtype=np.uint32))
    # the decomposition call against the model, every word
    mt = tg.model_terms(polys, rot, w, beta, ell, mode)
    want = tg.to_array(plan, tg.flat(mt))
    terms = tg.dev(torch, np.zeros_like(want))
    plan.gadget_decompose_batch(terms, polys_t, beta, ell, rot=rot_t, mode=mode)
    torch.cuda.synchronize()
    assert first_bad(tg.host(terms, want.dtype), want) is None, ("terms", first_bad(tg.host(terms, want.dtype), want), c)
    # the fused call under both switch settings
    keyw = tg.key_words(nrng, plan, npolys * ell * nout)
    kr = tg.key_residues(torch, plan, keyw)
    got = {}
    for sw in (1, 0):
        with cntt.debug_switches(native_gadget=sw):
            got[sw], add_w = tg.run_fused(torch, plan, polys_t, rot_t, kr, beta, ell, nout, mode, c["addend"], batch)
    assert np.array_equal(got[1], got[0]), ("switch native_gadget 1 / 0 differ", first_bad(got[1], got[0]), c)
    # model digits -> oracle products -> sum
    for b in sample_elements(rng, batch, max(1, min(MODEL_ELEMENTS, ORACLE_WORDS // (npolys * ell * nout * n)))):
        exp = [x for o in tg.oracle_element(oracle, kind, plan, mt[b], keyw, nout) for x in o]
        if add_w is not None:
            exp = [(x + y) % M for x, y in zip(exp, tg.to_ints(plan, add_w[b * nout * per:(b + 1) * nout * per]))]
        assert tg.to_ints(plan, got[1][b * nout * per:(b + 1) * nout * per]) == exp, ("model digits x oracle, element", b, c)
    # the elements not replayed above: the terms just checked word for word, through cntt_native_external_product_batch
    ext = tg.dev(torch, np.zeros(batch * nout * per, dtype=plan.word_dtype))
    plan.external_product_batch(ext, terms, kr, npolys * ell, nout)
    torch.cuda.synchronize()
    comp = tg.host(ext, plan.word_dtype)
    if add_w is not None:
        comp = tg.wadd(plan, comp, add_w)
    assert first_bad(got[1], comp) is None, ("composition", first_bad(got[1], comp), c)


# -- nativepbs ------------------------------------------------------------------------------------------------------------------------------
def native_iteration(ref, plan, acc, a, keyp, w, beta, ell):
    """acc + sum_j digit_j(X^a acc - acc) (*) key_j mod 2^w: the model's digits, the oracle's products"""
    M, n, npolys = 1 << w, len(acc[0]), len(acc)
    terms = tnp.model_terms_element(acc, a, w, beta, ell)
    new = []
    for o in range(npolys):
        add = [0] * n
        for j, t in enumerate(terms):
            prod = np.zeros_like(tnp.to_array(plan, t))
            ref.negacyclic_polymul(prod, tnp.to_array(plan, t), tnp.to_array(plan, keyp[j * npolys + o]))
            add = [(x + y) % M for x, y in zip(add, tnp.to_ints(plan, prod))]
        new.append([(x + y) % M for x, y in zip(acc[o], add)])
    return new


def check_nativepbs(oracle, c):
    torch = tnp._torch()
    kind, w, n, k, L, beta, ell, batch, per_element = (c[x] for x in ("kind", "w", "n", "k", "L", "base_log", "levels", "batch", "per_element"))
    plan = tnp.KINDS[kind].try_new(n)
    assert plan is not None and (k + 1) * ell <= plan.max_terms(), c
    logn, npolys, mult = n.bit_length() - 1, k + 1, 2 if plan.WORD == 16 else 1
    rng, nrng = random.Random(c["data_seed"]), np.random.default_rng(c["data_seed"])
    # modulus switch
    lwe = tnp.modswitch_words(nrng, w, logn, batch * (L + 1))
    rot = tnp.model_modswitch(lwe, L, batch, w, logn)
    lwe_t = tnp.dev(torch, tnp.to_array(plan, lwe))
    rot_t = torch.full(((L + 1) * batch,), -1, dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    torch.cuda.synchronize()
    assert [int(x) for x in tnp.host(rot_t, np.uint32)] == rot, ("modswitch", c)
    # sample extraction
    eb = min(batch, 3)
    ga = tnp.random_words(nrng, plan, eb * npolys * n)
    gi = chunks(tnp.to_ints(plan, ga), n)
    want = tnp.to_array(plan, [x for b in range(eb) for x in tnp.model_extract(gi[b * npolys:(b + 1) * npolys], c["index"], w)])
    out = tnp.dev(torch, np.zeros_like(want))
    plan.sample_extract_batch(out, tnp.dev(torch, ga), k, c["index"])
    torch.cuda.synchronize()
    assert np.array_equal(tnp.host(out, want.dtype), want), ("extract", c)
    # blind rotation with the exponents just checked
    lut_a = tnp.random_words(nrng, plan, (batch if per_element else 1) * npolys * n)
    key_a = tnp.random_key_words(nrng, plan, L * npolys * ell * npolys)
    res_t = torch.int64 if plan.RES == 8 else torch.int32
    kr = tnp.key_planes(torch, plan, key_a) if L else [torch.empty(0, dtype=res_t, device="cuda") for _ in range(plan.NPRIMES)]
    lut_t = tnp.dev(torch, lut_a)
    acc_t = tnp.dev(torch, tnp.random_words(nrng, plan, batch * npolys * n))          # written only: the prior content must not matter
    ws = tnp.workspace(torch, plan, L, k, ell, batch) if c["workspace"] else None
    plan.blind_rotate_batch(acc_t, lut_t, rot_t, kr, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    inplace, pingpong = tnp.per_iteration_references(torch, plan, lut_t, per_element, rot_t, kr, L, k, beta, ell, batch)
    assert torch.equal(acc_t, inplace) and torch.equal(acc_t, pingpong), ("blind rotation against the per-iteration calls", c)
    got = chunks(tnp.to_ints(plan, tnp.host(acc_t, plan.word_dtype)), n)
    ref = oracle.Native(kind, n)
    lut_p, keyp = chunks(tnp.to_ints(plan, lut_a), n), chunks(tnp.to_ints(plan, key_a), n)
    slice_ = npolys * ell * npolys
    elements = sample_elements(rng, batch, max(1, min(MODEL_ELEMENTS, ORACLE_WORDS // max(1, L * slice_ * n))))
    if n <= rc.SCHOOLBOOK_MAX_N or L == 0:
        for b in elements:          # the whole iteration on integers
            lb = lut_p[b * npolys:(b + 1) * npolys] if per_element else lut_p
            acc = [tnp.source(f, rot[L * batch + b], w, "rotate") for f in lb]
            for i in range(L):
                acc = native_iteration(ref, plan, acc, rot[i * batch + b], keyp[i * slice_:(i + 1) * slice_], w, beta, ell)
            assert got[b * npolys:(b + 1) * npolys] == acc, ("blind rotation against the integer model, element", b, c)
    else:                           # the last iteration on integers, from the accumulator the first L - 1 leave
        prev_t = torch.zeros_like(acc_t)
        rot_prev = torch.cat([rot_t[:(L - 1) * batch], rot_t[L * batch:]])
        plan.blind_rotate_batch(prev_t, lut_t, rot_prev, [p[:(L - 1) * slice_ * n] for p in kr], L - 1, k, beta, ell, lut_per_element=per_element)
        torch.cuda.synchronize()
        prev = chunks(tnp.to_ints(plan, tnp.host(prev_t, plan.word_dtype)), n)
        for b in elements[:3]:
            acc = native_iteration(ref, plan, prev[b * npolys:(b + 1) * npolys], rot[(L - 1) * batch + b], keyp[(L - 1) * slice_:L * slice_], w, beta, ell)
            assert got[b * npolys:(b + 1) * npolys] == acc, ("last iteration against the integer model, element", b, c)
    # bootstrap: the three steps in one call
    want = tnp.to_array(plan, [x for b in range(batch) for x in tnp.model_extract(got[b * npolys:(b + 1) * npolys], 0, w)])
    boot = tnp.dev(torch, np.full(batch * (k * n + 1) * mult, 0xA5, dtype=plan.word_dtype))
    ws = tnp.workspace(torch, plan, L, k, ell, batch) if c["workspace"] else None
    plan.bootstrap_batch(boot, lwe_t, lut_t, kr, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    assert np.array_equal(tnp.host(boot, plan.word_dtype), want), ("bootstrap", c)


# -- keyswitch ------------------------------------------------------------------------------------------------------------------------------
def check_keyswitch(oracle, c):
    torch = tks._torch()
    w, beta, ell, lin, lout, pad, batch = (c[x] for x in ("w", "base_log", "levels", "lin", "lout", "pad", "batch"))
    plan = tks.WORDS[w].try_new(32)          # ntt_size plays no part
    rng = random.Random(c["data_seed"])
    stride = lout + 1 + pad
    lwe = rc.special_words(rng, w, batch * (lin + 1))
    ksk = [rng.getrandbits(w) for _ in range(tks.key_len(lin, ell, lout, stride))]
    want = tks.model_keyswitch_batch(lwe, ksk, lin, lout, stride, w, beta, ell, batch)
    got = tks.run_keyswitch(torch, plan, "device", lwe, ksk, lin, lout, stride, beta, ell, batch)          # onto a poisoned buffer
    bad = [i for i, (x, y) in enumerate(zip(got, want)) if x != y]
    assert not bad, ("first bad word", bad[0], hex(got[bad[0]]), hex(want[bad[0]]), len(bad), c)
    if pad and lin:
        other = list(ksk)
        for r in range(lin * ell - 1):
            for col in range(lout + 1, stride):
                other[r * stride + col] ^= (1 << w) - 1
        assert tks.run_keyswitch(torch, plan, "device", lwe, other, lin, lout, stride, beta, ell, batch) == got, ("padding read", c)


# -- pack -----------------------------------------------------------------------------------------------------------------------------------
def check_pack(oracle, c):
    torch = tpk._torch()
    w, n, k, m, lin, beta, ell, batch = (c[x] for x in ("w", "n", "k", "m", "lin", "base_log", "levels", "batch"))
    plan = tpk.WORDS[w].try_new(n)
    assert plan is not None and ell <= plan.max_terms() and c["C"] == tpk.C(plan, ell), c
    rng = random.Random(c["data_seed"])
    lwe = rc.special_words(rng, w, batch * m * (lin + 1))
    key = [rng.getrandbits(w) for _ in range(lin * ell * (k + 1) * n)]
    want = tpk.model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch, dtype={32: np.uint32, 64: np.uint64, 128: object}[w])
    got = tpk.run_pack(torch, plan, "device", lwe, key, lin, m, k, beta, ell, batch, with_ws=c["workspace"])
    assert got == want, ("first bad word", tpk.first_difference(got, want), c)


# -- primepbs -------------------------------------------------------------------------------------------------------------------------------
_applies = {}


def model_applies(oracle, p, bits):
    if (p, bits) not in _applies:
        _applies[(p, bits)] = rc.model_applies(oracle, p, bits)
    return _applies[(p, bits)]


def prime_words(rng, p, beta, ell, count, dtype):
    edge = pm.edge_words(p, beta, ell)
    return np.array([edge[rng.randrange(len(edge))] if rng.randrange(4) == 0 else rng.randrange(p) for _ in range(count)], dtype=dtype)


def check_primepbs(oracle, c):
    torch = tpp._torch()
    bits, p, n, k, L, beta, ell, batch, per_element = (c[x] for x in ("bits", "p", "n", "k", "L", "base_log", "levels", "batch", "per_element"))
    plan = (prime64 if bits == 64 else prime32).Plan.try_new(n, p)
    assert plan is not None, c
    dtype, tt = (np.uint64, torch.int64) if bits == 64 else (np.uint32, torch.int32)
    logn, npolys = n.bit_length() - 1, k + 1
    rng, nrng = random.Random(c["data_seed"]), np.random.default_rng(c["data_seed"])
    # decomposition
    q, mode = c["npolys"], c["mode"]
    polys = prime_words(rng, p, beta, ell, batch * q * n, dtype)
    drot = rc.rot_values(rng, n, batch)
    terms = torch.zeros(polys.size * ell, dtype=tt, device="cuda")
    plan.gadget_decompose_batch(terms, tpp.dev(torch, polys), beta, ell, rot=tpp.dev(torch, np.array(drot, dtype=np.uint32)), mode=mode)
    torch.cuda.synchronize()
    have, f = tpp.host(terms, dtype), polys.tolist()
    for b in sample_elements(rng, batch):
        elem = [f[(b * q + j) * n:(b * q + j + 1) * n] for j in range(q)]
        want = [x for t in pm.model_terms_element(elem, drot[b], p, beta, ell, mode) for x in t]
        assert [int(x) for x in have[b * q * ell * n:(b + 1) * q * ell * n]] == want, ("decomposition, element", b, c)
    # modulus switch
    special = pm.modswitch_words(p, logn, nrng)
    lwe = [special[rng.randrange(len(special))] if rng.randrange(2) else rng.randrange(p) for _ in range(batch * (L + 1))]
    rot = pm.model_modswitch(lwe, L, batch, p, logn)
    lwe_t = tpp.dev(torch, np.array(lwe, dtype=dtype))
    rot_t = torch.full(((L + 1) * batch,), -1, dtype=torch.int32, device="cuda")
    plan.lwe_modswitch_batch(rot_t, lwe_t, L)
    torch.cuda.synchronize()
    assert [int(x) for x in tpp.host(rot_t, np.uint32)] == rot, ("modswitch", c)
    # sample extraction
    eb = min(batch, 3)
    glwe = prime_words(rng, p, beta, ell, eb * npolys * n, dtype)
    g = chunks(glwe.tolist(), n)
    want = [x for b in range(eb) for x in pm.model_extract(g[b * npolys:(b + 1) * npolys], c["index"], p)]
    out = torch.zeros(eb * (k * n + 1), dtype=tt, device="cuda")
    plan.sample_extract_batch(out, tpp.dev(torch, glwe), k, c["index"])
    torch.cuda.synchronize()
    assert [int(x) for x in tpp.host(out, dtype)] == want, ("extract", c)
    # blind rotation with the exponents just checked
    exact = n <= rc.SCHOOLBOOK_MAX_N and model_applies(oracle, p, bits)
    lut_a = prime_words(rng, p, beta, ell, (batch if per_element else 1) * npolys * n, dtype)
    key_a = nrng.integers(0, p, size=L * npolys * ell * npolys * n, dtype=np.uint64).astype(dtype)
    lut_t = tpp.dev(torch, lut_a)
    bsk = tpp.key_ntt(torch, plan, key_a) if L else torch.empty(0, dtype=tt, device="cuda")          # n^-1 fwd(key): the header's convention
    acc_t = tpp.dev(torch, prime_words(rng, p, beta, ell, batch * npolys * n, dtype))                  # written only
    ws = tpp.workspace(torch, plan, L, k, ell, batch) if c["workspace"] else None
    plan.blind_rotate_batch(acc_t, lut_t, rot_t, bsk, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    want_t = tpp.per_iteration_reference(torch, plan, p, lut_t, per_element, rot_t, bsk, L, k, beta, ell, batch)
    assert torch.equal(acc_t, want_t), ("blind rotation against the per-iteration calls", c)
    got = chunks(tpp.host(acc_t, dtype).tolist(), n)
    slice_ = npolys * ell * npolys
    if exact or L == 0:
        lut_p, keyp = chunks(lut_a.tolist(), n), chunks(key_a.tolist(), n)
        budget = max(1, min(MODEL_ELEMENTS, 3 * 10 ** 6 // max(1, L * slice_ * n * n)))
        for b in sample_elements(rng, batch, budget) if budget >= 3 else [rng.randrange(batch)]:
            lb = lut_p[b * npolys:(b + 1) * npolys] if per_element else lut_p
            acc = [pm.source(f, rot[L * batch + b], p, "rotate") for f in lb]
            for i in range(L):
                tms = pm.model_terms_element(acc, rot[i * batch + b], p, beta, ell)
                new = []
                for o in range(npolys):
                    add = [0] * n
                    for j, t in enumerate(tms):
                        add = [(x + y) % p for x, y in zip(add, pm.negacyclic(t, keyp[i * slice_ + j * npolys + o], p))]
                    new.append([(x + y) % p for x, y in zip(acc[o], add)])
                acc = new
            assert got[b * npolys:(b + 1) * npolys] == acc, ("blind rotation against the big-integer model, element", b, c)
    else:
        # the last iteration without the library: the model's digits of the accumulator the first L - 1 iterations leave, and the CPU
        # oracle's fwd / mul_accumulate / inv on a key it transformed itself (it restates the reference, wraps included)
        prev_t = torch.zeros_like(acc_t)
        rot_prev = torch.cat([rot_t[:(L - 1) * batch], rot_t[L * batch:]])
        plan.blind_rotate_batch(prev_t, lut_t, rot_prev, bsk[:(L - 1) * slice_ * n], L - 1, k, beta, ell, lut_per_element=per_element)
        torch.cuda.synchronize()
        prev = chunks(tpp.host(prev_t, dtype).tolist(), n)
        ref = oracle.Plan.try_new(n, p, bits)
        keyn = []
        for j in range((L - 1) * slice_, L * slice_):
            y = key_a[j * n:(j + 1) * n].copy()
            ref.fwd(y)
            ref.normalize(y)
            keyn.append(y)
        for b in sample_elements(rng, batch, 3 if n * slice_ <= ORACLE_WORDS else 1):
            acc = prev[b * npolys:(b + 1) * npolys]
            if any(x >= p for f in acc for x in f):
                continue          # a wrap left words above p: the digits of such words are unspecified (cntt_prime_pbs.h)
            tms = pm.model_terms_element(acc, rot[(L - 1) * batch + b], p, beta, ell)
            for o in range(npolys):
                add = np.zeros(n, dtype=dtype)
                for j, t in enumerate(tms):
                    x = np.array(t, dtype=dtype)
                    ref.fwd(x)
                    ref.mul_accumulate(add, x, keyn[j * npolys + o])
                ref.inv(add)
                if int(add.max()) >= p:
                    continue      # likewise: the wrap took inv outside its input contract
                assert got[b * npolys + o] == [(u + int(v)) % p for u, v in zip(acc[o], add)], ("last iteration against the oracle, element", b, "output", o, c)
    # bootstrap: the three steps in one call
    want = [x for b in range(batch) for x in pm.model_extract(got[b * npolys:(b + 1) * npolys], 0, p)]
    boot = torch.full((batch * (k * n + 1),), -1, dtype=tt, device="cuda")
    ws = tpp.workspace(torch, plan, L, k, ell, batch) if c["workspace"] else None
    plan.bootstrap_batch(boot, lwe_t, lut_t, bsk, L, k, beta, ell, workspace=ws, lut_per_element=per_element)
    torch.cuda.synchronize()
    assert [int(x) for x in tpp.host(boot, dtype)] == want, ("bootstrap", c)


CHECKS = {"ext": check_ext, "gadget": check_gadget, "nativepbs": check_nativepbs, "keyswitch": check_keyswitch, "pack": check_pack,
          "primepbs": check_primepbs}


def check(oracle, family, seed):
    CHECKS[family](oracle, rc.case(family, seed))


@pytest.mark.parametrize("seed", range(rc.SEEDS))
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_gpu_random_fhe(oracle, family, seed):
    check(oracle, family, seed)
