"""cntt_native_gadget_decompose_batch and cntt_native_external_product_decomposed_batch (include/cntt_gadget.h) on the MI355X,
bit-exact.  The decomposition kernel is compared with a big-integer model written here in plain Python ints (rotation, CMux
difference, rounding, signed digits, term order); the fused call with (i) decomposition kernel -> cntt_native_external_product_batch
-> word-wise add on the whole batch and (ii) on sampled elements the oracle: sum_j negacyclic_polymul(model digit j, key j) mod 2^w
with the key in coefficient form.  No tolerance anywhere."""
import zlib

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import (native32, native64, native128, native_binary32, native_binary64, native_binary128)

pytestmark = pytest.mark.gpu

KINDS = {"native32_plan32": native32.Plan32, "native64_plan32": native64.Plan32, "native128_plan32": native128.Plan32,
         "native_binary32_plan32": native_binary32.Plan32, "native_binary64_plan32": native_binary64.Plan32,
         "native_binary128_plan32": native_binary128.Plan32, "native32_plan52": native32.Plan52,
         "native64_plan52": native64.Plan52, "native_binary32_plan52": native_binary32.Plan52,
         "native_binary64_plan52": native_binary64.Plan52}
FUSED = ["native32_plan32", "native64_plan32", "native_binary32_plan32", "native_binary64_plan32"]
MODES = ["plain", "rotate", "cmux"]
STREAM_BYTES = 384 << 20   # the library's streaming threshold (host_common.hpp)


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


# -- the model: plain Python ints ------------------------------------------------------------------------------------------------
def source(f, a, w, mode):
    n, M = len(f), 1 << w
    if mode == "plain":
        return list(f)
    g = [0] * n
    for i in range(n):
        t = (i - a) % (2 * n)
        g[i] = f[t % n] if t < n else (-f[t % n]) % M
    if mode == "cmux":
        g = [(x - y) % M for x, y in zip(g, f)]
    return g


def digits(x, w, beta, ell):
    """d_1 .. d_ell, sequential rule of cntt_gadget.h."""
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


def model_terms(polys, rot, w, beta, ell, mode):
    """polys[b][p] = list of n ints -> terms[b][p * ell + l - 1] = list of n ints mod 2^w."""
    out = []
    for b, elem in enumerate(polys):
        row = []
        for f in elem:
            g = source(f, rot[b] if rot is not None else 0, w, mode)
            ds = [digits(x, w, beta, ell) for x in g]
            row.extend([[d[l] % (1 << w) for d in ds] for l in range(ell)])
        out.append(row)
    return out


# -- words <-> arrays ------------------------------------------------------------------------------------------------------------
def wbits(plan):
    return 8 * plan.WORD


def to_array(plan, ints):
    """flat list of ints mod 2^w -> numpy words (128-bit: (lo, hi) uint64 pairs)."""
    if plan.WORD == 16:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=plan.word_dtype)


def to_ints(plan, a):
    if plan.WORD == 16:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[0::2], a[1::2])]
    return [int(x) for x in a]


def flat(nested):
    return [x for b in nested for p in b for x in p]


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def wadd(plan, a, b):
    w = wbits(plan)
    return to_array(plan, [(x + y) % (1 << w) for x, y in zip(to_ints(plan, a), to_ints(plan, b))])


def sample_words(rng, w, beta, ell, count):
    """edge words, the rounding ties k 2^s + 2^(s-1), and random ones."""
    s = w - beta * ell
    ws = [0, 1, (1 << (w - 1)) - 1, 1 << (w - 1), (1 << w) - 1]
    if s:
        ws += [((k << s) + (1 << (s - 1))) % (1 << w) for k in (0, 1, 5, (1 << (beta * ell)) - 1, 1 << (beta * ell - 1))]
        ws += [((k << s) + (1 << (s - 1)) - 1) % (1 << w) for k in (0, 1, (1 << (beta * ell)) - 1)]
    out = [ws[i % len(ws)] if i % 3 == 0 else int.from_bytes(rng.bytes(w // 8), "little") for i in range(count)]
    return out


def make_polys(rng, plan, batch, npolys, beta, ell):
    n, w = plan.ntt_size(), wbits(plan)
    words = sample_words(rng, w, beta, ell, batch * npolys * n)
    return [[words[(b * npolys + p) * n:(b * npolys + p + 1) * n] for p in range(npolys)] for b in range(batch)]


def exponents(rng, n, batch):
    fixed = [0, 1, n - 1, n, n + 1, 2 * n - 1]
    return [fixed[b] if b < len(fixed) else int(rng.integers(0, 2 * n)) for b in range(batch)]


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


# -- the decomposition kernel against the model ------------------------------------------------------------------------------------
def shapes_for(w):
    out = [(w // 2, 2), (1, 3), (7, 1), (5, 3), (w, 1)]   # beta * ell == w, beta == 1, ell == 1, a rounded shape, one full-width digit
    if w == 64:
        out.append((32, 2))
    if w >= 64:
        out.append((32, 1))
    return out


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("n", [32, 1024, 4096, 32768])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_decompose_matches_model(kind, n, where):
    torch = _torch()
    plan = KINDS[kind].try_new(n)
    assert plan is not None
    w = wbits(plan)
    rng = np.random.default_rng(seed(kind, n, where))
    # ragged batches: 1, 3, and one that is not a multiple of what a workgroup of the kernel covers (256 threads x 16 bytes)
    batches = [1, 3, 7] if n <= 1024 else [3] if n <= 4096 else [1]
    shapes = shapes_for(w) if n <= 1024 else shapes_for(w)[:2] + shapes_for(w)[-1:]
    if where == "host":
        batches, shapes = batches[-1:], shapes[:3]
    for batch in batches:
        for si, (beta, ell) in enumerate(shapes):
            mode = MODES[(si + batch) % 3] if n > 32 else None
            for mode in ([mode] if mode else MODES):
                npolys = 1 + (si + batch) % 2 if n <= 4096 else 1
                polys = make_polys(rng, plan, batch, npolys, beta, ell)
                rot = exponents(rng, n, batch)
                if batch == 1:
                    rot = [[0, 1, n - 1, n, n + 1, 2 * n - 1][si % 6]]
                want = to_array(plan, flat(model_terms(polys, rot, w, beta, ell, mode)))
                pa, ra = to_array(plan, flat(polys)), np.array(rot, dtype=np.uint32)
                if where == "host":
                    got = np.zeros_like(want)
                    plan.gadget_decompose_batch(got, pa, beta, ell, rot=ra, mode=mode)
                else:
                    t = dev(torch, np.zeros_like(want))
                    plan.gadget_decompose_batch(t, dev(torch, pa), beta, ell, rot=dev(torch, ra), mode=mode)
                    torch.cuda.synchronize()
                    got = host(t, want.dtype)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (kind, n, batch, beta, ell, mode, npolys, "first bad word", int(bad[0]))


def test_decompose_plain_without_rot_and_streaming_batch():
    """rot = None in the plain mode; a batch whose terms exceed the streaming threshold (non-temporal stores) at n = 1024, compared
    with the same kernel below the threshold on every element and with the model on sampled ones."""
    torch = _torch()
    plan = native64.Plan32.try_new(1024)
    n, beta, ell = 1024, 16, 4
    batch = STREAM_BYTES // (n * 8 * ell) + 5
    g = torch.Generator(device="cuda").manual_seed(5)
    polys = torch.randint(-2 ** 63, 2 ** 63 - 1, (batch * n,), dtype=torch.int64, device="cuda", generator=g)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=g)
    terms = torch.empty(batch * ell * n, dtype=torch.int64, device="cuda")
    plan.gadget_decompose_batch(terms, polys, beta, ell, rot=rot, mode="cmux")
    half = batch // 2
    small = torch.empty((batch - half) * ell * n, dtype=torch.int64, device="cuda")
    plan.gadget_decompose_batch(small[:half * ell * n], polys[:half * n], beta, ell, rot=rot[:half], mode="cmux")
    assert torch.equal(small[:half * ell * n], terms[:half * ell * n])
    plan.gadget_decompose_batch(small[:(batch - half) * ell * n], polys[half * n:], beta, ell, rot=rot[half:], mode="cmux")
    assert torch.equal(small[:(batch - half) * ell * n], terms[half * ell * n:])
    for b in (0, batch // 2, batch - 1):
        f = to_ints(plan, host(polys[b * n:(b + 1) * n], np.uint64))
        want = to_array(plan, flat(model_terms([[f]], [int(rot[b])], 64, beta, ell, "cmux")))
        assert np.array_equal(host(terms[b * ell * n:(b + 1) * ell * n], np.uint64), want), b
    plain = torch.empty(3 * ell * n, dtype=torch.int64, device="cuda")
    plan.gadget_decompose_batch(plain, polys[:3 * n], beta, ell)
    f3 = [[to_ints(plan, host(polys[b * n:(b + 1) * n], np.uint64))] for b in range(3)]
    assert np.array_equal(host(plain, np.uint64), to_array(plan, flat(model_terms(f3, None, 64, beta, ell, "plain"))))


# -- the fused call ---------------------------------------------------------------------------------------------------------------
def key_words(rng, plan, npoly):
    n, w = plan.ntt_size(), wbits(plan)
    if plan.BINARY:
        return [[int(x) for x in rng.integers(0, 2, size=n)] for _ in range(npoly)]
    return [[int.from_bytes(rng.bytes(w // 8), "little") for _ in range(n)] for _ in range(npoly)]


def key_residues(torch, plan, keyw):
    res_t = torch.int64 if plan.RES == 8 else torch.int32
    kr = [torch.empty(len(keyw) * plan.ntt_size(), dtype=res_t, device="cuda") for _ in range(plan.NPRIMES)]
    plan.fwd_batch(dev(torch, to_array(plan, [x for k in keyw for x in k])), kr, binary=plan.BINARY)
    return kr


def oracle_element(oracle, kind, plan, terms_b, keyw, nout):
    """sum_j negacyclic_polymul(terms_b[j], key[j][o]) mod 2^w for one element: nout lists of n ints."""
    ref, n, w = oracle.Native(kind, plan.ntt_size()), plan.ntt_size(), wbits(plan)
    outs = []
    for o in range(nout):
        acc = [0] * n
        for j, t in enumerate(terms_b):
            prod = np.zeros_like(to_array(plan, t))
            ref.negacyclic_polymul(prod, to_array(plan, t), to_array(plan, keyw[j * nout + o]))
            acc = [(x + y) % (1 << w) for x, y in zip(acc, to_ints(plan, prod))]
        outs.append(acc)
    return outs


def run_fused(torch, plan, polys_t, rot_t, kr, beta, ell, nout, mode, addend, batch):
    """addend in {None, "out", "polys", "third"}: returns (out words, the addend's words before the call or None)."""
    n = plan.ntt_size()
    per = n * (2 if plan.WORD == 16 else 1)
    rng = np.random.default_rng(batch + nout)
    prior = rng.integers(0, np.iinfo(plan.word_dtype).max, size=batch * nout * per, dtype=plan.word_dtype, endpoint=True)
    out = dev(torch, prior)
    add_t, add_w = None, None
    if addend == "out":
        add_t, add_w = out, prior
    elif addend == "polys":
        add_t, add_w = polys_t, host(polys_t, plan.word_dtype).copy()
    elif addend == "third":
        add_w = prior[::-1].copy()
        add_t = dev(torch, add_w)
    plan.external_product_decomposed_batch(out, polys_t, kr, beta, ell, nout, rot=rot_t, mode=mode, addend=add_t)
    torch.cuda.synchronize()
    return host(out, plan.word_dtype), add_w


def check_fused(torch, oracle, kind, n, npolys, beta, ell, nout, mode, addend, batch, sample=True):
    plan = KINDS[kind].try_new(n)
    assert plan.max_terms() >= npolys * ell
    w = wbits(plan)
    rng = np.random.default_rng(seed(kind, n, npolys, beta, ell, nout, mode, addend))
    polys = make_polys(rng, plan, batch, npolys, beta, ell)
    rot = exponents(rng, n, batch)
    keyw = key_words(rng, plan, npolys * ell * nout)
    kr = key_residues(torch, plan, keyw)
    polys_t, rot_t = dev(torch, to_array(plan, flat(polys))), dev(torch, np.array(rot, dtype=np.uint32))
    got = {}
    for sw in (1, 0):
        with cntt.debug_switches(native_gadget=sw):
            got[sw], add_w = run_fused(torch, plan, polys_t, rot_t, kr, beta, ell, nout, mode, addend, batch)
    assert np.array_equal(got[1], got[0]), (kind, n, "switch native_gadget 1 / 0 differ")
    # (i) decomposition kernel -> existing external product -> word-wise add, whole batch
    per = n * (2 if plan.WORD == 16 else 1)
    terms = dev(torch, np.zeros(batch * npolys * ell * per, dtype=plan.word_dtype))
    plan.gadget_decompose_batch(terms, polys_t, beta, ell, rot=rot_t, mode=mode)
    ext = dev(torch, np.zeros(batch * nout * per, dtype=plan.word_dtype))
    plan.external_product_batch(ext, terms, kr, npolys * ell, nout)
    torch.cuda.synchronize()
    want = host(ext, plan.word_dtype)
    if add_w is not None:
        want = wadd(plan, want, add_w)
    bad = np.nonzero(got[1] != want)[0]
    assert bad.size == 0, (kind, n, npolys, beta, ell, nout, mode, addend, "vs composition, first bad word", int(bad[0]))
    # (ii) the oracle on the model's digits, sampled elements
    if sample:
        mt = model_terms(polys, rot, w, beta, ell, mode)
        for b in sorted({0, batch // 2, batch - 1}):
            exp = [x for o in oracle_element(oracle, kind, plan, mt[b], keyw, nout) for x in o]
            if add_w is not None:
                exp = [(x + y) % (1 << w) for x, y in zip(exp, to_ints(plan, add_w[b * nout * per:(b + 1) * nout * per]))]
            assert to_ints(plan, got[1][b * nout * per:(b + 1) * nout * per]) == exp, (kind, n, mode, addend, "element", b)


def ragged(n):
    return 4096 // n + 1 if n <= 2048 else 2


@pytest.mark.parametrize("n", [32, 256, 1024, 2048, 4096])
@pytest.mark.parametrize("kind", FUSED)
def test_fused_matches_composition_and_oracle(oracle, kind, n):
    torch = _torch()
    w = 8 * KINDS[kind].WORD
    # (npolys, beta, ell, nout, mode, addend): odd nout (the one-output tail launch), npolys * ell = 1 and = 12, every mode and addend
    cases = [(1, 7, 1, 1, "plain", None), (2, 8, 2, 2, "cmux", "polys"), (2, 5, 3, 3, "rotate", "out"), (3, 4, 4, 2, "cmux", "third"),
             (2, 31, 1, 1, "rotate", None), (2, w // 2 if w == 32 else 16, 2 if w == 32 else 4, 2, "cmux", "out")]
    if n > 1024:
        cases = cases[1:4]
    for npolys, beta, ell, nout, mode, addend in cases:
        check_fused(torch, oracle, kind, n, npolys, beta, ell, nout, mode, addend, ragged(n), sample=(n <= 1024 or addend == "polys"))


@pytest.mark.parametrize("kind,n,beta,ell", [("native128_plan32", 256, 16, 3), ("native_binary128_plan32", 64, 40, 2),
                                             ("native64_plan52", 1024, 8, 3), ("native_binary32_plan52", 256, 4, 2),
                                             ("native64_plan32", 8192, 12, 2), ("native64_plan32", 512, 32, 2)])
def test_composed_shapes_match_composition_and_oracle(oracle, kind, n, beta, ell):
    torch = _torch()
    for mode, addend in (("cmux", "polys"), ("rotate", None)):
        check_fused(torch, oracle, kind, n, 2, beta, ell, 2, mode, addend, 2)


@pytest.mark.parametrize("kind", FUSED)
def test_worst_case_digits_against_the_largest_key(oracle, kind):
    """Every digit at -B/2 (the word whose rounded value has all digit fields zero after the offset: x = -(K 2^s) - ... built from
    the model) against an all-(2^w - 1) key (all ones for the binary kinds) at npolys * levels = 12, n = 4096."""
    torch = _torch()
    n, npolys, beta, ell, nout = 4096, 3, 8, 4, 2
    plan = KINDS[kind].try_new(n)
    assert plan.max_terms() >= 12
    w = wbits(plan)
    B = 1 << beta
    x = sum((-(B // 2)) << (w - beta * l) for l in range(1, ell + 1)) % (1 << w)
    assert digits(x, w, beta, ell) == [-(B // 2)] * ell
    batch = 2
    polys = [[[x] * n for _ in range(npolys)] for _ in range(batch)]
    keyw = [[1 if plan.BINARY else (1 << w) - 1] * n for _ in range(npolys * ell * nout)]
    kr = key_residues(torch, plan, keyw)
    out = dev(torch, np.zeros(batch * nout * n, dtype=plan.word_dtype))
    res = {}
    for sw in (1, 0):
        with cntt.debug_switches(native_gadget=sw):
            plan.external_product_decomposed_batch(out, dev(torch, to_array(plan, flat(polys))), kr, beta, ell, nout)
            torch.cuda.synchronize()
            res[sw] = host(out, plan.word_dtype).copy()
    assert np.array_equal(res[0], res[1])
    mt = model_terms(polys[:1], None, w, beta, ell, "plain")
    exp = [v for o in oracle_element(oracle, kind, plan, mt[0], keyw, nout) for v in o]
    assert to_ints(plan, res[1][:nout * n]) == exp and to_ints(plan, res[1][nout * n:]) == exp


@pytest.mark.parametrize("switch", [0, 1])
@pytest.mark.parametrize("kind", ["native64_plan32", "native_binary32_plan32"])
def test_blind_rotation_shape_three_iterations_on_two_buffers(oracle, kind, switch):
    """acc' = acc + ExtProd(key_i, X^a_i acc - acc): addend = polys, buffers swapped after every call, against the model."""
    torch = _torch()
    n, npolys, beta, ell, batch = 256, 2, 6, 3, 5
    plan = KINDS[kind].try_new(n)
    w = wbits(plan)
    rng = np.random.default_rng(seed(kind, "blind"))
    acc = make_polys(rng, plan, batch, npolys, beta, ell)
    bufs = [dev(torch, to_array(plan, flat(acc))), dev(torch, np.zeros(batch * npolys * n, dtype=plan.word_dtype))]
    for it in range(3):
        rot = exponents(np.random.default_rng(it), n, batch)[::-1]
        keyw = key_words(rng, plan, npolys * ell * npolys)
        kr = key_residues(torch, plan, keyw)
        with cntt.debug_switches(native_gadget=switch):
            plan.external_product_decomposed_batch(bufs[1], bufs[0], kr, beta, ell, npolys,
                                                   rot=dev(torch, np.array(rot, dtype=np.uint32)), mode="cmux", addend=bufs[0])
        torch.cuda.synchronize()
        mt = model_terms(acc, rot, w, beta, ell, "cmux")
        for b in range(batch):
            ext = oracle_element(oracle, kind, plan, mt[b], keyw, npolys)
            acc[b] = [[(x + y) % (1 << w) for x, y in zip(acc[b][p], ext[p])] for p in range(npolys)]
        bufs.reverse()
        assert to_ints(plan, host(bufs[0], plan.word_dtype)) == flat(acc), (kind, "iteration", it)


def test_graph_capture_of_the_fused_call():
    torch = _torch()
    plan = native64.Plan32.try_new(1024)
    n, npolys, beta, ell, nout, batch = 1024, 2, 8, 3, 2, 37
    rng = np.random.default_rng(9)
    polys = dev(torch, to_array(plan, flat(make_polys(rng, plan, batch, npolys, beta, ell))))
    rot = dev(torch, np.array(exponents(rng, n, batch), dtype=np.uint32))
    kr = key_residues(torch, plan, key_words(rng, plan, npolys * ell * nout))
    eager = torch.zeros(batch * nout * n, dtype=torch.int64, device="cuda")
    plan.external_product_decomposed_batch(eager, polys, kr, beta, ell, nout, rot=rot, mode="cmux", addend=polys)
    torch.cuda.synchronize()
    out = torch.zeros_like(eager)
    g = torch.cuda.CUDAGraph()
    with cntt.debug_switches(native_gadget=1):   # the fused kernel: no workspace
        with torch.cuda.graph(g):
            plan.external_product_decomposed_batch(out, polys, kr, beta, ell, nout, rot=rot, mode="cmux", addend=polys)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
