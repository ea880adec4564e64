"""The STREAM = true forms of the automorphism, Galois-keyswitch, merge and ring-pack kernels of the prime plans, and the two multi-bit
call sites of the streaming set-up, on the MI355X.  Every kernel that writes a large intermediate is compiled twice and the host picks
the non-temporal form per launch with `bytes > STREAM_BYTES`; the shapes of the other test files stay far below that threshold, so these
cases sit on the first batch that passes it.  tests/streaming_cases.py computes the shapes and tests/test_streaming_cases.py proves on
the CPU that each full call here streams, that one batch element fewer would not, and that no reference call streams at any launch.

Bit-exact throughout, no tolerance anywhere.  Every full call is compared on every word with the same call made over halves (chunks) of
the batch, and with a second reference that shares no kernel form with it: a numpy restatement (automorphism), the composition of public
calls per element (keyswitch, merge) or per chunk (ring packing), the plain-int `source` model (set-up).  Inputs are drawn on the device;
the first and the last element start with edge_words(p, base_log, levels), so the digit rule's corners pass through the streaming
stores.  The cases that take the "autom_lds" switch run under both of its settings."""
import gc

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import streaming_cases as sc
import test_gpu_prime_automorphism as tga
import test_gpu_prime_ring_pack as tgr
from prime_automorphism_model import autom_gather_np, ntt_permutation
from test_gpu_native_pbs import KINDS, per as native_per, source as native_source, to_ints
from test_gpu_prime_pack import first_difference
from test_gpu_prime_pbs import _torch, dev, device_words, dt, host, is64, make_plan, seed
from test_prime_pbs_model import edge_words, source

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
REFERENCE = {}            # ring packing: the composition's words of a case, computed once and shared by both settings of the switch


@pytest.fixture(autouse=True)
def free_device_memory():
    """a case holds up to a gigabyte: hand it back before the next one"""
    yield
    gc.collect()
    _torch().cuda.empty_cache()


def word(p):
    return np.dtype(dt(p)).itemsize


def sampled(rng, batch, count):
    return sorted({0, batch - 1} | {int(x) for x in rng.integers(0, batch, size=count)})


def generator(torch, *parts):
    return torch.Generator(device="cuda").manual_seed(seed("streaming", *parts))


def stream_words(torch, p, count, per, gen, beta, ell):
    """count canonical words drawn on the device; the first and the last element (per words each) start with the edge words"""
    t = device_words(torch, p, count, gen)
    e = dev(torch, np.array(edge_words(p, beta, ell), dtype=dt(p)))[:per]
    t[:e.numel()] = e
    t[count - per:count - per + e.numel()] = e
    return t


def poisoned(torch, like, count=None):
    return torch.full((like.numel() if count is None else count,), POISON, dtype=like.dtype, device="cuda")


def assert_halves(torch, call, out, half_words, what):
    """call(small, lo, hi) runs the same call on the elements whose output words are out[lo:hi]; both halves against the full call"""
    small = poisoned(torch, out, out.numel() - half_words)
    for lo, hi in ((0, half_words), (half_words, out.numel())):
        part = small[:hi - lo]
        call(part, lo, hi)
        assert torch.equal(part, out[lo:hi]), (what, "words %d .. %d" % (lo, hi), first_difference(host(part, np.uint8), host(out[lo:hi], np.uint8)))


# -- a. the automorphism in both domains -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,lds", sc.gpu_cases("automorphism"), ids=sc.case_id)
def test_automorphism_of_a_streaming_batch(case, lds):
    """prime_automorphism_kernel<T, true, LDS> and prime_automorphism_ntt_kernel<T, true, LDS>: the first polynomial count with
    2 * polys * n * word > STREAM_BYTES.  Coefficient domain: every word against the numpy gather out[j] = +-in[j t^-1 mod 2n] and against
    the call in two halves.  NTT domain: every word against the halves, and the first, the last and 32 sampled polynomials against the
    slot rule 2 brev(c') + 1 = t (2 brev(c) + 1) mod 2n.  At n = 16384 the polynomial cannot be staged: autom_lds = 1 takes the
    launcher's fallback to the global gather."""
    torch = _torch()
    p, n, polys = case["p"], case["n"], case["batch"]
    assert sc.streams(sc.autom_bytes(polys, n, word(p))) and (n * word(p) > tga.LDS_BYTES) == (n == 16384)
    plan = make_plan(p, n)
    f = stream_words(torch, p, polys * n, n, generator(torch, case["name"]), 4 if is64(p) else 2, 15)
    fh = host(f, dt(p)).reshape(polys, n)
    out = poisoned(torch, f)
    picks = sampled(np.random.default_rng(seed("streaming", case["name"])), polys, 32)
    with cntt.debug_switches(autom_lds=lds):
        for t in case["ts"]:
            for ntt in (False, True):
                call = plan.automorphism_ntt_batch if ntt else plan.automorphism_batch
                out.fill_(POISON)
                call(out, f, t)
                assert_halves(torch, lambda part, lo, hi: call(part, f[lo:hi], t), out, polys // 2 * n, (case["name"], lds, t, ntt))
                got = host(out, dt(p)).reshape(polys, n)
                if ntt:
                    src = ntt_permutation(t, n)
                    for b in picks:
                        assert np.array_equal(got[b], fh[b, src]), (case["name"], lds, t, "ntt", "polynomial", b)
                else:
                    want = autom_gather_np(fh, t, p)
                    assert np.array_equal(got, want), (case["name"], lds, t, first_difference(got.reshape(-1), want.reshape(-1)))
    assert np.array_equal(host(f, dt(p)).reshape(polys, n), fh)


# -- b. the Galois keyswitch and the trace ---------------------------------------------------------------------------------------------------
def ciphertext_case(torch, case, keys=1, inputs=1):
    """the plan, the seeded generator, the NTT-domain key(s), `inputs` ciphertext batches of a case and the words of one ciphertext"""
    p, n, k, beta, ell, batch = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["batch"]
    assert sc.streams(sc.digit_bytes(batch, k, ell, n, word(p))) and not sc.streams(sc.digit_bytes(batch - 1, k, ell, n, word(p)))
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("streaming", case["name"]))
    kw, kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=keys)
    del kw
    gen = generator(torch, case["name"])
    per = (k + 1) * n
    cts = [stream_words(torch, p, batch * per, per, gen, beta, ell) for _ in range(inputs)]
    return plan, rng, kt, cts, per


@pytest.mark.parametrize("case,lds", sc.gpu_cases("autoks"), ids=sc.case_id)
def test_galois_keyswitch_of_a_streaming_batch(case, lds):
    """prime_automorphism_gadget_kernel<T, true, LDS>: the first batch whose digits (batch * k * 15 levels * n words) pass STREAM_BYTES,
    with add_input false and true and a caller workspace of exactly glwe_automorphism_keyswitch_workspace_bytes.  Every word against
    the call over two halves of the batch (library-allocated workspace); the first, the last and 8 sampled elements against the header's
    sequence of public calls (automorphism_batch, gadget_decompose_batch, external_product_batch), one element at a time."""
    torch = _torch()
    p, n, k, beta, ell, batch = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["batch"]
    plan, rng, kt, (ct,), per = ciphertext_case(torch, case)
    nws = plan.glwe_automorphism_keyswitch_workspace_bytes(k, ell, batch)
    assert nws == sc.up256(sc.digit_bytes(batch, k, ell, n, word(p)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = poisoned(torch, ct)
    picks = sampled(rng, batch, 8)
    with cntt.debug_switches(autom_lds=lds):
        for t, add in zip(case["ts"], (False, True)):
            out.fill_(POISON)
            plan.glwe_automorphism_keyswitch_batch(out, ct, kt, t, k, beta, ell, add, workspace=ws)
            assert_halves(torch, lambda part, lo, hi: plan.glwe_automorphism_keyswitch_batch(part, ct[lo:hi], kt, t, k, beta, ell, add), out,
                          batch // 2 * per, (case["name"], lds, t, add))
            for b in picks:
                one = host(ct[b * per:(b + 1) * per], dt(p))
                want = tga.compose(torch, plan, p, one, kt, t, k, beta, ell, add, 1)
                got = host(out[b * per:(b + 1) * per], dt(p))
                assert got.any() and np.array_equal(got, want), (case["name"], lds, t, add, "element", b, first_difference(got, want))


@pytest.mark.parametrize("case,lds", sc.gpu_cases("trace"), ids=sc.case_id)
def test_trace_of_a_streaming_batch(case, lds):
    """glwe_trace_batch with steps = 2 at the keyswitch's shape: both steps stream (add_input), the second from the workspace's second
    ciphertext.  Every word against two keyswitch calls per half of the batch, which do not stream."""
    torch = _torch()
    p, n, k, beta, ell, batch, steps = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["batch"], case["steps"]
    plan, rng, kt, (ct,), per = ciphertext_case(torch, case, keys=steps)
    ws = torch.empty(plan.glwe_trace_workspace_bytes(k, ell, batch), dtype=torch.uint8, device="cuda")
    out = poisoned(torch, ct)
    key_words = k * ell * (k + 1) * n

    def in_steps(part, lo, hi):
        cur = ct[lo:hi]
        for r, t in enumerate(case["ts"]):
            nxt = part if r == steps - 1 else poisoned(torch, cur)
            plan.glwe_automorphism_keyswitch_batch(nxt, cur, kt[r * key_words:(r + 1) * key_words], t, k, beta, ell, True)
            cur = nxt

    with cntt.debug_switches(autom_lds=lds):
        plan.glwe_trace_batch(out, ct, kt, steps, k, beta, ell, workspace=ws)
        assert_halves(torch, in_steps, out, batch // 2 * per, (case["name"], lds))
    assert bool(out.any()) and not torch.equal(out, ct)


# -- c. one tree node, and the whole packing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,lds", sc.gpu_cases("merge"), ids=sc.case_id)
def test_merge_of_a_streaming_batch(case, lds):
    """prime_ring_merge_kernel<T, true, LDS, false> at the keyswitch's shapes, shift 1 and n / 2, with a caller workspace of exactly
    glwe_merge_workspace_bytes.  Every word against the call over two halves; the first, the last and 8 sampled elements against
    E + X^shift O + AutoKS_t(E - X^shift O) built from the public calls."""
    torch = _torch()
    p, n, k, beta, ell, batch = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["batch"]
    plan, rng, kt, (E, O), per = ciphertext_case(torch, case, inputs=2)
    nws = plan.glwe_merge_workspace_bytes(k, ell, batch)
    assert nws == sc.up256(sc.digit_bytes(batch, k, ell, n, word(p)))
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = poisoned(torch, E)
    picks = sampled(rng, batch, 8)
    with cntt.debug_switches(autom_lds=lds):
        for shift, t in zip(case["shifts"], case["ts"]):
            out.fill_(POISON)
            plan.glwe_merge_batch(out, E, O, kt, shift, t, k, beta, ell, workspace=ws)
            assert_halves(torch, lambda part, lo, hi: plan.glwe_merge_batch(part, E[lo:hi], O[lo:hi], kt, shift, t, k, beta, ell), out,
                          batch // 2 * per, (case["name"], lds, shift, t))
            for b in picks:
                e1, o1 = (host(x[b * per:(b + 1) * per], dt(p)) for x in (E, O))
                want = tgr.compose_merge(torch, plan, p, e1, o1, kt, shift, t, k, beta, ell)
                got = host(out[b * per:(b + 1) * per], dt(p))
                assert got.any() and np.array_equal(got, want), (case["name"], lds, shift, t, "element", b, first_difference(got, want))


@pytest.mark.parametrize("case,lds", sc.gpu_cases("ring_pack"), ids=sc.case_id)
def test_ring_pack_of_a_streaming_batch(case, lds):
    """prime_ring_merge_kernel<T, true, LDS, true>.  lwe_count = 2: the one tree level is a leaf level that streams, and the nine trace
    steps after it stream too.  lwe_count = 4: the leaf level holds 2 * batch ciphertexts and streams while the level above it and the
    trace do not, so one call crosses the threshold between two of its own launches.  Every word against the call over two chunks of the
    batch and against embed -> merges -> trace on the same chunks; neither streams at any level (tests/test_streaming_cases.py)."""
    torch = _torch()
    p, n, k, beta, ell, batch, m = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["batch"], case["lwe_count"]
    w, logn, row, per = word(p), n.bit_length() - 1, k * n + 1, (k + 1) * n
    full = dict(sc.ring_pack_launches(n, w, m, k, ell, batch))
    assert sc.streams(full["tree level 1 (leaf)"]) and sc.streams(full["trace step 0"]) == (m == 2)
    plan = make_plan(p, n)
    rng = np.random.default_rng(seed("streaming", case["name"]))
    kt = tga.key_for(torch, plan, p, rng, k, ell, n, keys=logn)[1]
    lwe = stream_words(torch, p, batch * m * row, m * row, generator(torch, case["name"]), beta, ell)
    nws = plan.ring_pack_workspace_bytes(m, k, ell, batch)
    assert nws == sc.ring_pack_workspace(n, w, m, k, ell, batch)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    out = poisoned(torch, lwe, batch * per)
    bounds = [(lo, lo + cb) for lo, cb in zip([0, case["chunks"][0]], case["chunks"])]
    assert bounds[-1][1] == batch
    with cntt.debug_switches(autom_lds=lds):
        plan.ring_pack_batch(out, lwe, kt, m, k, beta, ell, workspace=ws)
        for lo, hi in bounds:
            part = poisoned(torch, lwe, (hi - lo) * per)
            plan.ring_pack_batch(part, lwe[lo * m * row:hi * m * row], kt, m, k, beta, ell)
            assert torch.equal(part, out[lo * per:hi * per]), (case["name"], lds, "chunk", lo, hi)
            del part
    del ws
    if case["name"] not in REFERENCE:
        REFERENCE[case["name"]] = np.concatenate([tgr.compose_pack(torch, plan, p, host(lwe[lo * m * row:hi * m * row], dt(p)), kt, m, k, beta, ell, hi - lo)
                                                  for lo, hi in bounds])
    got, want = host(out, dt(p)), REFERENCE[case["name"]]
    assert got.any() and np.array_equal(got, want), (case["name"], lds, first_difference(got, want))


# -- d. the two multi-bit call sites of the streaming set-up ---------------------------------------------------------------------------------
def test_prime_multibit_set_up_of_a_streaming_batch():
    """prime_pbs_init_kernel<T, true> from multibit_blind_rotate_batch: lwe_dim = 0 is the set-up alone (acc = X^rot lut: no digits, no
    key); grouping 2, a table per element.  Every word against the call in two halves; the first, the last and 32 sampled elements
    against the `source` model."""
    torch = _torch()
    case = sc.BY_NAME["multibit-setup-p62"]
    p, n, k, beta, ell, g, batch = case["p"], case["n"], case["k"], case["base_log"], case["levels"], case["grouping"], case["batch"]
    per = (k + 1) * n
    assert sc.streams(sc.acc_bytes(batch, k, n, word(p))) and not sc.streams(sc.acc_bytes(batch - 1, k, n, word(p))) and case["lut_per_element"]
    plan = make_plan(p, n)
    gen = generator(torch, case["name"])
    lut = stream_words(torch, p, batch * per, per, gen, beta, ell)
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=gen)
    nokey = torch.empty(0, dtype=lut.dtype, device="cuda")
    acc = poisoned(torch, lut)
    plan.multibit_blind_rotate_batch(acc, lut, rot, nokey, 0, k, beta, ell, g, lut_per_element=True)
    assert_halves(torch, lambda part, lo, hi: plan.multibit_blind_rotate_batch(part, lut[lo:hi], rot[lo // per:hi // per], nokey, 0, k, beta, ell, g,
                                                                               lut_per_element=True), acc, batch // 2 * per, case["name"])
    rot_h = rot.cpu().tolist()
    for b in sampled(np.random.default_rng(seed("streaming", case["name"])), batch, 32):
        f = host(lut[b * per:(b + 1) * per], dt(p)).tolist()
        want = [x for q in range(k + 1) for x in source(f[q * n:(q + 1) * n], rot_h[b], p, "rotate")]
        assert host(acc[b * per:(b + 1) * per], dt(p)).tolist() == want, (case["name"], "element", b)


def test_native_multibit_set_up_of_a_streaming_batch():
    """the native set-up kernel's streaming form from multibit_blind_rotate_batch on 64-bit words: lwe_dim = 0, grouping 2, one shared
    table.  Every word against the call in two halves; the first, the last and 32 sampled elements against the `source` model."""
    torch = _torch()
    case = sc.BY_NAME["multibit-setup-native64"]
    n, k, beta, ell, g, batch = case["n"], case["k"], case["base_log"], case["levels"], case["grouping"], case["batch"]
    plan = KINDS[case["kind"]].try_new(n)
    assert plan.WORD == case["word"] == 8 and not case["lut_per_element"]
    assert sc.streams(sc.acc_bytes(batch, k, n, plan.WORD)) and not sc.streams(sc.acc_bytes(batch - 1, k, n, plan.WORD))
    pe = (k + 1) * native_per(plan)
    gen = generator(torch, case["name"])
    lut = torch.randint(-2 ** 63, 2 ** 63 - 1, (pe,), dtype=torch.int64, device="cuda", generator=gen)
    lut[:4] = torch.tensor([0, 1, -1, -2 ** 63], dtype=torch.int64, device="cuda")          # 0, 1, 2^64 - 1, 2^63
    rot = torch.randint(0, 2 * n, (batch,), dtype=torch.int32, device="cuda", generator=gen)
    nokey = [torch.empty(0, dtype=torch.int32, device="cuda") for _ in range(plan.NPRIMES)]
    acc = poisoned(torch, lut, batch * pe)
    plan.multibit_blind_rotate_batch(acc, lut, rot, nokey, 0, k, beta, ell, g)
    assert_halves(torch, lambda part, lo, hi: plan.multibit_blind_rotate_batch(part, lut, rot[lo // pe:hi // pe], nokey, 0, k, beta, ell, g), acc,
                  batch // 2 * pe, case["name"])
    rot_h = rot.cpu().tolist()
    f = to_ints(plan, host(lut, plan.word_dtype))
    for b in sampled(np.random.default_rng(seed("streaming", case["name"])), batch, 32):
        want = [x for q in range(k + 1) for x in native_source(f[q * n:(q + 1) * n], rot_h[b], 64, "rotate")]
        assert to_ints(plan, host(acc[b * pe:(b + 1) * pe], plan.word_dtype)) == want, (case["name"], "element", b)
