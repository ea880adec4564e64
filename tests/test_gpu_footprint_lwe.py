"""tests/test_gpu_footprint.py continued for the calls on LWE ciphertexts around the bootstrap: cntt_keyswitch.h and
cntt_prime_keyswitch.h (the LWE keyswitch, and keyswitch + bootstrap in one call), cntt_pack.h and cntt_prime_pack.h (the LWE-to-GLWE
packing keyswitch).  Every operand -- lwe_in, the key, the output, the caller's workspace -- is an exact-size slice of a guard-band arena
(tests/guard_arena.py); the native plans' key residue planes live in a uint32 arena of their own.  Each case asserts
  * the written slice bit-exact against the integer model of the module that owns the call (the combined call: keyswitch_batch followed
    by bootstrap_batch on plain tensors, which those modules pin to the models);
  * check() on every arena it built: every band word, and lwe_in, ksk, lut and the key, byte for byte what they were.
The value tests of those modules walk the same tile and chunk edges on whole tensors, where a store one row or one polynomial past an
operand, or past the workspace, lands in the allocator's padding; here it lands in a band.

What is live at these shapes.  The keyswitch is a tiled GEMM: a workgroup owns BM batch elements x BN = 128 columns, computes the rows
past `batch` and the columns past Lout + 1 anyway, and only its masks keep them from being stored into rows that have no padding.  The
packing keyswitch transposes TT = 64 ciphertexts x TI mask words through LDS into the workspace, zero tail included, chunk by chunk, the
last chunk ragged.  The combined call keeps the keyswitched ciphertexts at the very END of the caller's workspace, so the keyswitch's
masked edges sit on the end of a caller buffer.  The tile constants are those the owning test modules restate from the kernels.

Bands.  Behind a keyswitch output one full tile of rows plus one tile of columns, BM (Lout + 1) + BN words (256 at least); behind a GLWE
or bootstrap output the band of test_gpu_footprint; behind a packing workspace one tile's stores, TI * levels polynomials
(MIN_GUARD_POLYS at least); behind the combined call's workspace the larger of the bootstrap's and the keyswitch's band: a store that
lost its mask still lands inside the arena.  u32 and u64 words run 16-byte aligned and one word past a 16-byte boundary; u128 words
(two uint64 arena words per coefficient) are 16-byte aligned by their type and run aligned only; workspaces are always 16-byte aligned.
The host path (numpy arenas) runs one case per call: its copies in and out move byte counts computed on the host."""
import numpy as np
import pytest

import prime_pack_model as ppm
import test_gpu_native_keyswitch as nks
import test_gpu_native_pack as npk
import test_gpu_prime_keyswitch as pks
from guard_arena import MIN_GUARD_POLYS, GuardArena
from test_gpu_footprint import PBS_BATCH, PBS_ELL, PBS_K, PBS_L, PBS_N, Family, _dev, batches_of, guard, guard_both
from test_gpu_prime_pbs import dt, host, key_ntt, make_plan, min_n, random_words
from test_prime_keyswitch_abi import chunk_words, model_keyswitch
from test_prime_pbs_model import P30, P62

pytestmark = pytest.mark.gpu

BN = nks.TILE_C
assert pks.TILE_C == BN
KS_DIGITS = (4, 3)                     # the combined call's keyswitch digits
ODD = [False, True]
ODD_IDS = ["aligned", "odd"]
WS_IDS = ["null-workspace", "caller-workspace"]
# (word width, odd): u128 words have no odd placement
NATIVE = [(w, odd) for w in (32, 64, 128) for odd in ODD if not (odd and w == 128)]
NATIVE_IDS = ["u%d-%s" % (w, "odd" if o else "aligned") for (w, o) in NATIVE]
PRIMES = [(P62, "P62"), (P30, "P30")]


def _torch():
    import torch
    return torch


def empty(torch, dtype, device):
    """an operand of no words (a key when Lin == 0), as the owning tests pass it"""
    if device:
        return torch.empty(0, dtype=torch.int32 if np.dtype(dtype).itemsize == 4 else torch.int64, device="cuda")
    return np.zeros(0, dtype=dtype)


def picked(cases, only):
    """every case, or the one the host-path tests run"""
    return cases if only is None else [cases[only]]


def check_all(arenas):
    for a in arenas:
        a.check()


# ---- a. the keyswitch alone -----------------------------------------------------------------------------------------------------------
def ks_guard(bm, lout):
    """coefficients behind a keyswitch output: one full tile of rows and one tile of columns"""
    return max(256, bm * (lout + 1) + BN)


def ks_cases(bm, c):
    """(batch, Lin, Lout, row pad, base_log, levels); bm = the tile's batch elements, c = the chunk in mask words at (4, 3)"""
    cases = [(1, 3, 0, 0, 5, 3),                 # body-only output, one row
             (bm - 1, 2, BN - 2, 3, 4, 3),       # one column short of a column tile, padded key rows
             (bm + 1, 2, BN, 0, 4, 3),           # one row and one column into the second tile in both directions
             (3, c + 1, 4, 1, 4, 3),             # two chunks along Lin, the second of one word
             (5, 0, 9, 0, 6, 2)]                 # Lin == 0: body copied, mask zeroed
    assert set(batches_of([bm])) <= {case[0] for case in cases}
    return cases


def keyswitch_on_arena(torch, plan, dtype, mult, device, odd, seed, lwe_a, ksk_a, case, bm):
    """the call with ksk, lwe_out and lwe_in carved from one arena in that order -> the output words"""
    batch, lin, lout, pad, beta, ell = case
    ar = GuardArena(dtype, device, seed, odd)
    if lin:
        ar.take("ksk", ksk_a)                    # exactly (Lin levels - 1) row_stride + Lout + 1 words: it ends where the last row ends
    ar.take("lwe_out", batch * (lout + 1) * mult, written=True, guard=ks_guard(bm, lout) * mult).take("lwe_in", lwe_a).build()
    plan.keyswitch_batch(ar["lwe_out"], ar["lwe_in"], ar["ksk"] if lin else empty(torch, dtype, device), lin, lout, beta, ell,
                         row_stride=lout + 1 + pad)
    return ar.check()["lwe_out"]


def run_native_keyswitch(w, odd, device, only=None):
    torch = _torch()
    plan = nks.WORDS[w].try_new(32)                           # ntt_size plays no part
    mult = 2 if w == 128 else 1
    for case in picked(ks_cases(nks.TILE_B[w], nks.ROWS // 3), only):
        batch, lin, lout, pad, beta, ell = case
        stride = lout + 1 + pad
        rng = np.random.default_rng(nks.seed("footprint", w, *case))
        lwe = nks.rand_ints(rng, w, batch * (lin + 1))
        ksk = nks.rand_ints(rng, w, nks.key_len(lin, ell, lout, stride))
        want = nks.model_keyswitch_batch(lwe, ksk, lin, lout, stride, w, beta, ell, batch)
        got = keyswitch_on_arena(torch, plan, plan.word_dtype, mult, device, odd, 11 + batch, nks.to_array(plan, lwe),
                                 nks.to_array(plan, ksk), case, nks.TILE_B[w])
        assert nks.to_ints(plan, got) == want, (w, odd, device, case)


def run_prime_keyswitch(p, odd, device, only=None):
    torch = _torch()
    plan = make_plan(p, min_n(p))
    for case in picked(ks_cases(pks.TILE_B, chunk_words(4, 3)), only):
        batch, lin, lout, pad, beta, ell = case
        stride = lout + 1 + pad
        rng = np.random.default_rng(nks.seed("footprint", p, *case))
        lwe = pks.words_with_edges(rng, p, batch * (lin + 1), beta, ell, dt(p))
        ksk = random_words(rng, p, nks.key_len(lin, ell, lout, stride))
        want = model_keyswitch(lwe.tolist(), ksk.tolist(), p, lin, lout, stride, beta, ell, batch)
        got = keyswitch_on_arena(torch, plan, dt(p), 1, device, odd, 12 + batch, lwe, ksk, case, pks.TILE_B)
        assert got.tolist() == want, (p, odd, device, case)


@pytest.mark.parametrize("w,odd", NATIVE, ids=NATIVE_IDS)
def test_native_keyswitch_footprint(w, odd):
    """cntt_native_keyswitch_batch on u32 / u64 / u128 words against model_keyswitch_batch"""
    run_native_keyswitch(w, odd, True)


@pytest.mark.parametrize("odd", ODD, ids=ODD_IDS)
@pytest.mark.parametrize("p,name", PRIMES, ids=[nm for (_, nm) in PRIMES])
def test_prime_keyswitch_footprint(p, name, odd):
    """cntt_prime64 / prime32_keyswitch_batch against model_keyswitch"""
    run_prime_keyswitch(p, odd, True)


# ---- b. keyswitch + bootstrap in one call -----------------------------------------------------------------------------------------------
def bootstrap_key(f, torch, rng, npoly, odd, device):
    """Family.key, and the same on numpy arenas for the host path: (the key argument, its arenas, the key on plain device tensors)"""
    if device:
        return f.key(torch, rng, npoly, odd)
    kw = f.words(rng, npoly * f.n)
    if not f.native:
        ar = GuardArena(f.dt, False, 91, odd).take("bsk", kw).build()
        return ar["bsk"], [ar], f.tpp.dev(torch, kw)
    plain = f.tnp.key_planes(torch, f.plan, kw)
    ar = GuardArena(np.uint32, False, 92, odd)
    for i, t in enumerate(plain):
        ar.take("k%d" % i, f.tnp.host(t, np.uint32))
    ar.build()
    return [ar["k%d" % i] for i in range(len(plain))], [ar], plain


def run_combined(fam, odd, with_ws, device):
    torch = _torch()
    f = Family(fam, PBS_N)
    n, L, k, ell, batch = PBS_N, PBS_L, PBS_K, PBS_ELL, PBS_BATCH
    assert (n, L, k, ell, batch) == (64, 3, 1, 2, 3)
    ks_beta, ks_ell = KS_DIGITS
    big, stride = k * n, L + 1 + (1 if odd else 0)
    rng = np.random.default_rng(nks.seed("combined", fam, odd, with_ws, device))
    lwe, lut = f.words(rng, batch * (big + 1)), f.words(rng, (k + 1) * n)
    ksk = f.words(rng, nks.key_len(big, ks_ell, L, stride))     # k n ks_levels rows, the last one ends after its L + 1 words
    key, key_arenas, key_plain = bootstrap_key(f, torch, rng, L * (k + 1) * ell * (k + 1), odd, device)
    wsb, isz = f.plan.ks_pbs_workspace_bytes(L, k, ell, batch), np.dtype(f.dt).itemsize
    assert wsb % isz == 0 and wsb > f.plan.pbs_workspace_bytes(L, k, ell, batch)
    g = guard(f.bits, n)
    bm = nks.TILE_B[64] if f.native else pks.TILE_B
    ar = GuardArena(f.dt, device, 14, odd).take("ksk", ksk).take("lwe_out", batch * (big + 1), written=True, guard=g).take("lwe_in", lwe)
    ar.take("lut", lut)
    if with_ws:                                                  # the keyswitched ciphertexts are the last words of this slice
        ar.take("ws", wsb // isz, written=True, guard=max(g, ks_guard(bm, L)), aligned=True)
    ar.build()
    f.plan.keyswitch_bootstrap_batch(ar["lwe_out"], ar["lwe_in"], ar["ksk"], ks_beta, ks_ell, ar["lut"], key, L, k, f.beta, ell,
                                     workspace=ar["ws"] if with_ws else None, row_stride=stride)
    got = ar.check()["lwe_out"]
    check_all(key_arenas)
    lwe_t = _dev(torch, lwe)
    mid = torch.zeros(batch * (L + 1), dtype=lwe_t.dtype, device="cuda")
    two = torch.zeros(batch * (big + 1), dtype=lwe_t.dtype, device="cuda")
    f.plan.keyswitch_batch(mid, lwe_t, _dev(torch, ksk), big, L, ks_beta, ks_ell, row_stride=stride)
    f.plan.bootstrap_batch(two, mid, _dev(torch, lut), key_plain, L, k, f.beta, ell)
    torch.cuda.synchronize()
    assert np.array_equal(got, two.cpu().numpy().view(f.dt)), (fam, odd, with_ws, device)
    assert got.any() and mid.any()


@pytest.mark.parametrize("with_ws", [False, True], ids=WS_IDS)
@pytest.mark.parametrize("odd", ODD, ids=ODD_IDS)
@pytest.mark.parametrize("fam", ["native64", "prime64", "prime32"])
def test_keyswitch_bootstrap_footprint(fam, odd, with_ws):
    """cntt_native / prime64 / prime32_keyswitch_bootstrap_batch: lwe_out and the workspace written; lwe_in, ksk, lut and the bootstrapping
    key read; against keyswitch_batch followed by bootstrap_batch on plain tensors"""
    run_combined(fam, odd, with_ws, True)


# ---- c. the packing keyswitch ---------------------------------------------------------------------------------------------------------
def pack_cases(ti, c):
    """(n, batch, m, Lin, k, base_log, levels); ti = the tile's mask words, c = the chunk in mask words at 3 levels"""
    return [(32, 1, 1, 0, 1, 5, 3),              # Lin == 0: only the body kernel runs, no workspace
            (32, 3, 31, ti + 1, 2, 4, 3),        # n < TT, m = n - 1, second i tile of one word, three outputs
            (128, 2, ppm.TT + 1, 3, 1, 5, 3),    # second t tile: one live coefficient, then the zero tail
            (32, 1, 32, c + 1, 1, 4, 3)]         # two chunks, the second of one mask word


assert npk.TT == ppm.TT


def pack_on_arenas(torch, plan, dtype, mult, device, odd, seed, lwe_a, key_dtype, key_parts, case, with_ws, out_guard, ti):
    """the call with glwe_out, lwe_in and (with_ws) the workspace carved from one arena, the key's parts from a second one -> the output
    words.  key_parts: the native plans' residue planes (a list), or the prime plans' one buffer (an array)."""
    n, batch, m, lin, k, beta, ell = case
    single = not isinstance(key_parts, list)
    parts = [key_parts] if single else key_parts
    arenas = []
    if lin:
        ka = GuardArena(key_dtype, device, seed + 1, odd)
        for i, q in enumerate(parts):
            ka.take("k%d" % i, q)
        ka.build()
        arenas.append(ka)
        key = [ka["k%d" % i] for i in range(len(parts))]
    else:
        key = [empty(torch, key_dtype, device) for _ in parts]
    wsb, isz = plan.pack_workspace_bytes(lin, ell, batch), np.dtype(dtype).itemsize
    assert wsb % isz == 0 and (wsb == 0) == (lin == 0)
    use_ws = with_ws and wsb > 0                                 # a workspace of zero bytes: pass none
    ar = GuardArena(dtype, device, seed, odd).take("glwe_out", batch * (k + 1) * n * mult, written=True, guard=out_guard).take("lwe_in", lwe_a)
    if use_ws:
        ar.take("ws", wsb // isz, written=True, guard=max(ti * ell, MIN_GUARD_POLYS) * n * mult, aligned=True)
    ar.build()
    arenas.append(ar)
    plan.pack_keyswitch_batch(ar["glwe_out"], ar["lwe_in"], key[0] if single else key, lin, m, k, beta, ell,
                              workspace=ar["ws"] if use_ws else None)
    got = ar.check()["glwe_out"]
    check_all(arenas[:-1])
    return got


def run_native_pack(w, odd, with_ws, device, only=None):
    torch = _torch()
    plans = {n: npk.WORDS[w].try_new(n) for n in (32, 128)}
    mult = 2 if w == 128 else 1
    model_dtype = {32: np.uint32, 64: np.uint64, 128: object}[w]
    for case in picked(pack_cases(npk.TI[w], npk.C(plans[32], 3)), only):
        n, batch, m, lin, k, beta, ell = case
        plan = plans[n]
        rng = np.random.default_rng(npk.seed("footprint", w, *case))
        lwe = npk.rand_ints(rng, w, batch * m * (lin + 1))
        key = npk.rand_ints(rng, w, lin * ell * (k + 1) * n)
        want = npk.model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch, dtype=model_dtype)
        planes = [npk.host(t, plan.res_dtype) for t in npk.key_planes(torch, plan, npk.to_array(plan, key))]
        got = pack_on_arenas(torch, plan, plan.word_dtype, mult, device, odd, 21 + batch, npk.to_array(plan, lwe), plan.res_dtype, planes,
                             case, with_ws, guard_both(n, mult), npk.TI[w])
        assert npk.to_ints(plan, got) == want, (w, odd, with_ws, device, case, npk.first_difference(npk.to_ints(plan, got), want))


def run_prime_pack(p, odd, with_ws, device, only=None):
    torch = _torch()
    plans = {n: make_plan(p, n) for n in (32, 128)}
    bits = 8 * np.dtype(dt(p)).itemsize
    for case in picked(pack_cases(ppm.TI, ppm.C(3)), only):
        n, batch, m, lin, k, beta, ell = case
        plan = plans[n]
        rng = np.random.default_rng(npk.seed("footprint", p, *case))
        lwe = random_words(rng, p, batch * m * (lin + 1))
        key = random_words(rng, p, lin * ell * (k + 1) * n)
        want = ppm.model_pack_batch(lwe.tolist(), key.tolist(), p, lin, m, k, n, beta, ell, batch)
        kt = host(key_ntt(torch, plan, key), dt(p)) if lin else np.zeros(0, dtype=dt(p))
        torch.cuda.synchronize()
        got = pack_on_arenas(torch, plan, dt(p), 1, device, odd, 22 + batch, lwe, dt(p), kt, case, with_ws, guard(bits, n), ppm.TI)
        assert got.tolist() == want, (p, odd, with_ws, device, case)


@pytest.mark.parametrize("with_ws", [False, True], ids=WS_IDS)
@pytest.mark.parametrize("w,odd", NATIVE, ids=NATIVE_IDS)
def test_native_pack_footprint(w, odd, with_ws):
    """cntt_native_pack_keyswitch_batch on u32 / u64 / u128 words against model_pack_batch; glwe_out starts as pattern words, so the
    comparison also proves the zero mask polynomials and the zero tail were stored"""
    run_native_pack(w, odd, with_ws, True)


@pytest.mark.parametrize("with_ws", [False, True], ids=WS_IDS)
@pytest.mark.parametrize("odd", ODD, ids=ODD_IDS)
@pytest.mark.parametrize("p,name", PRIMES, ids=[nm for (_, nm) in PRIMES])
def test_prime_pack_footprint(p, name, odd, with_ws):
    """cntt_prime64 / prime32_pack_keyswitch_batch against prime_pack_model.model_pack_batch"""
    run_prime_pack(p, odd, with_ws, True)


# ---- d. the host path -------------------------------------------------------------------------------------------------------------------
# CNTT_MEM_HOST: numpy arenas, one word past a 16-byte boundary, the smallest non-trivial shape of each call.  The kernels work on the
# library's staging copies; what the bands see here are the copies in and out, whose byte counts are computed on the host -- a count one
# row too long lands in a band.
@pytest.mark.parametrize("family", ["native64", "prime32"])
def test_keyswitch_footprint_host_path(family):
    """two chunks along Lin, padded key rows whose last row ends early"""
    if family == "native64":
        run_native_keyswitch(64, True, False, only=3)
    else:
        run_prime_keyswitch(P30, True, False, only=3)


@pytest.mark.parametrize("with_ws", [False, True], ids=WS_IDS)
@pytest.mark.parametrize("family", ["native64", "prime32"])
def test_pack_footprint_host_path(family, with_ws):
    """n < TT, m = n - 1, two i tiles, three outputs; the caller's workspace is host memory too"""
    if family == "native64":
        run_native_pack(64, True, with_ws, False, only=1)
    else:
        run_prime_pack(P30, True, with_ws, False, only=1)


@pytest.mark.parametrize("with_ws", [False, True], ids=WS_IDS)
@pytest.mark.parametrize("family", ["native64", "prime32"])
def test_keyswitch_bootstrap_footprint_host_path(family, with_ws):
    run_combined(family, True, with_ws, False)
