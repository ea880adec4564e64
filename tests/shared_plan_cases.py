"""Cases and expected words for the shared-plan tests (tests/test_gpu_shared_plan.py): one plan used from two streams, from two host
threads, by several first callers at once, and on a second device.  Nothing here touches the GPU.

    ROWS                  one representative shape per call family (see the table below)
    batch_of(row, regime, ncu)
    inputs(row, batch)    -> (shared, sets): the arrays every set shares (keys, table) and four independent input sets
    want(oracle, row, shared, one_set, b) -> the expected output words of batch element b, as an array of the output's dtype

Expected words come from the CPU side only: the CPU oracle or the big-integer model that the family's own value test uses, imported
from that test or its model file and not restated.  The models are slow, so the GPU tests replay the first, the second and the last
element of every set (sampled(batch)) and compare everything else with a serial single-stream run that is itself checked against the
model on the same sample -- the arrangement of WHOLE in tests/test_gpu_prime_pbs.py.

Batches.  "small": a handful of elements, so that every kernel of the call has fewer workgroups than half the CUs and the kernels of two
streams are co-resident.  "large": 2 * CUs * per_wg + 5 elements, per_wg the elements one workgroup of the family's widest kernel takes
(4096 / n for the fused products, fewer for the composed calls whose workspace grows with the batch): every grid-stride kernel walks its
grid more than twice and ends on a ragged round (per_wg = 1 at n = 4096 and 16384, where one element is a workgroup or several).
In the ring-pack, merge and Galois-keyswitch rows an element is several workgroups of the widest kernel (widest_polys: up to 64 in the
m = n packing, whose small batch of 3 is 192 workgroups and not below half the CUs); per_wg follows from the exported grid rules, with
the arithmetic in the comments of those rows and asserted in tests/test_shared_plan_cases.py.

The prime rows cover both word widths and the lazy (P62, P30), strict (P63, P31), doubles (P50, P32) and 2^64 - c (PM64) classes; the
native rows the 32-, 64- and 128-bit Plan32 kinds and one Plan52 kind on the composed path; "ws" says whether the concurrent calls
allocate per call (False: workspace=None) or bring one caller workspace per concurrent call (True).  A caller workspace is never shared
between the two sides: that is documented misuse."""
import zlib

import numpy as np

import native_multibit_model as nmm
import prime_automorphism_model as pam
import prime_multibit_model as pmm
import prime_pack_model as ppm
import prime_ring_pack_model as prm
import test_prime_pbs_model as pm
from test_prime_keyswitch_abi import model_keyswitch
from test_prime_pbs_model import P30, P32, P50, P62, P63, PM64

P31 = 2147352577                                   # 32-bit strict range
PRODUCT_PRIMES = [257, 641, 769, 1153, 1409]       # all = 1 mod 128: a product::Plan of five 32-bit primes at n = 64
REPS = 6                                           # repetitions of the interleaved calls (calibrated: see test_gpu_shared_plan.py)
SETS = 4

ROWS = [
    # -- prime plans ---------------------------------------------------------------------------------------------------------------------
    dict(name="prime_ext_fused", fam="prime_ext", p=P62, n=1024, J=6, O=2, small=5, per_wg=4, ws=False),
    dict(name="prime_ext_fused_4096", fam="prime_ext", p=P31, n=4096, J=2, O=2, small=3, per_wg=1, ws=False),
    dict(name="prime_ext_composed", fam="prime_ext", p=P63, n=1024, J=3, O=5, small=5, per_wg=4, ws=False),
    dict(name="prime_ext_16384_split_and_not", fam="prime_ext", p=P62, p_odd=P50, n=16384, J=2, O=3, small=3, per_wg=1, ws=False),
    dict(name="product_ext", fam="product_ext", n=64, J=2, O=2, small=7, per_wg=64, ws=False),
    dict(name="prime_bootstrap", fam="prime_pbs", p=PM64, n=64, L=4, k=1, beta=7, ell=3, small=5, per_wg=8, ws=True),
    dict(name="prime_ks_bootstrap", fam="prime_kspbs", p=P30, n=64, L=4, k=1, beta=7, ell=3, ks_beta=4, ks_ell=3, small=5, per_wg=8,
         ws=False),
    dict(name="prime_pack", fam="prime_pack", p=P50, n=64, lin=8, m=48, k=1, beta=7, ell=3, small=3, per_wg=2, ws=True),
    dict(name="prime_multibit_g2", fam="prime_mb", p=P62, n=64, L=4, k=1, beta=7, ell=3, g=2, small=5, per_wg=8, ws=False),
    dict(name="prime_multibit_g3", fam="prime_mb", p=P32, n=64, L=6, k=1, beta=7, ell=3, g=3, small=5, per_wg=8, ws=True),
    dict(name="prime_trace", fam="prime_trace", p=P31, n=64, steps=3, k=1, beta=7, ell=3, small=5, per_wg=8, ws=False),
    # The ring-pack, merge and Galois-keyswitch rows.  Their kernels take one workgroup per polynomial up to the cap of the exported grid
    # rules, cntt_prime_ring_pack_grid and cntt_prime_automorphism_grid: 8 workgroups per CU of a 256-CU part = 2048 at n = 64 on both
    # word widths.  The widest kernel of a row has E polynomials per batch element (widest_polys), so 2 * 256 * per_wg + 5 elements walk
    # the grid more than twice as soon as 256 * per_wg * E >= 2048, per_wg = ceil(8 / E), and the 5 further elements leave a ragged round.
    # E = (m / 2) (k + 1) = 8 in the stage-1 merge (LWE rows as leaves), three stages buf_a -> buf_b -> buf_a, three trace steps with
    # buf_b idle: per_wg = 1, 517 elements, 4136 workgroups = 2 * 2048 + 40
    dict(name="prime_ring_pack", fam="prime_ring_pack", p=P62, n=64, m=8, k=1, beta=7, ell=3, small=5, per_wg=1, ws=False),
    # m = n: no trace, the last merge writes the output.  E = 32 * 2 = 64: per_wg = 1, 517 elements, 33088 workgroups = 16 * 2048 + 320;
    # the large batch holds 4 * 8.6 MB of LWE rows and one workspace of 25.4 MB per concurrent call.  The model takes 0.2 s per element at m = 64, 3 s for
    # the three sampled elements of four sets, so the row keeps n = m = 64
    dict(name="prime_ring_pack_full", fam="prime_ring_pack", p=P32, n=64, m=64, k=1, beta=7, ell=3, small=3, per_wg=1, ws=True),
    # m = 1: no tree, the embedding into buf_a and the full trace of six steps.  E = k + 1 = 3 (the embedding and every keyswitch of
    # the trace): per_wg = 3, 1541 elements, 4623 workgroups = 2 * 2048 + 527
    dict(name="prime_ring_pack_single", fam="prime_ring_pack", p=PM64, n=64, m=1, k=2, beta=7, ell=3, small=5, per_wg=3, ws=False),
    # one tree node through the public call; the rotation by 101 is past the sign wrap at n and no multiple of the four words of a
    # 16-byte vector.  E = k + 1 = 2: per_wg = 4, 2053 elements, 4106 workgroups = 2 * 2048 + 10
    dict(name="prime_merge", fam="prime_merge", p=P30, n=64, shift=101, t=5, k=1, beta=7, ell=3, small=5, per_wg=4, ws=False),
    # the Galois keyswitch alone, input added, t = n + 1.  E = k + 1 = 3: per_wg = 3, 1541 elements, 4623 workgroups = 2 * 2048 + 527
    dict(name="prime_autoks", fam="prime_autoks", p=P63, n=64, t=65, k=2, beta=7, ell=3, small=5, per_wg=3, ws=True),
    # -- native plans --------------------------------------------------------------------------------------------------------------------
    dict(name="native_ext_fused", fam="native_ext", kind="native64_plan32", n=1024, J=4, O=2, small=5, per_wg=4, ws=False),
    dict(name="native_ext_16384", fam="native_ext", kind="native32_plan32", n=16384, J=2, O=2, small=3, per_wg=1, ws=False),
    dict(name="native_ext_plan52", fam="native_ext", kind="native64_plan52", n=1024, J=3, O=2, small=5, per_wg=4, ws=False),
    dict(name="native_decomposed", fam="native_dec", kind="native128_plan32", n=64, npolys=2, beta=8, ell=3, O=2, small=5, per_wg=8,
         ws=False),
    dict(name="native_bootstrap", fam="native_pbs", kind="native32_plan32", n=1024, L=2, k=1, beta=6, ell=3, small=5, per_wg=4, ws=True),
    dict(name="native_ks_bootstrap", fam="native_kspbs", kind="native64_plan32", n=64, L=4, k=1, beta=6, ell=3, ks_beta=4, ks_ell=3,
         small=5, per_wg=8, ws=False),
    dict(name="native_pack", fam="native_pack", kind="native32_plan32", n=64, lin=8, m=48, k=1, beta=6, ell=3, small=3, per_wg=2,
         ws=True),
    dict(name="native_multibit", fam="native_mb", kind="native64_plan32", n=64, L=4, k=1, beta=15, ell=2, g=2, small=5, per_wg=8,
         ws=False),
]
BY_NAME = {r["name"]: r for r in ROWS}
REGIMES = [(r["name"], regime) for r in ROWS for regime in ("small", "large")]


def seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def batch_of(row, regime, ncu):
    return row["small"] if regime == "small" else 2 * ncu * row["per_wg"] + 5


def widest_polys(row):
    """polynomials per batch element in the widest kernel of a ring-pack, merge or Galois-keyswitch row, one workgroup each up to the cap
    of the exported grid rule: the stage-1 merge of the packing, batch * (m / 2) * (k + 1) (without a tree, m = 1, the embedding and the
    keyswitches of the trace, batch * (k + 1)); the merge kernel and the keyswitch's gadget kernel, batch * (k + 1)"""
    return max(row.get("m", 1) // 2, 1) * (row["k"] + 1)


def sampled(batch):
    """the elements the CPU model replays: the first, the second and the last"""
    return sorted({0, min(1, batch - 1), batch - 1})


def is64(p):
    return p >= 1 << 32


def plan_index(k):
    """which of a row's two plans set k runs on.  Stream and thread t take the sets t and t + 2, so each of them uses both plans and each
    plan is used from both"""
    return k // 2


def prime_of(row, k=0):
    """the modulus set k runs on: in the 16384 row the sets 0, 1 run on a class that does not split three outputs, 2, 3 on one that does"""
    return row.get("p_odd", row["p"]) if plan_index(k) else row["p"]


def pdt(p):
    return np.uint64 if is64(p) else np.uint32


def wbits(kind):
    return 128 if "128" in kind else 64 if "64" in kind else 32


def ndt(kind):
    return np.uint32 if wbits(kind) == 32 else np.uint64


def mult(kind):
    """array elements per word"""
    return 2 if wbits(kind) == 128 else 1


def to_array(kind, ints):
    if wbits(kind) == 128:
        a = np.empty(2 * len(ints), dtype=np.uint64)
        a[0::2] = [x & (2 ** 64 - 1) for x in ints]
        a[1::2] = [x >> 64 for x in ints]
        return a
    return np.array(ints, dtype=ndt(kind))


def to_ints(kind, a):
    if wbits(kind) == 128:
        return [int(lo) | (int(hi) << 64) for lo, hi in zip(a[0::2], a[1::2])]
    return [int(x) for x in a]


def native_workspace_bytes(kind, n, ncu, batch):
    """csrc/host_native.hip, native_workspace_bytes, restated for the two shapes the regrow and graph tests use under the default
    switches: a Plan32 kind at n >= 16384 parks (primes - 1) residue tiles of n u32 words per workgroup of the persistent kernel, one
    workgroup per compute unit and at most one per product (csrc/ntt_launch.hpp, native_fused_scratch_words); a Plan52 kind on the
    composed pipeline (plan52_via32 = 0) holds both operands' residue arrays, 2 * primes * batch * n u64 words."""
    from random_cases import KIND_INFO
    nprimes, is52, _ = KIND_INFO[kind]
    if is52:
        return 2 * nprimes * batch * n * 8
    assert n >= 16384, "smaller Plan32 shapes run the register-resident kernel: no workspace"
    return min(ncu, batch) * (nprimes - 1) * n * 4


def product_modulus():
    big = 1
    for q in PRODUCT_PRIMES:
        big *= q
    return big


# -- inputs -----------------------------------------------------------------------------------------------------------------------------
def _pwords(rng, p, count):
    return rng.integers(0, p, size=count, dtype=np.uint64).astype(pdt(p))


def _nwords(rng, kind, count):
    dt = ndt(kind)
    return rng.integers(0, np.iinfo(dt).max, size=count * mult(kind), dtype=dt, endpoint=True)


def _nkey(rng, kind, count):
    if "binary" not in kind:
        return _nwords(rng, kind, count)
    a = np.zeros(count * mult(kind), dtype=ndt(kind))
    a[0::mult(kind)] = rng.integers(0, 2, size=count)
    return a


def in_out_words(row, batch):
    """(input words per set, output array elements per batch element) -- in array elements of the word dtype"""
    f, n = row["fam"], row["n"]
    k = row.get("k", 0)
    if f in ("prime_ext", "product_ext"):
        return batch * row["J"] * n, row["O"] * n
    if f == "native_ext":
        return batch * row["J"] * n * mult(row["kind"]), row["O"] * n * mult(row["kind"])
    if f == "native_dec":
        return batch * row["npolys"] * n * mult(row["kind"]), row["O"] * n * mult(row["kind"])
    m = mult(row["kind"]) if "kind" in row else 1
    if f in ("prime_pbs", "prime_mb", "native_pbs", "native_mb"):
        return batch * (row["L"] + 1) * m, (k * n + 1) * m
    if f in ("prime_kspbs", "native_kspbs"):
        return batch * (k * n + 1) * m, (k * n + 1) * m
    if f in ("prime_pack", "native_pack"):
        return batch * row["m"] * (row["lin"] + 1) * m, (k + 1) * n * m
    if f in ("prime_trace", "prime_autoks"):
        return batch * (k + 1) * n, (k + 1) * n
    if f == "prime_ring_pack":
        return batch * row["m"] * (k * n + 1), (k + 1) * n
    if f == "prime_merge":                           # glwe_even of the whole batch, then glwe_odd of the whole batch
        return 2 * batch * (k + 1) * n, (k + 1) * n
    raise KeyError(f)


def shared_inputs(row, k=0):
    """the arrays all sets of a plan share: keys in the coefficient domain (the GPU test transforms them as the header prescribes; the
    prime external products take any canonical words as key_ntt), the table, the keyswitch key"""
    f, n = row["fam"], row["n"]
    rng = np.random.default_rng(seed("shared", row["name"], plan_index(k) if "p_odd" in row else 0))
    kk = row.get("k", 0)
    s = {}
    if f == "prime_ext":
        s["key"] = _pwords(rng, prime_of(row, k), row["J"] * row["O"] * n)
    elif f == "product_ext":
        s["planes"] = [_pwords(rng, q, row["J"] * row["O"] * n).astype(np.uint64) for q in PRODUCT_PRIMES]
    elif f == "native_ext":
        s["key"] = _nkey(rng, row["kind"], row["J"] * row["O"] * n)
    elif f == "native_dec":
        s["key"] = _nkey(rng, row["kind"], row["npolys"] * row["ell"] * row["O"] * n)
    elif f in ("prime_pbs", "prime_kspbs", "prime_mb"):
        p, g = row["p"], row.get("g", 0)
        rows = (row["L"] // g if g else row["L"]) * (kk + 1) * row["ell"] * (kk + 1) << g
        s["lut"], s["key"] = _pwords(rng, p, (kk + 1) * n), _pwords(rng, p, rows * n)
        if f == "prime_kspbs":
            s["ksk"] = _pwords(rng, p, kk * n * row["ks_ell"] * (row["L"] + 1))
    elif f in ("native_pbs", "native_kspbs", "native_mb"):
        kind, g = row["kind"], row.get("g", 0)
        rows = (row["L"] // g if g else row["L"]) * (kk + 1) * row["ell"] * (kk + 1) << g
        s["lut"], s["key"] = _nwords(rng, kind, (kk + 1) * n), _nkey(rng, kind, rows * n)
        if f == "native_kspbs":
            s["ksk"] = _nwords(rng, kind, kk * n * row["ks_ell"] * (row["L"] + 1))
    elif f == "prime_pack":
        s["key"] = _pwords(rng, row["p"], row["lin"] * row["ell"] * (kk + 1) * n)
    elif f == "native_pack":
        s["key"] = _nwords(rng, row["kind"], row["lin"] * row["ell"] * (kk + 1) * n)
    elif f == "prime_trace":
        s["key"] = _pwords(rng, row["p"], row["steps"] * kk * row["ell"] * (kk + 1) * n)
    elif f == "prime_ring_pack":                     # the log2 n trace keys back to back
        s["key"] = _pwords(rng, row["p"], (n.bit_length() - 1) * kk * row["ell"] * (kk + 1) * n)
    elif f in ("prime_merge", "prime_autoks"):       # one key
        s["key"] = _pwords(rng, row["p"], kk * row["ell"] * (kk + 1) * n)
    else:
        raise KeyError(f)
    return s


def set_inputs(row, batch, k):
    """input set k of SETS: the words the call reads per batch element, plus the exponents of the decomposed product"""
    rng = np.random.default_rng(seed("set", row["name"], batch, k))
    count = in_out_words(row, batch)[0]
    if row["fam"] == "product_ext":
        s = {"in": rng.integers(0, product_modulus(), size=count, dtype=np.uint64)}
    elif "kind" in row:
        s = {"in": _nwords(rng, row["kind"], count // mult(row["kind"]))}
    else:
        s = {"in": _pwords(rng, prime_of(row, k), count)}
    if row["fam"] == "native_dec":
        n = row["n"]
        rot = rng.integers(0, 2 * n, size=batch, dtype=np.uint32)
        rot[:min(batch, 3)] = [2 * n - 1, n, 0][:min(batch, 3)]
        s["rot"] = rot
    return s


def inputs(row, batch):
    shared = [shared_inputs(row, 2 * i) for i in range(2)] if "p_odd" in row else [shared_inputs(row)] * 2
    return shared, [set_inputs(row, batch, k) for k in range(SETS)]


# -- expected words of one batch element -------------------------------------------------------------------------------------------------
def _chunks(flat, n):
    return [flat[i * n:(i + 1) * n] for i in range(len(flat) // n)]


def _prime_rotation(p, n, rot, lut, key, L, k, beta, ell):
    """the classic blind rotation of one element on Python ints (tests/test_gpu_prime_pbs.py, section 5), exact products"""
    npolys = k + 1
    acc = [pm.source(f, rot[L], p, "rotate") for f in _chunks(lut, n)]
    keyp, per = _chunks(key, n), npolys * ell * npolys
    for i in range(L):
        terms = pm.model_terms_element(acc, rot[i], p, beta, ell)
        new = []
        for o in range(npolys):
            add = [0] * n
            for j, t in enumerate(terms):
                add = [(x + y) % p for x, y in zip(add, pmm.negacyclic_fast(t, keyp[i * per + j * npolys + o], p))]
            new.append([(x + y) % p for x, y in zip(acc[o], add)])
        acc = new
    return acc


def _prime_bootstrap(row, shared, lwe):
    p, n, L, k = row["p"], row["n"], row["L"], row["k"]
    rot = pm.model_modswitch(lwe, L, 1, p, n.bit_length() - 1)
    lut, key = shared["lut"].tolist(), shared["key"].tolist()
    if "g" in row:
        acc = _chunks(pmm.model_multibit_rotate(lut, rot, key, p, n, L, k, row["beta"], row["ell"], row["g"], 1), n)
    else:
        acc = _prime_rotation(p, n, rot, lut, key, L, k, row["beta"], row["ell"])
    return pm.model_extract(acc, 0, p)


def _native_plan(kind, n):
    import test_gpu_native_pbs as tnp
    return tnp.KINDS[kind].try_new(n)


def _native_bootstrap(oracle, row, shared, lwe):
    import test_gpu_native_pbs as tnp
    from test_gpu_random_fhe import native_iteration
    kind, n, L, k, beta, ell = (row[x] for x in ("kind", "n", "L", "k", "beta", "ell"))
    w = wbits(kind)
    rot = tnp.model_modswitch(lwe, L, 1, w, n.bit_length() - 1)
    lut, key = to_ints(kind, shared["lut"]), to_ints(kind, shared["key"])
    if "g" in row:
        acc = _chunks(nmm.model_multibit_rotate(lut, rot, key, w, n, L, k, beta, ell, row["g"], 1), n)
    else:
        plan, ref = _native_plan(kind, n), oracle.Native(kind, n)
        acc = [tnp.source(f, rot[L], w, "rotate") for f in _chunks(lut, n)]
        keyp, per = _chunks(key, n), (k + 1) * ell * (k + 1)
        for i in range(L):
            acc = native_iteration(ref, plan, acc, rot[i], keyp[i * per:(i + 1) * per], w, beta, ell)
    return tnp.model_extract(acc, 0, w)


def want(oracle, row, shared, one_set, b, batch, k=0):
    """expected output words of element b of one input set (shared: the arrays of the plan that set runs on)"""
    f, n = row["fam"], row["n"]
    per_in = in_out_words(row, batch)[0] // batch
    x = one_set["in"][b * per_in:(b + 1) * per_in]
    if f == "prime_ext":
        from test_external_product import _expected
        p = prime_of(row, k)
        oplan = oracle.Plan.try_new(n, p, 64 if is64(p) else 32)
        return _expected(oplan, x.copy(), shared["key"], None, n, row["J"], row["O"], 1, p, False)
    if f == "product_ext":
        J, O, big = row["J"], row["O"], product_modulus()
        oplan = oracle.Product.try_new(n, big, PRODUCT_PRIMES)
        dl = oplan.ntt_domain_len()
        acc = [np.zeros(dl, dtype=np.uint64) for _ in range(O)]
        for j in range(J):
            t = np.zeros(dl, dtype=np.uint64)
            oplan.fwd(t, x[j * n:(j + 1) * n].copy())
            for o in range(O):
                i = j * O + o
                kp = np.concatenate([pl[i * n:(i + 1) * n].astype(np.uint32) for pl in shared["planes"]]).view(np.uint64)
                oplan.mul_accumulate(acc[o], t, kp)
        out = np.zeros(O * n, dtype=np.uint64)
        for o in range(O):
            r = np.zeros(n, dtype=np.uint64)
            oplan.inv(r, acc[o], False)
            out[o * n:(o + 1) * n] = r
        return out
    if f == "native_ext":
        import test_gpu_native_external_product as tex
        plan = _native_plan(row["kind"], n)
        return tex.expected(oracle, row["kind"], plan, x.copy(), shared["key"], 1, row["J"], row["O"])
    if f == "native_dec":
        import test_gpu_native_gadget as tg
        kind = row["kind"]
        plan = _native_plan(kind, n)
        terms = tg.model_terms([_chunks(to_ints(kind, x), n)], [int(one_set["rot"][b])], wbits(kind), row["beta"], row["ell"], "cmux")[0]
        outs = tg.oracle_element(oracle, kind, plan, terms, _chunks(to_ints(kind, shared["key"]), n), row["O"])
        return to_array(kind, [v for o in outs for v in o])
    if f in ("prime_pbs", "prime_mb"):
        return np.array(_prime_bootstrap(row, shared, x.tolist()), dtype=pdt(row["p"]))
    if f == "prime_kspbs":
        p, L = row["p"], row["L"]
        mid = model_keyswitch(x.tolist(), shared["ksk"].tolist(), p, row["k"] * n, L, L + 1, row["ks_beta"], row["ks_ell"], 1)
        return np.array(_prime_bootstrap(row, shared, mid), dtype=pdt(p))
    if f in ("native_pbs", "native_mb"):
        return to_array(row["kind"], _native_bootstrap(oracle, row, shared, to_ints(row["kind"], x)))
    if f == "native_kspbs":
        import test_gpu_native_keyswitch as tks
        kind, L = row["kind"], row["L"]
        mid = tks.model_keyswitch_batch(to_ints(kind, x), to_ints(kind, shared["ksk"]), row["k"] * n, L, L + 1, wbits(kind), row["ks_beta"],
                                        row["ks_ell"], 1)
        return to_array(kind, _native_bootstrap(oracle, row, shared, mid))
    if f == "prime_pack":
        p = row["p"]
        out = ppm.model_pack_batch(x.tolist(), shared["key"].tolist(), p, row["lin"], row["m"], row["k"], n, row["beta"], row["ell"], 1)
        return np.array([int(v) for v in out], dtype=pdt(p))
    if f == "native_pack":
        import test_gpu_native_pack as tpk
        kind = row["kind"]
        out = tpk.model_pack_batch(to_ints(kind, x), to_ints(kind, shared["key"]), row["lin"], row["m"], row["k"], n, wbits(kind), row["beta"],
                                   row["ell"], 1)
        return to_array(kind, [int(v) for v in out])
    if f == "prime_trace":
        p = row["p"]
        out = pam.model_trace(x.tolist(), shared["key"].tolist(), p, row["steps"], row["k"], n, row["beta"], row["ell"])
        return np.array(out, dtype=pdt(p))
    if f == "prime_ring_pack":
        p, m, k = row["p"], row["m"], row["k"]
        out = prm.model_ring_pack(_chunks(x.tolist(), k * n + 1), shared["key"].tolist(), p, m, k, n, row["beta"], row["ell"])
        return np.array(out, dtype=pdt(p))
    if f == "prime_merge":
        p, k = row["p"], row["k"]
        ct = (k + 1) * n
        E, O = (one_set["in"][(h * batch + b) * ct:(h * batch + b + 1) * ct].tolist() for h in range(2))
        out = prm.model_merge(E, O, shared["key"].tolist(), p, row["shift"], row["t"], k, n, row["beta"], row["ell"])
        return np.array(out, dtype=pdt(p))
    if f == "prime_autoks":
        p = row["p"]
        out = pam.model_autoks_batch(x.tolist(), shared["key"].tolist(), p, row["t"], row["k"], n, row["beta"], row["ell"], True, 1)
        return np.array(out, dtype=pdt(p))
    raise KeyError(f)
