"""One plan, many callers (include/cntt.h, "streams and threads"): every composed call of the prime and the native plans issued from
two HIP streams and from two host threads at once, a plan's first call made by four threads together, the native workspace regrown
while another stream's work is queued, two captured graphs on two clones replayed side by side, cntt_last_error per thread, and the
same plans on a second device.  The value tests call the library from one thread, on one stream, on device 0 and with the plan's tables
in place; these tests hold the words fixed (the CPU oracle or the family's big-integer model, tests/shared_plan_cases.py) and vary the
way the library is called.

Calibration.  A concurrency test that never overlaps proves nothing, so the settings were checked once against a build made wrong on
purpose (not committed): the composed prime external product (csrc/host_prime.hip, external_product_device) taking one process-wide
scratch buffer instead of its stream-ordered allocation, which keeps every address valid and removes only the ordering between
streams.  With REPS = 6, every repetition writing an output of its own and all of them compared, that build fails
    prime_ext_composed           small (5 elements): two threads            large (2 * CUs * 4 + 5): two streams and two threads
    prime_ext_16384_split_and_not  small (3 elements): two streams and two threads
and passes prime_ext_composed small on two streams (kernels that short finish before the one host thread has enqueued the other
stream's call; 32 repetitions change nothing) and the 16384 row at its large batch (2 * CUs + 5 elements) both ways.  So each regime
rejects the defect in at least one of the two tests, neither regime in every row, and a row that passes is weaker evidence about
ordering than one of those above.  The library as it is passes everything; the same settings run every family.

The ring-pack rows were calibrated the same way against a second build (not committed): ring_pack (csrc/host_prime_ring_pack.inc)
taking its digits region and its two ciphertext buffers from one process-wide allocation, made once and larger than any test needs,
whenever the caller passes no workspace.  With REPS = 6 that build fails
    prime_ring_pack              small (5 elements) and large (517): two streams and two threads
    prime_ring_pack_single       small (5 elements) and large (1541): two streams and two threads
in the first repetition every time, and passes prime_ring_pack_full both ways at both batches, as it must: that row brings one caller
workspace per concurrent call, which the changed path never sees.  No row needed more repetitions than REPS."""
import gc
import threading

import numpy as np
import pytest

import concrete_ntt_amd as cntt
import shared_plan_cases as spc
from shared_plan_cases import REPS, SETS

gpu = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def cus():
    from test_gpu_multitrip_transforms import cus as _cus
    return _cus()


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32 if a.dtype == np.uint32 else np.int64)).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def poisoned(torch, count, dtype):
    t = torch.empty(count, dtype=torch.int32 if np.dtype(dtype).itemsize == 4 else torch.int64, device="cuda")
    t.view(torch.uint8).fill_(0xA5)
    return t


def run_threads(workers):
    """start one thread per callable, join them, return the exceptions they raised"""
    errors = []

    def guard(fn):
        try:
            fn()
        except BaseException as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=guard, args=(w,)) for w in workers]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return errors


# -- the device side of one row of shared_plan_cases.ROWS --------------------------------------------------------------------------------
def make_plan(row, k=0):
    import test_gpu_native_pbs as tnp
    import test_gpu_prime_pbs as tpp
    from concrete_ntt_amd import product
    if row["fam"] == "product_ext":
        plan = product.Plan.try_new(row["n"], spc.product_modulus(), spc.PRODUCT_PRIMES)
    elif "kind" in row:
        plan = tnp.KINDS[row["kind"]].try_new(row["n"])
    else:
        plan = tpp.make_plan(spc.prime_of(row, k), row["n"])
    assert plan is not None, row["name"]
    return plan


def device_key(torch, row, plan, shared):
    """the shared arrays as the call takes them: keys transformed the way the family's header prescribes"""
    import test_gpu_native_external_product as tex
    import test_gpu_native_pbs as tnp
    import test_gpu_prime_pbs as tpp
    f, d = row["fam"], {}
    if f == "prime_ext":
        d["key"] = dev(torch, shared["key"])
    elif f == "product_ext":
        d["key"] = dev(torch, np.concatenate([pl.astype(np.uint32) for pl in shared["planes"]]).view(np.uint64))
    elif f in ("native_ext", "native_dec"):
        d["key"] = tex.key_residues(torch, plan, shared["key"], len(shared["key"]) // tex.wpp(plan))
    elif f.startswith("prime_"):
        d["key"] = tpp.key_ntt(torch, plan, shared["key"])                 # n^-1 fwd(key)
    else:
        d["key"] = tnp.key_planes(torch, plan, shared["key"])
    for name in ("lut", "ksk"):
        if name in shared:
            d[name] = dev(torch, shared[name])
    return d


def workspace_bytes(row, plan, batch):
    f = row["fam"]
    if f in ("prime_pbs", "native_pbs"):
        return plan.pbs_workspace_bytes(row["L"], row["k"], row["ell"], batch)
    if f in ("prime_kspbs", "native_kspbs"):
        return plan.ks_pbs_workspace_bytes(row["L"], row["k"], row["ell"], batch)
    if f in ("prime_pack", "native_pack"):
        return max(plan.pack_workspace_bytes(row["lin"], row["ell"], batch), 16)
    if f in ("prime_mb", "native_mb"):
        return plan.multibit_pbs_workspace_bytes(row["L"], row["k"], row["ell"], row["g"], batch)
    if f == "prime_trace":
        return plan.glwe_trace_workspace_bytes(row["k"], row["ell"], batch)
    if f == "prime_ring_pack":
        return plan.ring_pack_workspace_bytes(row["m"], row["k"], row["ell"], batch)
    if f == "prime_merge":
        return plan.glwe_merge_workspace_bytes(row["k"], row["ell"], batch)
    if f == "prime_autoks":
        return plan.glwe_automorphism_keyswitch_workspace_bytes(row["k"], row["ell"], batch)
    raise KeyError(f)


def launch(row, plan, d, s, out, ws):
    """enqueue the row's call on the current stream: d the plan's shared device arrays, s one input set"""
    f = row["fam"]
    if f == "prime_ext" or f == "native_ext":
        plan.external_product_batch(out, s["in"], d["key"], row["J"], row["O"])
    elif f == "product_ext":
        from concrete_ntt_amd import product
        plan.external_product_batch(out, s["in"], d["key"], row["J"], row["O"], product.FwdMode.Generic, product.InvMode.Replace)
    elif f == "native_dec":
        plan.external_product_decomposed_batch(out, s["in"], d["key"], row["beta"], row["ell"], row["O"], rot=s["rot"], mode="cmux")
    elif f in ("prime_pbs", "native_pbs"):
        plan.bootstrap_batch(out, s["in"], d["lut"], d["key"], row["L"], row["k"], row["beta"], row["ell"], workspace=ws)
    elif f in ("prime_kspbs", "native_kspbs"):
        plan.keyswitch_bootstrap_batch(out, s["in"], d["ksk"], row["ks_beta"], row["ks_ell"], d["lut"], d["key"], row["L"], row["k"],
                                       row["beta"], row["ell"], workspace=ws)
    elif f in ("prime_pack", "native_pack"):
        plan.pack_keyswitch_batch(out, s["in"], d["key"], row["lin"], row["m"], row["k"], row["beta"], row["ell"], workspace=ws)
    elif f in ("prime_mb", "native_mb"):
        plan.multibit_bootstrap_batch(out, s["in"], d["lut"], d["key"], row["L"], row["k"], row["beta"], row["ell"], row["g"], workspace=ws)
    elif f == "prime_trace":
        plan.glwe_trace_batch(out, s["in"], d["key"], row["steps"], row["k"], row["beta"], row["ell"], workspace=ws)
    elif f == "prime_ring_pack":
        plan.ring_pack_batch(out, s["in"], d["key"], row["m"], row["k"], row["beta"], row["ell"], workspace=ws)
    elif f == "prime_merge":
        half = s["in"].numel() // 2                                        # glwe_even of the whole batch, then glwe_odd
        plan.glwe_merge_batch(out, s["in"][:half], s["in"][half:], d["key"], row["shift"], row["t"], row["k"], row["beta"], row["ell"],
                              workspace=ws)
    elif f == "prime_autoks":
        plan.glwe_automorphism_keyswitch_batch(out, s["in"], d["key"], row["t"], row["k"], row["beta"], row["ell"], add_input=True,
                                               workspace=ws)
    else:
        raise KeyError(f)


class Case:
    """One row at one batch: the plan(s), four input sets on the device, the model's words of the sampled elements and the words of a
    serial single-stream run, itself checked against the model."""

    def __init__(self, oracle, row, batch):
        torch = _torch()
        self.row, self.batch = row, batch
        shared, sets = spc.inputs(row, batch)
        self.plans = [make_plan(row, 0), make_plan(row, 2)] if "p_odd" in row else [make_plan(row)] * 2
        self.shared = [device_key(torch, row, self.plans[0], shared[0])]
        self.shared.append(device_key(torch, row, self.plans[1], shared[1]) if "p_odd" in row else self.shared[0])
        self.sets = [{name: dev(torch, a) for name, a in s.items()} for s in sets]
        self.dtype = sets[0]["in"].dtype
        self.per = spc.in_out_words(row, batch)[1]
        self.model = [{b: spc.want(oracle, row, shared[spc.plan_index(k)], sets[k], b, batch, k) for b in spc.sampled(batch)} for k in range(SETS)]
        torch.cuda.synchronize()
        self.serial = []          # on the device: every repetition of every test is compared with it whole
        for k in range(SETS):
            out, ws = self.new_out(), self.new_ws(k)
            self.launch(k, out, ws)
            torch.cuda.synchronize()
            self.serial.append(out)
            got = host(out, self.dtype)
            assert got.any()
            for b, w in self.model[k].items():
                bad = np.nonzero(got[b * self.per:(b + 1) * self.per] != w)[0]
                assert bad.size == 0, (row["name"], batch, "serial run against the model: set", k, "element", b, "first bad word", int(bad[0]),
                                       int(bad.size))

    def new_out(self):
        return poisoned(_torch(), self.batch * self.per, self.dtype)

    def new_outs(self):
        """one poisoned output per repetition and set, so that no repetition's words are overwritten before they are compared"""
        return [[self.new_out() for _ in range(SETS)] for _ in range(REPS)]

    def new_ws(self, k):
        """a caller workspace of this call's own, or None: the call allocates"""
        if not self.row["ws"]:
            return None
        torch = _torch()
        return torch.zeros(workspace_bytes(self.row, self.plans[spc.plan_index(k)], self.batch), dtype=torch.uint8, device="cuda")

    def launch(self, k, out, ws):
        i = spc.plan_index(k)
        launch(self.row, self.plans[i], self.shared[i], self.sets[k], out, ws)

    def check(self, outs, tag):
        """every repetition's output of every set equals the serial run, which equals the model on the sampled elements"""
        torch = _torch()
        for rep in range(REPS):
            for k in range(SETS):
                if torch.equal(outs[rep][k], self.serial[k]):
                    continue
                got, want = host(outs[rep][k], self.dtype), host(self.serial[k], self.dtype)
                bad = np.nonzero(got != want)[0]
                raise AssertionError((self.row["name"], self.batch, tag, "repetition", rep, "set", k, "first bad word", int(bad[0]),
                                      "element", int(bad[0]) // self.per, "bad words", int(bad.size)))


@pytest.fixture(scope="module", params=spc.REGIMES, ids=lambda p: "%s-%s" % p)
def case(request, oracle):
    name, regime = request.param
    row = spc.BY_NAME[name]
    c = Case(oracle, row, spc.batch_of(row, regime, cus()))
    yield c
    del c
    gc.collect()


# -- 1. two streams, one thread -----------------------------------------------------------------------------------------------------------
@gpu
def test_two_streams(case):
    """the four sets interleaved over two streams REPS times without a host synchronisation in between: stream t runs the sets t and
    t + 2, which in the 16384 row are one set of each plan; every repetition writes an output of its own"""
    torch = _torch()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = case.new_outs()
    wss = [case.new_ws(k) for k in range(SETS)]
    torch.cuda.synchronize()
    for rep in range(REPS):
        for k in range(SETS):
            with torch.cuda.stream(streams[k % 2]):
                case.launch(k, outs[rep][k], wss[k])
    torch.cuda.synchronize()
    case.check(outs, "streams")


# -- 2. two host threads, each on its own stream ------------------------------------------------------------------------------------------
@gpu
def test_two_threads(case):
    """thread t runs the sets t and t + 2 on its own stream; in the 16384 row that is one set of each plan, so both threads alternate
    between the class that splits three outputs and the one that does not (ext_split_wins, a thread-local set per call) while the
    other thread does the same on the same two plans"""
    torch = _torch()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = case.new_outs()
    wss = [case.new_ws(k) for k in range(SETS)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(2)

    def worker(t):
        def run():
            barrier.wait()
            with torch.cuda.stream(streams[t]):
                for rep in range(REPS):
                    for k in (t, t + 2):
                        case.launch(k, outs[rep][k], wss[k])
        return run

    errors = run_threads([worker(0), worker(1)])
    torch.cuda.synchronize()
    assert not errors, errors
    case.check(outs, "threads")


# -- 3. a plan's first call, made by four threads at once ---------------------------------------------------------------------------------
FIRST = 4


def race_first_call(torch, plan, call, inputs, verify):
    """FIRST threads meet at a barrier and each makes the plan's first call on its own stream and buffers; then a clone calls once
    more.  A prime plan's clone shares the raced cache (cntt_prime*_plan_clone copies the plan and its shared_ptr), a native plan's clone
    is a new plan with tables of its own (cntt_native_plan_clone), so there the call shows only that a clone made after the race works"""
    barrier = threading.Barrier(FIRST)
    streams = [torch.cuda.Stream() for _ in range(FIRST)]
    results = [None] * FIRST

    def worker(t):
        def run():
            barrier.wait()
            with torch.cuda.stream(streams[t]):
                results[t] = call(plan, inputs[t])
        return run

    torch.cuda.synchronize()
    errors = run_threads([worker(t) for t in range(FIRST)])
    torch.cuda.synchronize()
    assert not errors, errors
    for t in range(FIRST):
        verify(t, results[t])
    again = call(plan.clone(), inputs[0])
    torch.cuda.synchronize()
    verify(0, again)


@gpu
@pytest.mark.parametrize("p,n", [(spc.P62, 1024), (spc.P30, 1024), (spc.P50, 1024), (spc.PM64, 1024)])
def test_first_transform_raced(oracle, p, n):
    """device_tables (csrc/host_prime.hip): the twiddle upload of a fresh plan, P50 and PM64 with the second pair of tables (fwd_fp)"""
    import test_gpu_prime_pbs as tpp
    torch = _torch()
    bits, batch = 64 if spc.is64(p) else 32, 3
    ref = oracle.Plan.try_new(n, p, bits)
    words = [oracle.fill_uniform(batch * n, p, 500 + t, bits) for t in range(FIRST)]
    want = []
    for w in words:
        x = w.copy()
        ref.fwd_batch(x)
        want.append(x)
    inputs = [dev(torch, w) for w in words]

    def call(plan, x):
        y = x.clone()
        plan.fwd_batch(y)
        return y

    race_first_call(torch, tpp.make_plan(p, n), call, inputs,
                    lambda t, y: np.testing.assert_array_equal(host(y, spc.pdt(p)), want[t], err_msg="thread %d" % t))


@gpu
@pytest.mark.parametrize("p", [spc.P62, spc.P30])
def test_first_ring_pack_raced(oracle, p):
    """device_tables again, but built under the race by ring_pack_batch: the plan's first call launches the three tree stages and the
    three trace steps of the prime_ring_pack shape (n = 64, M = 8, per-call allocation) right behind the upload, seven dependent
    steps with the embedding.  The keys are transformed on a second plan of the same prime and size, so the plan under test makes no
    call before the race.  Every thread packs a batch of its own; all words against the model"""
    import test_gpu_prime_pbs as tpp
    torch = _torch()
    row = dict(spc.BY_NAME["prime_ring_pack"], p=p)
    n, m, k, batch = row["n"], row["m"], row["k"], 3
    shared = spc.shared_inputs(row)
    key = tpp.key_ntt(torch, tpp.make_plan(p, n), shared["key"])
    sets = [spc.set_inputs(row, batch, t) for t in range(FIRST)]
    per = spc.in_out_words(row, batch)[1]
    want = [np.concatenate([spc.want(oracle, row, shared, s, b, batch) for b in range(batch)]) for s in sets]
    inputs = [dev(torch, s["in"]) for s in sets]
    torch.cuda.synchronize()

    def call(plan, x):
        out = poisoned(torch, batch * per, spc.pdt(p))
        plan.ring_pack_batch(out, x, key, m, k, row["beta"], row["ell"])
        return out

    race_first_call(torch, tpp.make_plan(p, n), call, inputs,
                    lambda t, y: np.testing.assert_array_equal(host(y, spc.pdt(p)), want[t], err_msg="thread %d" % t))


@gpu
@pytest.mark.parametrize("p", [spc.P62, spc.P30])
def test_first_prime_multibit_accumulate_raced(p):
    """multibit_table (csrc/host_prime_multibit.inc: check, unlock, build, relock) and device_tables together, on both word widths"""
    import prime_multibit_model as pmm
    import test_gpu_prime_multibit as tpm
    import test_gpu_prime_pbs as tpp
    torch = _torch()
    n, g, nterms, nout, batch = 64, 2, 3, 2, 3
    plan = tpp.make_plan(p, n)
    psi = tpm.psi_of(plan)
    data, want = [], []
    for t in range(FIRST):
        rng = np.random.default_rng(spc.seed("first-mb", p, t))
        terms, key = tpm.special_words(rng, p, batch * nterms * n), tpm.special_words(rng, p, (nterms * nout << g) * n)
        rows = tpm.group_rows(rng, n, g, batch)
        want.append(pmm.model_accumulate(terms.tolist(), key.tolist(), rows.tolist(), psi, n, p, nterms, nout, g, batch))
        data.append((dev(torch, terms), dev(torch, rows), dev(torch, key)))

    def call(pl, d):
        out = poisoned(torch, batch * nout * n, spc.pdt(p))
        pl.multibit_accumulate_batch(out, d[0], d[1], d[2], nterms, nout, g)
        return out

    def verify(t, out):
        assert [int(x) for x in host(out, spc.pdt(p))] == want[t], (p, "thread", t)

    race_first_call(torch, plan, call, data, verify)


@gpu
def test_first_native_multibit_accumulate_raced():
    """the monomial tables of the native plans (csrc/host_native.hip, mono); psi_i is read from another plan of the same kind and size, so
    the plan under test makes no call before the race"""
    import native_multibit_model as nmm
    import test_gpu_native_multibit as tnm
    import test_gpu_native_pbs as tnp
    torch = _torch()
    kind, n, g, nterms, nout, batch = "native64_plan32", 64, 2, 3, 2, 3
    psis = tnm.psis_of(torch, tnp.KINDS[kind].try_new(n))
    plan = tnp.KINDS[kind].try_new(n)
    data, want = [], []
    for t in range(FIRST):
        rng = np.random.default_rng(spc.seed("first-nmb", t))
        T = [rng.integers(0, nmm.PRIMES32[i], size=batch * nterms * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
        K = [rng.integers(0, nmm.PRIMES32[i], size=(nterms * nout << g) * n, dtype=np.uint32) for i in range(plan.NPRIMES)]
        rows = rng.integers(0, 2 * n, size=g * batch, dtype=np.uint32)
        rows[0], rows[batch] = 2 * n - 1, n
        want.append([nmm.fast_accumulate_plane(T[i], K[i], rows, psis[i], n, nmm.PRIMES32[i], nterms, nout, g, batch)
                     for i in range(plan.NPRIMES)])
        data.append((tnm.planes(torch, T), dev(torch, rows), tnm.planes(torch, K)))

    def call(pl, d):
        out = [poisoned(torch, batch * nout * n, np.uint32) for _ in range(pl.NPRIMES)]
        pl.multibit_accumulate_batch(out, d[0], d[1], d[2], nterms, nout, g)
        return out

    def verify(t, out):
        for i, o in enumerate(out):
            np.testing.assert_array_equal(host(o, np.uint32), np.asarray(want[t][i], dtype=np.uint32), err_msg="thread %d plane %d" % (t, i))

    race_first_call(torch, plan, call, data, verify)


# -- 4. the native workspace regrown while another stream's work is queued ---------------------------------------------------------------
GROW = {"native128_plan32": [1, 3, 6, 12, 24], "native64_plan52": [1, 3, 9, 33, 129]}     # the oracle's time for native128 at 16384


@gpu
@pytest.mark.parametrize("kind,n,via32", [("native128_plan32", 16384, 1), ("native64_plan52", 1024, 0)])
def test_workspace_regrow_with_work_queued(oracle, kind, n, via32):
    """a fresh plan whose workspace depends on the batch under the default switches -- native128 at n = 16384: the persistent kernel
    parks tiles, one area per workgroup, min(CUs, batch) workgroups (below n = 16384 native128 runs the register-resident kernel and has
    no workspace at all); Plan52 with plan52_via32 = 0: the residue arrays of the composed pipeline, 2 * primes * batch * n words.
    Polymul batches of growing size alternate between two streams without a synchronisation, so every call needs more than the one
    before it and finds the other stream's product queued on the buffer it replaces; then the same from two threads on another fresh
    plan.  That the workspace exists and grew is read from the device's free memory around the calls (the library takes it with
    hipMalloc, outside torch's pool): it falls by at least what the last batch needs (shared_plan_cases.native_workspace_bytes)."""
    import test_gpu_native_pbs as tnp
    torch = _torch()
    grow = GROW[kind]
    need = [spc.native_workspace_bytes(kind, n, cus(), b) for b in sorted(grow + [b + 1 for b in grow])]
    assert need[0] > 0 and all(x < y for x, y in zip(need, need[1:])), need          # every call regrows
    cls = tnp.KINDS[kind]
    ref = oracle.Native(kind, n)
    wpp = n * (2 if cls.WORD == 16 else 1)
    dt = np.uint32 if cls.WORD == 4 else np.uint64
    jobs = []
    for i, batch in enumerate(grow + [b + 1 for b in grow]):          # the first half for stream 0, the second for stream 1
        lhs = oracle.fill_uniform(batch * wpp, 0, 900 + 2 * i, 8 * dt().itemsize)
        rhs = oracle.fill_uniform(batch * wpp, 0, 901 + 2 * i, 8 * dt().itemsize)
        want = np.zeros_like(lhs)
        ref.negacyclic_polymul_batch(want, lhs.copy(), rhs.copy(), batch, 16)
        jobs.append((dev(torch, lhs), dev(torch, rhs), want))
    half = len(grow)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def fresh_outs():
        return [poisoned(torch, j[2].size, dt) for j in jobs]

    def compare(outs, tag):
        for i, j in enumerate(jobs):
            np.testing.assert_array_equal(host(outs[i], dt), j[2], err_msg="%s %s job %d" % (kind, tag, i))

    with cntt.debug_switches(plan52_via32=via32):
        plan, outs = cls.try_new(n), fresh_outs()
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        for i in range(half):
            for t in range(2):
                with torch.cuda.stream(streams[t]):
                    j = jobs[t * half + i]
                    plan.negacyclic_polymul_batch(outs[t * half + i], j[0], j[1])
        torch.cuda.synchronize()
        assert free_before - torch.cuda.mem_get_info()[0] >= need[-1], (kind, "no workspace of", need[-1], "bytes was allocated")
        compare(outs, "streams")
        plan, outs = cls.try_new(n), fresh_outs()
        torch.cuda.synchronize()
        barrier = threading.Barrier(2)

        def worker(t):
            def run():
                barrier.wait()
                with torch.cuda.stream(streams[t]):
                    for i in range(half):
                        j = jobs[t * half + i]
                        plan.negacyclic_polymul_batch(outs[t * half + i], j[0], j[1])
            return run

        errors = run_threads([worker(0), worker(1)])
        torch.cuda.synchronize()
        assert not errors, errors
        compare(outs, "threads")


# -- 5. two captured graphs on two clones, replayed side by side --------------------------------------------------------------------------
@gpu
def test_two_graphs_two_clones(oracle):
    """the header's recipe for concurrent captured graphs (include/cntt.h, cntt_native_negacyclic_polymul_batch): one clone per
    concurrent stream.  Each graph is a linear chain on one stream -- a prime bootstrap with a caller workspace, then a native polymul
    whose workspace was reserved -- and the two are replayed back to back on two streams with fresh inputs between the replays.  The
    native plan is native128 at n = 16384, which parks tiles in its workspace under the default switches (the smaller sizes run the
    register-resident kernel and have none): reserve() must take at least native_workspace_bytes() from the device, read from its free
    memory, and the capture, which may not allocate, bakes that address into the graph."""
    import test_gpu_native_pbs as tnp
    torch = _torch()
    row = spc.BY_NAME["prime_bootstrap"]
    batch, replays = row["small"], 3
    shared = spc.shared_inputs(row)
    kind, n, nb = "native128_plan32", 16384, 6
    ncls, ref = tnp.KINDS[kind], oracle.Native(kind, n)
    pplans = [make_plan(row)]
    pplans.append(pplans[0].clone())
    nplans = [ncls.try_new(n)]
    nplans.append(nplans[0].clone())
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    per = spc.in_out_words(row, batch)[1]
    side = []
    for t in range(2):
        d = device_key(torch, row, pplans[t], shared)
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        nplans[t].reserve(nb)
        need = spc.native_workspace_bytes(kind, n, cus(), nb)
        assert 0 < need < spc.native_workspace_bytes(kind, n, cus(), nb + 1)
        assert free_before - torch.cuda.mem_get_info()[0] >= need, ("reserve() took no workspace of", need, "bytes")
        s = dict(d=d, lwe=dev(torch, spc.set_inputs(row, batch, 0)["in"]), out=poisoned(torch, batch * per, spc.pdt(row["p"])),
                 ws=torch.zeros(workspace_bytes(row, pplans[t], batch), dtype=torch.uint8, device="cuda"),
                 lhs=dev(torch, oracle.fill_uniform(nb * 2 * n, 0, 70 + t, 64)), rhs=dev(torch, oracle.fill_uniform(nb * 2 * n, 0, 80 + t, 64)),
                 prod=poisoned(torch, nb * 2 * n, np.uint64))
        side.append(s)

    def chain(t):
        s = side[t]
        launch(row, pplans[t], s["d"], {"in": s["lwe"]}, s["out"], s["ws"])
        nplans[t].negacyclic_polymul_batch(s["prod"], s["lhs"], s["rhs"])

    for t in range(2):          # eager warm-up: tables and kernels exist before the capture
        chain(t)
    torch.cuda.synchronize()
    graphs = []
    for t in range(2):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=streams[t]):
            chain(t)
        graphs.append(g)
    torch.cuda.synchronize()
    for r in range(replays):
        fresh = []
        for t in range(2):
            lwe = spc.set_inputs(row, batch, 1 + 2 * r + t)["in"]
            lhs, rhs = oracle.fill_uniform(nb * 2 * n, 0, 100 + 4 * r + t, 64), oracle.fill_uniform(nb * 2 * n, 0, 102 + 4 * r + t, 64)
            s = side[t]
            s["lwe"].copy_(dev(torch, lwe))
            s["lhs"].copy_(dev(torch, lhs))
            s["rhs"].copy_(dev(torch, rhs))
            s["out"].view(torch.uint8).fill_(0xA5)
            s["prod"].view(torch.uint8).fill_(0xA5)
            fresh.append((lwe, lhs, rhs))
        torch.cuda.synchronize()
        for t in range(2):
            with torch.cuda.stream(streams[t]):
                graphs[t].replay()
        torch.cuda.synchronize()
        for t in range(2):
            lwe, lhs, rhs = fresh[t]
            got = host(side[t]["out"], spc.pdt(row["p"]))
            for b in range(batch):
                want = spc.want(oracle, row, shared, {"in": lwe}, b, batch)
                np.testing.assert_array_equal(got[b * per:(b + 1) * per], want, err_msg="replay %d graph %d bootstrap element %d" % (r, t, b))
            prod = np.zeros_like(lhs)
            ref.negacyclic_polymul_batch(prod, lhs.copy(), rhs.copy(), nb, 16)
            np.testing.assert_array_equal(host(side[t]["prod"], np.uint64), prod, err_msg="replay %d graph %d polymul" % (r, t))


# -- 6. cntt_last_error is per thread (no GPU) -----------------------------------------------------------------------------------------------
def test_error_text_is_per_thread():
    """thread A keeps making a call the library refuses for its length, thread B one it refuses for a NULL plan; each reads
    cntt_last_error after every refusal and must only ever see the text its own refusal gives when made alone"""
    from concrete_ntt_amd import prime64
    from concrete_ntt_amd._lib import MEM_HOST, last_error
    L = cntt.lib()
    n = 32
    plan = prime64.Plan.try_new(n, spc.P62)
    buf = [np.zeros(n, dtype=np.uint64) for _ in range(2)]

    def wrong_length():
        return L.cntt_prime64_fwd(plan._h, buf[0].ctypes.data, n - 1)

    def null_plan():
        return L.cntt_prime64_fwd_batch(None, buf[1].ctypes.data, 1, MEM_HOST, None)

    refusals, own = [wrong_length, null_plan], []
    for fn in refusals:
        assert fn() != 0
        own.append(last_error())
    assert own[0] and own[1] and own[0] != own[1], own
    seen = [set(), set()]
    barrier = threading.Barrier(2)

    def worker(t):
        def run():
            barrier.wait()
            for _ in range(3000):
                assert refusals[t]() != 0
                seen[t].add(last_error())
        return run

    errors = run_threads([worker(0), worker(1)])
    assert not errors, errors
    assert seen[0] == {own[0]} and seen[1] == {own[1]}, seen


# -- 7. a second device --------------------------------------------------------------------------------------------------------------------------
@gpu
def test_second_device(oracle):
    """one prime and one native plan used on device 0 and on device 1 (the per-device replicas of the tables, the workspace and the
    monomial tables): a transform, a multi-bit accumulate and a polymul give the oracle's words on both; the plans are then dropped
    while device 0 is current, and device 0 still computes"""
    import prime_multibit_model as pmm
    import test_gpu_native_pbs as tnp
    import test_gpu_prime_multibit as tpm
    import test_gpu_prime_pbs as tpp
    torch = _torch()
    count = cntt.device_count()
    if count < 2:
        pytest.skip("needs two devices: cntt.device_count() == %d" % count)
    p, n, batch = spc.P62, 64, 3
    g, nterms, nout = 2, 3, 2
    kind, nn, nb = "native128_plan32", 1024, 4
    plan, nplan = tpp.make_plan(p, n), tnp.KINDS[kind].try_new(nn)
    ref, nref = oracle.Plan.try_new(n, p, 64), oracle.Native(kind, nn)
    x = oracle.fill_uniform(batch * n, p, 31, 64)
    want_fwd = x.copy()
    ref.fwd_batch(want_fwd)
    rng = np.random.default_rng(spc.seed("second-device"))
    terms, key = tpm.special_words(rng, p, batch * nterms * n), tpm.special_words(rng, p, (nterms * nout << g) * n)
    rows = tpm.group_rows(rng, n, g, batch)
    want_mb = pmm.model_accumulate(terms.tolist(), key.tolist(), rows.tolist(), tpm.psi_of(plan), n, p, nterms, nout, g, batch)
    lhs, rhs = oracle.fill_uniform(nb * 2 * nn, 0, 41, 64), oracle.fill_uniform(nb * 2 * nn, 0, 42, 64)
    want_prod = np.zeros_like(lhs)
    nref.negacyclic_polymul_batch(want_prod, lhs.copy(), rhs.copy(), nb, 4)

    def on_current_device(tag):
        y = dev(torch, x)
        plan.fwd_batch(y)
        acc = poisoned(torch, batch * nout * n, np.uint64)
        plan.multibit_accumulate_batch(acc, dev(torch, terms), dev(torch, rows), dev(torch, key), nterms, nout, g)
        prod = poisoned(torch, lhs.size, np.uint64)
        nplan.negacyclic_polymul_batch(prod, dev(torch, lhs), dev(torch, rhs))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(host(y, np.uint64), want_fwd, err_msg=tag)
        assert [int(v) for v in host(acc, np.uint64)] == want_mb, tag
        np.testing.assert_array_equal(host(prod, np.uint64), want_prod, err_msg=tag)

    on_current_device("device 0")
    with torch.cuda.device(1):
        on_current_device("device 1")
    on_current_device("device 0 again")
    assert torch.cuda.current_device() == 0
    del plan, nplan
    gc.collect()
    other = tpp.make_plan(p, n)
    y = dev(torch, x)
    other.fwd_batch(y)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(host(y, np.uint64), want_fwd, err_msg="device 0 after the plans were dropped")
