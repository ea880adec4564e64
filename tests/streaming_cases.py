"""Shape calculator of tests/test_gpu_prime_streaming.py: the cases that put the automorphism, Galois-keyswitch, merge, ring-pack and
multi-bit set-up kernels on their STREAM = true form.  The host picks that form per launch with `bytes > STREAM_BYTES`
(csrc/host_common.hpp); this module restates the constant and the byte count of every launch site

    host_prime_automorphism.inc  automorphism_device   2 * polys * n * word                       autom_bytes
    host_prime_automorphism.inc  autoks_device         batch * k * levels * n * word              digit_bytes   (every trace step too)
    host_prime_ring_pack.inc     merge_device          nct * k * levels * n * word                digit_bytes   (nct: the tree level's)
    multibit_host.hpp            multibit_rotate_device<PrimePbs<T>>  batch * (k + 1) * n * word      acc_bytes
    multibit_host.hpp            multibit_rotate_device<NativePbs>    the same with the native word   acc_bytes

and returns, for each GPU case, the full call's shape with the bytes of each of its launches, the same at one batch element fewer, the
shapes of the reference calls with theirs, and the buffers the test holds on the device.  Pure: no GPU, no plan, no state of the
library.  tests/test_streaming_cases.py asserts, without a GPU, that every full call sits on its first streaming batch, that no
reference launch streams, that a case stays within MEM_CAP and that the calls accept its arguments.  Not a test module."""
from test_prime_pbs_model import P30, P62

STREAM_BYTES = 384 << 20      # the library's streaming threshold (host_common.hpp)
MEM_CAP = 4 << 30             # device bytes one GPU case may hold
NATIVE64 = "native64_plan32"  # the 64-bit native kind of the multi-bit set-up case (KINDS of tests/test_gpu_native_pbs.py)


def up256(x):
    return (x + 255) // 256 * 256


def word_bytes(p):
    return 8 if p >= 1 << 32 else 4


def streams(nbytes):
    return nbytes > STREAM_BYTES


# -- the byte counts the launch sites compare with STREAM_BYTES ----------------------------------------------------------------------------
def autom_bytes(polys, n, word):
    return 2 * polys * n * word


def digit_bytes(nct, k, levels, n, word):
    return nct * k * levels * n * word


def acc_bytes(batch, k, n, word):
    return batch * (k + 1) * n * word


def gadget_bytes(polys, levels, n, word):
    """gadget_decompose_batch (host_prime_pbs.inc): a call of the per-element composition"""
    return polys * levels * n * word


def first_streaming(unit):
    """the first count whose count * unit bytes exceed the threshold"""
    return STREAM_BYTES // unit + 1


def halves(batch):
    return [batch // 2, batch - batch // 2]


# -- the launches of one call: (label, bytes) ----------------------------------------------------------------------------------------------
def automorphism_launches(n, word, polys):
    return [("automorphism", autom_bytes(polys, n, word))]


def autoks_launches(n, word, k, levels, batch, steps=1):
    return [("keyswitch step %d" % r, digit_bytes(batch, k, levels, n, word)) for r in range(steps)]


def merge_launches(n, word, k, levels, batch):
    return [("merge", digit_bytes(batch, k, levels, n, word))]


def ring_pack_launches(n, word, m, k, levels, batch):
    """ring_pack_device: tree level s = 1 .. log2 m merges batch * m / 2^s ciphertexts (level 1 reads the LWE rows as leaves), then the
    trace of log2 n - log2 m steps runs on batch ciphertexts"""
    logn, l = n.bit_length() - 1, m.bit_length() - 1
    out = [("tree level %d%s" % (s, " (leaf)" if s == 1 else ""), digit_bytes(batch * (m >> s), k, levels, n, word)) for s in range(1, l + 1)]
    return out + [("trace step %d" % r, digit_bytes(batch, k, levels, n, word)) for r in range(logn - l)]


def setup_launches(n, word, k, batch):
    return [("set-up", acc_bytes(batch, k, n, word))]


def composition_launches(n, word, k, levels, batch, with_automorphism=True):
    """the public calls of one Galois keyswitch or one merge on `batch` ciphertexts: automorphism_batch on the polynomials it permutes,
    gadget_decompose_batch(plain) on the k mask polynomials, the digits of the external product"""
    out = [("composition: automorphism_batch", autom_bytes(batch * (k + 1), n, word))] if with_automorphism else []
    return out + [("composition: gadget_decompose_batch", gadget_bytes(batch * k, levels, n, word)),
                  ("composition: external_product_batch terms", digit_bytes(batch, k, levels, n, word))]


def compose_pack_launches(n, word, m, k, levels, batch):
    """embed -> one glwe_merge_batch per stage on batch * h pairs -> glwe_trace_batch (compose_pack of tests/test_gpu_prime_ring_pack.py)"""
    return ring_pack_launches(n, word, m, k, levels, batch)


# -- the buffers a GPU case holds: (label, bytes) --------------------------------------------------------------------------------------------
def ring_pack_workspace(n, word, m, k, levels, batch):
    h, q, ct = max(m // 2, 1), max(m // 4, 1), (k + 1) * n * word
    return up256(batch * h * k * levels * n * word) + up256(batch * h * ct) + up256(batch * q * ct)


def generated(count, word):
    """device_words draws 64-bit integers and narrows them for the 32-bit plans: the draw lives beside the words for a moment"""
    return count * 8 if word == 4 else 0


def key_bytes(n, word, k, levels, keys=1):
    return keys * k * levels * (k + 1) * n * word


def automorphism_buffers(c):
    n, w, polys = c["n"], c["word"], c["batch"]
    return [("in", polys * n * w), ("the draw", generated(polys * n, w)), ("out", polys * n * w), ("out of a half", max(halves(polys)) * n * w)]


def autoks_buffers(c):
    n, w, k, L, b = c["n"], c["word"], c["k"], c["levels"], c["batch"]
    ct, hb = (k + 1) * n * w, max(halves(b))
    bufs = [("glwe_in", b * ct), ("the draw", generated(b * (k + 1) * n, w)), ("glwe_out", b * ct), ("workspace", up256(digit_bytes(b, k, L, n, w))),
            ("key and its coefficient form", 2 * key_bytes(n, w, k, L, c["steps"])), ("out of a half", c["steps"] * hb * ct),
            ("the library's workspace of a half", up256(digit_bytes(hb, k, L, n, w)))]
    if c["call"] == "trace":
        bufs.append(("second ciphertext of the trace", up256(b * ct)))
    else:   # one element through the public calls: in, out, permuted masks, digits twice
        bufs.append(("composition of one element", (2 * (k + 1) + k + 2 * k * L) * n * w))
    return bufs


def merge_buffers(c):
    n, w, k, L, b = c["n"], c["word"], c["k"], c["levels"], c["batch"]
    ct, hb = (k + 1) * n * w, max(halves(b))
    return [("even, odd", 2 * b * ct), ("the draws", generated(b * (k + 1) * n, w)), ("glwe_out", b * ct), ("workspace", up256(digit_bytes(b, k, L, n, w))),
            ("key and its coefficient form", 2 * key_bytes(n, w, k, L)), ("out of a half", hb * ct),
            ("the library's workspace of a half", up256(digit_bytes(hb, k, L, n, w))),
            ("composition of one element", (4 * (k + 1) + k + 2 * k * L) * n * w)]


def ring_pack_buffers(c):
    n, w, k, L, b, m = c["n"], c["word"], c["k"], c["levels"], c["batch"], c["lwe_count"]
    ct, row, cb, logn = (k + 1) * n * w, (k * n + 1) * w, max(c["chunks"]), n.bit_length() - 1
    h = max(m // 2, 1)
    # compose_pack on a chunk, stage by stage; the largest stage counts (the buffers of a stage are freed before the next)
    embed = cb * m * (row + ct)
    merge = 3 * cb * h * ct + up256(digit_bytes(cb * h, k, L, n, w))
    trace = 2 * cb * ct + up256(digit_bytes(cb, k, L, n, w)) + up256(cb * ct)
    return [("lwe_in", b * m * row), ("the draw", generated(b * m * (k * n + 1), w)), ("glwe_out", b * ct),
            ("workspace", ring_pack_workspace(n, w, m, k, L, b)), ("keys and their coefficient form", 2 * key_bytes(n, w, k, L, logn)),
            ("out of a chunk", cb * ct), ("the library's workspace of a chunk", ring_pack_workspace(n, w, m, k, L, cb)),
            ("composition of a chunk", max(embed, merge, trace))]


def setup_buffers(c):
    n, w, k, b = c["n"], c["word"], c["k"], c["batch"]
    lut = (b if c["lut_per_element"] else 1) * (k + 1) * n
    return [("acc", acc_bytes(b, k, n, w)), ("lut", lut * w), ("the draw", generated(lut, w)), ("rot", 4 * b), ("acc of a half", acc_bytes(max(halves(b)), k, n, w))]


# -- the cases -------------------------------------------------------------------------------------------------------------------------------
def _case(name, call, p, n, k, base_log, levels, batch, launches, references, buffers, **more):
    """launches: batch -> [(label, bytes)] of the full call; references: [(call, batch, launches)]"""
    c = {"name": name, "call": call, "p": p, "n": n, "word": more.pop("word", None) or word_bytes(p), "k": k, "base_log": base_log,
         "levels": levels, "batch": batch, "steps": 1, "lwe_count": 1, "ts": [], "shifts": [], "lds": (1, 0)}
    c.update(more)
    c["launches"] = launches(batch)
    c["below"] = launches(batch - 1)
    c["references"] = [{"call": rc, "batch": rb, "launches": rl} for rc, rb, rl in references]
    c["device_buffers"] = buffers(c)
    c["device_bytes"] = sum(x for _, x in c["device_buffers"])
    return c


def _automorphism(name, p, n, ts, lds=(1, 0)):
    w = word_bytes(p)
    polys = first_streaming(2 * n * w)
    refs = [("automorphism (half)", h, automorphism_launches(n, w, h)) for h in halves(polys)]
    return _case(name, "automorphism", p, n, 0, 0, 0, polys, lambda b: automorphism_launches(n, w, b), refs, automorphism_buffers, ts=ts, lds=lds)


def _levels(p, base_log):
    """the largest level count the calls accept for the prime (base_log * levels <= the bit length of p), up to 15"""
    return min(15, p.bit_length() // base_log)


def _autoks(name, p, n, k, base_log, ts):
    w, levels = word_bytes(p), _levels(p, base_log)
    batch = first_streaming(k * levels * n * w)
    refs = [("keyswitch (half)", h, autoks_launches(n, w, k, levels, h)) for h in halves(batch)]
    refs.append(("keyswitch through the public calls (one element)", 1, composition_launches(n, w, k, levels, 1)))
    return _case(name, "autoks", p, n, k, base_log, levels, batch, lambda b: autoks_launches(n, w, k, levels, b), refs, autoks_buffers, ts=ts)


def _trace(name, p, n, k, base_log, steps):
    w, levels = word_bytes(p), _levels(p, base_log)
    batch = first_streaming(k * levels * n * w)
    refs = [("keyswitch (half), step %d" % r, h, autoks_launches(n, w, k, levels, h)) for h in halves(batch) for r in range(steps)]
    return _case(name, "trace", p, n, k, base_log, levels, batch, lambda b: autoks_launches(n, w, k, levels, b, steps), refs, autoks_buffers,
                 steps=steps, ts=[(n >> r) + 1 for r in range(steps)])


def _merge(name, p, n, k, base_log, ts):
    w, levels = word_bytes(p), _levels(p, base_log)
    batch = first_streaming(k * levels * n * w)
    refs = [("merge (half)", h, merge_launches(n, w, k, levels, h)) for h in halves(batch)]
    refs.append(("merge through the public calls (one element)", 1, composition_launches(n, w, k, levels, 1)))
    return _case(name, "merge", p, n, k, base_log, levels, batch, lambda b: merge_launches(n, w, k, levels, b), refs, merge_buffers, ts=ts,
                 shifts=[1, n // 2])


def _ring_pack(name, p, n, k, base_log, m, expect):
    """batch: the first at which the leaf level (batch * m / 2 ciphertexts) streams; expect: which launches of the full call stream"""
    w, levels = word_bytes(p), _levels(p, base_log)
    h = m // 2
    batch = -(-first_streaming(k * levels * n * w) // h)
    chunks = halves(batch)
    refs = [("ring_pack (chunk)", cb, ring_pack_launches(n, w, m, k, levels, cb)) for cb in chunks]
    refs += [("embed, merges and trace (chunk)", cb, compose_pack_launches(n, w, m, k, levels, cb)) for cb in chunks]
    return _case(name, "ring_pack", p, n, k, base_log, levels, batch, lambda b: ring_pack_launches(n, w, m, k, levels, b), refs, ring_pack_buffers,
                 lwe_count=m, chunks=chunks, expect=expect)


def _setup(name, call, p, n, k, word, kind=None, lut_per_element=False):
    batch = first_streaming((k + 1) * n * word)
    refs = [("set-up (half)", h, setup_launches(n, word, k, h)) for h in halves(batch)]
    return _case(name, call, p, n, k, 7, 3, batch, lambda b: setup_launches(n, word, k, b), refs, setup_buffers, word=word, grouping=2, kind=kind,
                 lut_per_element=lut_per_element, lds=(None,))


def _cases():
    n = 1024
    cs = [_automorphism("autom-p62-1024", P62, n, [3, n + 1]),
          _automorphism("autom-p30-1024", P30, n, [2 * n - 1, 3]),
          _automorphism("autom-p62-16384", P62, 16384, [16384 + 1, 2 * 16384 - 1], lds=(1,)),      # past the LDS limit: the global gather
          _autoks("autoks-p62-k1", P62, n, 1, 4, [3, 2 * n - 1]),
          _autoks("autoks-p30-k2", P30, n, 2, 2, [n + 1, 3]),
          _trace("trace-p62-k1", P62, n, 1, 4, 2),
          _merge("merge-p62-k1", P62, n, 1, 4, [n + 1, 3]),
          _merge("merge-p30-k2", P30, n, 2, 2, [2 * n - 1, n + 1]),
          _ring_pack("ringpack-p62-m2", P62, n, 1, 4, 2, expect="every launch"),
          _ring_pack("ringpack-p62-m4", P62, n, 1, 4, 4, expect="the leaf level only"),
          _setup("multibit-setup-p62", "prime_multibit_setup", P62, n, 1, 8, lut_per_element=True),
          _setup("multibit-setup-native64", "native_multibit_setup", None, n, 1, 8, kind=NATIVE64)]
    return cs


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}


def gpu_cases(call):
    """(case, autom_lds setting) of every GPU case of one call"""
    return [(c, lds) for c in CASES if c["call"] == call for lds in c["lds"]]


def case_id(param):
    return param["name"] if isinstance(param, dict) else "lds%s" % param


# -- what the calls check before they launch -------------------------------------------------------------------------------------------------
def refusals(c):
    """the argument checks of the calls (gadget_check, autom_check_t, ring_check_sizes and the shift bound) a case or one of its references
    would fail: empty when the calls accept it"""
    bad = []
    n, k, L = c["n"], c["k"], c["levels"]
    if c["call"] in ("autoks", "trace", "merge", "ring_pack", "prime_multibit_setup", "native_multibit_setup"):
        width = c["p"].bit_length() if c["p"] else 8 * c["word"]
        if not (c["base_log"] >= 1 and L >= 1 and c["base_log"] * L <= width):
            bad.append("base_log * levels = %d * %d exceeds %d bits" % (c["base_log"], L, width))
    for t in c["ts"]:
        if t % 2 == 0 or not 0 < t < 2 * n:
            bad.append("t = %d is not an odd exponent below 2n" % t)
    for s in c["shifts"]:
        if not 0 <= s < 2 * n:
            bad.append("shift = %d is not below 2n" % s)
    m = c["lwe_count"]
    if m < 1 or m & (m - 1) or m > n:
        bad.append("lwe_count = %d" % m)
    per = max(m // 2, 1)
    if c["call"] in ("autoks", "trace", "merge", "ring_pack"):
        for batch in [c["batch"]] + [r["batch"] for r in c["references"]]:
            if batch * per * max(k * L, k + 1) >= 1 << 32:
                bad.append("batch %d: too large for one launch" % batch)
    if c["call"].endswith("multibit_setup"):
        if not 1 <= c["grouping"] <= 4:
            bad.append("grouping = %d" % c["grouping"])
        if c["batch"] * (k + 1) * L >= 1 << 32:
            bad.append("batch %d: too large for one transform launch" % c["batch"])
    return bad
