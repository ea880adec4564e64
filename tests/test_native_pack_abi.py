"""C ABI of the LWE-to-GLWE packing keyswitch (include/cntt_pack.h through include/cntt_ext.h): the header is plain C11, its two names
are declared through cntt_ext.h (after cntt_keyswitch.h) and exported, every CNTT_EINVAL case is refused on host buffers by the
argument checks that precede any device call (output untouched, argument named), pack_workspace_bytes is the header's formula, the
Python wrappers panic on bad shapes, the code object of the new unit has six kernels without scratch or spills -- and the plain-int
model of the packing keyswitch (digits, transpose, negacyclic sums: the header's formula to the letter) is checked here against the
phase identity the header states, together with the matrix form of it that tests/test_gpu_native_pack.py compares the device with.
No GPU needed."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import concrete_ntt_amd as cntt
from concrete_ntt_amd import native32, native64, native128
from concrete_ntt_amd._lib import EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT = os.path.join(ROOT, "include", "cntt_ext.h")
PACK = os.path.join(ROOT, "include", "cntt_pack.h")
NEW = {"cntt_native_pack_keyswitch_batch", "cntt_native_pack_workspace_bytes"}
PACK_TERMS = int(re.search(r"#define\s+CNTT_PACK_TERMS\s+(\d+)", open(PACK).read()).group(1))


# -- the model ---------------------------------------------------------------------------------------------------------------------
def digits(x, w, beta, ell):
    """the signed digits of cntt_gadget.h, d_1 first"""
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


def rounded(x, w, beta, ell):
    """r of cntt_gadget.h: the (beta * ell)-bit number closest to x / 2^s, ties up, wrapping at the top"""
    s = w - beta * ell
    return (x if s == 0 else ((x + (1 << (s - 1))) % (1 << w)) >> s) % (1 << (beta * ell))


def negacyclic(a, b, n):
    """a (*) b in Z[X]/(X^n + 1), Python ints"""
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                if i + j < n:
                    out[i + j] += x * y
                else:
                    out[i + j - n] -= x * y
    return out


def model_pack_literal(lwe, key, lin, m, k, n, w, beta, ell):
    """The header's formula to the letter for one batch element.  lwe: m * (lin + 1) ints; key: lin * ell * (k + 1) polynomials of n
    ints, K[r][p] at (r * (k + 1) + p) * n -> (k + 1) * n ints."""
    M = 1 << w
    out = [[0] * n for _ in range(k + 1)]
    for t in range(m):
        out[k][t] = lwe[t * (lin + 1) + lin]
    for i in range(lin):
        dig = [digits(lwe[t * (lin + 1) + i], w, beta, ell) for t in range(m)]
        for l in range(ell):
            D = [dig[t][l] for t in range(m)] + [0] * (n - m)              # the transpose: coefficient t from ciphertext t
            for p in range(k + 1):
                base = ((i * ell + l) * (k + 1) + p) * n
                for c, v in enumerate(negacyclic(D, key[base:base + n], n)):
                    out[p][c] -= v
    return [v % M for row in out for v in row]


def model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, batch, dtype=object):
    """The same words as one matrix product per batch element (restated in tests/test_gpu_native_pack.py): row t of D K is
    sum_r d_r(lwe_t) K[r], the output is the body polynomial minus sum_t X^t (row t).  dtype object: Python ints, reduced at the end;
    np.uint32 / np.uint64 for w = 32 / 64: the arithmetic wraps modulo 2^w by itself."""
    M = 1 << w
    Kmat = np.array(key, dtype=dtype).reshape(lin * ell, (k + 1) * n) if lin else None
    out = []
    for g in range(batch):
        cts = lwe[g * m * (lin + 1):(g + 1) * m * (lin + 1)]
        acc = np.zeros((k + 1, n), dtype=dtype)
        if lin:
            D = np.array([[d if dtype is object else d % M for i in range(lin) for d in digits(cts[t * (lin + 1) + i], w, beta, ell)]
                          for t in range(m)], dtype=dtype)
            A = D.dot(Kmat).reshape(m, k + 1, n)
            for t in range(m):                                             # acc -= X^t A[t]
                acc[:, t:] -= A[t][:, :n - t]
                if t:
                    acc[:, :t] += A[t][:, n - t:]
        acc[k, :m] += np.array([cts[t * (lin + 1) + lin] for t in range(m)], dtype=dtype)
        out += [int(x) % M for x in acc.reshape(-1)]
    return out


def rand_word(rng, w):
    return int.from_bytes(rng.bytes(w // 8), "little")


def noise_free_key(rng, s_in, S, k, n, w, beta, ell):
    """row (i, l): uniform mask polynomials, body = sum_q A_q (*) S_q + s_in[i] 2^(w - beta l) at coefficient 0"""
    M, key = 1 << w, []
    for i in range(len(s_in)):
        for l in range(1, ell + 1):
            body = [0] * n
            for q in range(k):
                a = [rand_word(rng, w) for _ in range(n)]
                key += a
                body = [(x + y) % M for x, y in zip(body, negacyclic(a, S[q], n))]
            body[0] = (body[0] + s_in[i] * (1 << (w - beta * l))) % M
            key += body
    return key


@pytest.mark.parametrize("w,beta,ell", [(32, 8, 4), (32, 5, 3), (64, 16, 4), (64, 4, 3), (64, 31, 2), (64, 33, 1), (128, 16, 8), (128, 7, 5),
                                        (32, 1, 9)])
def test_model_satisfies_the_phase_identity_of_the_header(w, beta, ell):
    """n = 16, k = 1 and 2, m = 5 and n: with a noise-free key the phase of the model's output under the output key is
    sum_t X^t (body_t - sum_i s_in[i] r_{t,i} 2^s) exactly -- zero past m -- and the matrix form gives the literal form's words."""
    M, s, n, lin = 1 << w, w - beta * ell, 16, 5
    rng = np.random.default_rng(w * 1000 + beta * 10 + ell)
    edge = [0, M - 1, M - (1 << s >> 1), (M - (1 << s >> 1) - 1) % M, 1 << (w - 1), (1 << s >> 1)]
    for k, m in ((1, 5), (2, n), (1, 1)):
        s_in = [int(x) for x in rng.integers(0, 2, size=lin)]
        S = [[int(x) for x in rng.integers(0, 2, size=n)] for _ in range(k)]
        key = noise_free_key(rng, s_in, S, k, n, w, beta, ell)
        lwe = []
        for t in range(m):
            lwe += [edge[(t + i) % len(edge)] if (i + t) % 2 else rand_word(rng, w) for i in range(lin)] + [rand_word(rng, w)]
        out = model_pack_literal(lwe, key, lin, m, k, n, w, beta, ell)
        phase = out[k * n:]
        for q in range(k):
            phase = [(x - y) % M for x, y in zip(phase, negacyclic(out[q * n:(q + 1) * n], S[q], n))]
        want = [(lwe[t * (lin + 1) + lin] - sum(si * rounded(x, w, beta, ell) * (1 << s) for x, si in zip(lwe[t * (lin + 1):], s_in))) % M
                for t in range(m)] + [0] * (n - m)
        assert phase == want, (w, beta, ell, k, m)
        assert model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1) == out, (w, beta, ell, k, m)
        if w <= 64:
            assert model_pack_batch(lwe, key, lin, m, k, n, w, beta, ell, 1, dtype=np.uint32 if w == 32 else np.uint64) == out


def test_the_kernels_bit_fields_are_the_negated_digits():
    """native_pack_decompose_kernel restated: y = x + off with off = 2^(s-1) + sum_l (B/2) 2^(w - beta l) (gadget_offset of the host),
    and the stored word B/2 - ((y >> (w - beta l)) & (B - 1)) mod 2^w is -d_l(x) -- for every word width, s = 0 and s > 0, one digit
    as wide as the word, and the words that round across the top."""
    for w, beta, ell in [(32, 8, 4), (32, 5, 3), (32, 31, 1), (32, 32, 1), (64, 4, 6), (64, 32, 2), (64, 33, 1), (64, 1, 64), (128, 16, 8),
                         (128, 64, 2), (128, 128, 1), (128, 7, 5)]:
        M, s, B = 1 << w, w - beta * ell, 1 << beta
        off = ((1 << (s - 1) if s else 0) + sum((B // 2) << (w - beta * l) for l in range(1, ell + 1))) % M
        rng = np.random.default_rng(w + beta + ell)
        words = [0, 1, M - 1, M // 2, M // 2 - 1, (M - (1 << s >> 1)) % M, (M - (1 << s >> 1) - 1) % M] + [rand_word(rng, w) for _ in range(200)]
        for x in words:
            y = (x + off) % M
            got = [(B // 2 - ((y >> (w - beta * l)) & (B - 1))) % M for l in range(1, ell + 1)]
            assert got == [(-d) % M for d in digits(x, w, beta, ell)], (w, beta, ell, hex(x))


# -- the surface -----------------------------------------------------------------------------------------------------------------
def declarations(path):
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.findall(r"\b(cntt_[a-z0-9_]+)\s*\([^;{}]*\)\s*;", text)


def test_header_is_plain_c11_and_reached_through_cntt_ext_h():
    for path in (PACK, EXT):
        r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c", path],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    assert set(declarations(PACK)) == NEW and len(declarations(PACK)) == 2
    text = subprocess.run(["gcc", "-std=c11", "-E", "-P", "-x", "c", EXT], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", text))
    lines = open(EXT).read().splitlines()
    assert lines.index('#include "cntt_pack.h"') > lines.index('#include "cntt_keyswitch.h"')
    assert lines.index('#include "cntt_pack.h"') == max(i for i, ln in enumerate(lines) if ln.startswith("#include"))   # the last one
    for name in ("cntt.h", "cntt_gadget.h", "cntt_pbs.h", "cntt_keyswitch.h"):                                          # and only there
        assert not (NEW & set(re.findall(r"\b(cntt_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", name)).read()))), name
    assert sorted(declarations(EXT)) == ["cntt_native_external_product_batch", "cntt_native_max_terms"]


def test_library_exports_the_two_symbols():
    cntt.lib()
    so = os.path.join(ROOT, "concrete-ntt_amd", "libcntt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert NEW <= set(re.findall(r"\b(cntt_[a-z0-9_]+)\b", syms))


def test_pack_kernels_have_no_scratch_and_no_spills(tmp_path):
    """The gfx950 code object of the new unit: two kernels, each for u32 / u64 / 128-bit words, none with a private segment or a
    spilled register."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")):
        assert os.environ.get("CNTT_REQUIRE_CODE_OBJECTS") != "1", "ROCm LLVM tools not present"
        pytest.skip("ROCm LLVM tools not present on this machine")
    obj = os.path.join(ROOT, "concrete-ntt_amd", "csrc", "_obj", "native_pack.o")
    assert os.path.exists(obj), "objects not built in-tree (run __graft_entry__.build())"
    fat, co = str(tmp_path / "pack.fat"), str(tmp_path / "pack.co")
    subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + fat, "--output=" + co, "--unbundle"], check=True)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    seen = []
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)) + int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
        assert spills == 0 and scratch == 0, (name, spills, scratch)
        seen.append(name)
    assert len(seen) == 6, seen
    assert sum("native_pack_decompose_kernel" in s for s in seen) == 3 and sum("native_pack_body_kernel" in s for s in seen) == 3, seen


def chunk(plan, lin, levels):
    """C of the header, capped at Lin"""
    return min(max(1, min(plan.max_terms(), PACK_TERMS) // levels), lin)


@pytest.mark.parametrize("cls,wb", [(native32.Plan32, 4), (native64.Plan32, 8), (native128.Plan32, 16), (native64.Plan52, 8)])
def test_workspace_bytes_is_the_formula_of_the_header(cls, wb):
    def up(x):
        return (x + 255) // 256 * 256

    text = re.sub(r"\s+", " ", open(PACK).read())
    assert "cntt_native_pack_workspace_bytes = up(batch * C * levels * n * wb)" in text
    assert "C = max(1, min(cntt_native_max_terms(plan), CNTT_PACK_TERMS) / levels)" in text
    assert PACK_TERMS in (32, 64, 128)
    for n, lin, levels, batch in ((32, 0, 1, 1), (32, 1, 1, 1), (1024, 7, 3, 5), (256, 630, 4, 37), (2048, 2048, 2, 1000), (1024, 500, 65, 2),
                                  (65536, 40, 3, 2)):
        plan = cls.try_new(n)
        if plan is None:
            continue
        want = up(batch * chunk(plan, lin, levels) * levels * n * wb)
        assert plan.pack_workspace_bytes(lin, levels, batch) == want, (n, lin, levels, batch)
    assert cntt.lib().cntt_native_pack_workspace_bytes(None, 5, 2, 3) == 0


# -- CNTT_EINVAL: host buffers, refused before any device call ---------------------------------------------------------------------
N, K, B = 32, 1, 2
LIN, M_, LEVELS = 6, 5, 3


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def err():
    return cntt.lib().cntt_last_error().decode()


class Case:
    """Valid host arguments for native64 Plan32 at n = 32: 2 x 5 ciphertexts of dimension 6 into 2 GLWE ciphertexts with k = 1,
    levels = 3; the output filled with 7."""

    def __init__(self, cls=native64.Plan32):
        self.plan = cls.try_new(N)
        mult = 2 if self.plan.WORD == 16 else 1
        dt = self.plan.word_dtype
        self.lwe_in = np.arange(B * M_ * (LIN + 1) * mult, dtype=dt)
        self.out = np.full(B * (K + 1) * N * mult, 7, dtype=dt)
        self.keys = [np.zeros(LIN * LEVELS * (K + 1) * N, dtype=self.plan.res_dtype) for _ in range(self.plan.NPRIMES)]
        self.ws = np.zeros(self.plan.pack_workspace_bytes(LIN, LEVELS, B), dtype=np.uint8)

    def kp(self, null_plane=None):
        return (ctypes.c_void_p * self.plan.NPRIMES)(*[None if i == null_plane else k.ctypes.data for i, k in enumerate(self.keys)])

    def call(self, base_log=8, levels=LEVELS, out="own", lwe_in="own", keys="own", lin=LIN, m=M_, k=K, batch=B, ws=None, ws_bytes=None,
             plan="own"):
        out = self.out if isinstance(out, str) else out
        lwe_in = self.lwe_in if isinstance(lwe_in, str) else lwe_in
        keys = self.kp() if isinstance(keys, str) else keys
        return cntt.lib().cntt_native_pack_keyswitch_batch(self.plan._h if plan == "own" else plan, ptr(out), ptr(lwe_in), keys, lin, m, k,
                                                           base_log, levels, batch, ptr(ws),
                                                           (0 if ws is None else ws.nbytes) if ws_bytes is None else ws_bytes, 0, None)

    def untouched(self):
        return (self.out == 7).all()


@pytest.mark.parametrize("base_log,levels,word", [(0, 2, "base_log is 0"), (8, 0, "levels is 0"), (33, 2, "base_log * levels"),
                                                  (1, 65, "base_log * levels")])
def test_the_digit_cases_are_refused(base_log, levels, word):
    c = Case()
    assert c.call(base_log=base_log, levels=levels) == EINVAL and word in err()
    assert c.untouched()


def test_base_log_above_31_is_valid_here():
    """the digits of cntt_gadget.h, not the keyswitch's 32-bit ones: base_log = 32, levels = 2 passes the argument checks (what follows
    needs a device: any other status than CNTT_EINVAL)"""
    c = Case()
    keys = [np.zeros(LIN * 2 * (K + 1) * N, dtype=np.uint32) for _ in range(c.plan.NPRIMES)]
    assert c.call(base_log=32, levels=2, keys=(ctypes.c_void_p * c.plan.NPRIMES)(*[k.ctypes.data for k in keys])) != EINVAL


def test_levels_above_max_terms_is_refused():
    plan = native64.Plan32.try_new(32768)
    levels = plan.max_terms() + 1
    assert levels <= 64, "a size whose max_terms is below the 64 levels a 64-bit word allows"
    out = np.full(2 * 32768, 7, dtype=np.uint64)
    rc = cntt.lib().cntt_native_pack_keyswitch_batch(plan._h, ptr(out), ptr(np.zeros(4, dtype=np.uint64)), None, 1, 2, 1, 1, levels, 1, None, 0,
                                                     0, None)
    assert rc == EINVAL and "cntt_native_max_terms" in err() and "levels" in err()
    assert (out == 7).all()


def test_lwe_count_outside_1_to_n_is_refused():
    c = Case()
    assert c.call(m=0) == EINVAL and "lwe_count" in err()
    assert c.call(m=N + 1, lwe_in=np.zeros(B * (N + 1) * (LIN + 1), dtype=np.uint64)) == EINVAL and "lwe_count" in err()
    assert c.untouched()


def test_null_arguments_are_refused():
    c = Case()
    assert c.call(plan=None) == EINVAL and "plan" in err()
    assert c.call(out=None) == EINVAL and "glwe_out" in err()
    assert c.call(lwe_in=None) == EINVAL and "lwe_in" in err()
    assert c.call(keys=None) == EINVAL and "pksk_ntt" in err()
    assert c.call(keys=c.kp(null_plane=3)) == EINVAL and "key residue plane" in err() and "pksk_ntt[3]" in err()
    assert c.untouched()


def test_overlaps_are_refused():
    c = Case()
    big = np.full(4096, 7, dtype=np.uint64)
    out = big[:B * (K + 1) * N]
    ws = big.view(np.uint8)[16 * 8:16 * 8 + c.ws.nbytes]
    assert c.call(out=out, lwe_in=big[8:8 + c.lwe_in.size]) == EINVAL and "glwe_out overlaps lwe_in" in err()
    assert c.call(out=out, ws=ws) == EINVAL and "glwe_out overlaps workspace" in err()
    assert c.call(lwe_in=big[:c.lwe_in.size], ws=ws) == EINVAL and "lwe_in overlaps workspace" in err()
    assert (big == 7).all() and c.untouched()


def test_workspace_too_small_or_misaligned_is_refused():
    c = Case()
    assert c.call(ws=c.ws, ws_bytes=c.ws.nbytes - 1) == EINVAL and "workspace_bytes" in err()
    odd = np.zeros(c.ws.nbytes + 16, dtype=np.uint8)
    off = (4 - odd.ctypes.data) % 16                                                        # an address that is 4 mod 16
    assert c.call(ws=odd[off:off + c.ws.nbytes]) == EINVAL and "aligned" in err()
    assert c.untouched()


@pytest.mark.parametrize("cls", [native32.Plan32, native128.Plan32, native64.Plan52])
def test_the_other_kinds_refuse_the_same_way(cls):
    c = Case(cls)
    assert c.call(base_log=0) == EINVAL and "base_log is 0" in err()
    assert c.call(base_log=8 * c.plan.WORD, levels=2) == EINVAL and "base_log * levels" in err()
    assert c.call(m=N + 1) == EINVAL and "lwe_count" in err()
    assert c.call(ws=c.ws, ws_bytes=c.ws.nbytes - 1) == EINVAL and "workspace_bytes" in err()
    assert c.untouched()


def test_batch_zero_does_nothing():
    c = Case()
    assert cntt.lib().cntt_native_pack_keyswitch_batch(c.plan._h, None, None, None, LIN, M_, K, 8, 3, 0, None, 0, 0, None) == 0
    assert c.call(batch=0) == 0 and c.untouched()


def test_python_wrappers_panic_on_bad_shapes():
    c = Case()
    p = c.plan
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out[:-1], c.lwe_in, c.keys, LIN, M_, K, 8, LEVELS)                  # glwe_out too short
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN + 1, M_, K, 8, LEVELS)                   # not whole ciphertexts
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_ + 1, K, 8, LEVELS)                   # not whole groups of lwe_count
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, 0, K, 8, LEVELS)
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_, K + 1, 8, LEVELS)                   # out sized for k = 1
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, [k[:-N] for k in c.keys], LIN, M_, K, 8, LEVELS)     # a key polynomial missing
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_, K, 8, LEVELS + 1)                   # key sized for levels = 3
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys[:-1], LIN, M_, K, 8, LEVELS)
    with pytest.raises(cntt.Panic):
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_, K, 0, LEVELS)
    with pytest.raises(cntt.Panic):   # through the C checks
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_, K, 33, LEVELS)
    with pytest.raises(cntt.Panic):   # through the C checks: the workspace is too small
        p.pack_keyswitch_batch(c.out, c.lwe_in, c.keys, LIN, M_, K, 8, LEVELS, workspace=c.ws[:-256])
    with pytest.raises(cntt.Panic):
        p.pack_workspace_bytes(LIN, LEVELS, -1)
    with pytest.raises(cntt.Panic):
        p.pack_workspace_bytes(LIN, 0, 1)
    assert c.untouched()
