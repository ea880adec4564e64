"""prime32::Plan / prime64::Plan over the C ABI (shared implementation)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import Panic, buffer_info, check, lib
from ._pbs import PbsMixin


class PrimePlan(PbsMixin):
    """Negacyclic NTT plan for a prime modulus; mirrors concrete_ntt::prime{32,64}::Plan
    (src/prime64.rs:221-236, :701-1129 ; src/prime32.rs:601-616, :627-927).

    INPUT CONTRACT (include/cntt.h): every coefficient handed to fwd / inv / the pointwise calls is canonical, 0 <= x < modulus --
    what the reference's own tests feed and the only range on which its back ends agree with each other.  The
    kernels rely on it (the lazy classes skip the first stage's conditional subtraction); words >= modulus are NOT rejected and
    NOT reduced: the call completes and the affected outputs are unspecified residues (tests/test_gpu_parity.py pins exactly
    that: no fault, canonical inputs of the same batch unaffected).  `check_canonical(buf)` below validates a host array."""

    def check_canonical(self, buf):
        """Raise Panic if a host array holds a word >= modulus (the transforms do not check: see the class docstring)."""
        a = np.asarray(buf)
        if a.dtype.kind == "i":   # device tensors travel as int64 / int32: compare the words as the unsigned words they are
            a = a.view(np.dtype("u%d" % a.dtype.itemsize))
        if a.size and int(a.max()) >= self.modulus():
            raise Panic("coefficient %d >= modulus %d: outside the transforms' input contract" % (int(a.max()), self.modulus()))

    BITS = 64

    def __init__(self, handle, owned=True, parent=None):
        # a borrowed sub-plan (native ntt_i(), product plan_32()/plan_64()) keeps its parent alive: the C++ object
        # belongs to the parent and is freed with it
        self._h, self._owned, self._parent = handle, owned, parent
        self._p = "cntt_prime%d_" % self.BITS
        self._n = getattr(lib(), self._p + "ntt_size")(handle)

    # -- construction ------------------------------------------------------------------------
    @classmethod
    def try_new(cls, polynomial_size, modulus):
        """Plan::try_new -> plan or None; raises Panic where the reference panics (modulus <= 1)."""
        out = ctypes.c_void_p()
        rc = getattr(lib(), "cntt_prime%d_plan_new" % cls.BITS)(polynomial_size, modulus, ctypes.byref(out))
        if rc == _lib.NONE:
            return None
        check(rc)
        return cls(out.value)

    def clone(self):
        return type(self)(getattr(lib(), self._p + "plan_clone")(self._h))

    def __del__(self):
        try:
            if self._owned and self._h:
                getattr(lib(), self._p + "plan_free")(self._h)
        except Exception:
            pass

    def __repr__(self):  # Debug prints only ntt_size and modulus: src/prime64.rs:238-245
        return "Plan { ntt_size: %d, modulus: %d }" % (self.ntt_size(), self.modulus())

    # -- accessors ---------------------------------------------------------------------------
    def ntt_size(self):
        return self._n

    def modulus(self):
        return getattr(lib(), self._p + "modulus")(self._h)

    def info(self):
        out = _lib.PlanInfo()
        check(getattr(lib(), self._p + "plan_info")(self._h, ctypes.byref(out)))
        return out

    def table(self, which):
        out = np.zeros(self._n, dtype=self.dtype)
        rc = getattr(lib(), self._p + "plan_table")(self._h, which, out.ctypes.data, out.size)
        if rc == _lib.NONE:
            return None
        check(rc)
        return out

    @property
    def dtype(self):
        return np.uint64 if self.BITS == 64 else np.uint32

    def _arg(self, buf):
        ptr, count, esz, where, stream = buffer_info(buf)
        if esz != self.BITS // 8:
            raise TypeError("expected %d-byte elements" % (self.BITS // 8))
        return ptr, count, where, stream

    def _host(self, buf, what):
        """Argument of the reference's slice API: a host array (the C entry points take host pointers)."""
        ptr, count, where, _ = self._arg(buf)
        if where != _lib.MEM_HOST:
            raise TypeError("%s() takes host slices; use %s_batch() for device tensors" % (what, what))
        return ptr, count

    # -- the reference's slice API (host memory, one polynomial) -------------------------------
    def fwd(self, buf):
        ptr, count = self._host(buf, "fwd")
        check(getattr(lib(), self._p + "fwd")(self._h, ptr, count))

    def inv(self, buf):
        ptr, count = self._host(buf, "inv")
        check(getattr(lib(), self._p + "inv")(self._h, ptr, count))

    def mul_assign_normalize(self, lhs, rhs):
        lp, lc = self._host(lhs, "mul_assign_normalize")
        rp, rc_ = self._host(rhs, "mul_assign_normalize")
        check(getattr(lib(), self._p + "mul_assign_normalize")(self._h, lp, lc, rp, rc_))

    def normalize(self, values):
        vp, vc = self._host(values, "normalize")
        check(getattr(lib(), self._p + "normalize")(self._h, vp, vc))

    def mul_accumulate(self, acc, lhs, rhs):
        ap, ac = self._host(acc, "mul_accumulate")
        lp, lc = self._host(lhs, "mul_accumulate")
        rp, rc_ = self._host(rhs, "mul_accumulate")
        check(getattr(lib(), self._p + "mul_accumulate")(self._h, ap, ac, lp, lc, rp, rc_))

    # -- batched API: `batch` polynomials back to back, host arrays or device tensors ----------
    def _batch(self, buf):
        ptr, count, where, stream = self._arg(buf)
        if count % self._n:
            raise Panic("buffer length %d is not a multiple of ntt_size %d" % (count, self._n))
        return ptr, count // self._n, where, stream

    def fwd_batch(self, bufs):
        ptr, batch, where, stream = self._batch(bufs)
        check(getattr(lib(), self._p + "fwd_batch")(self._h, ptr, batch, where, stream))

    def inv_batch(self, bufs):
        ptr, batch, where, stream = self._batch(bufs)
        check(getattr(lib(), self._p + "inv_batch")(self._h, ptr, batch, where, stream))

    def mul_assign_normalize_batch(self, lhs, rhs):
        lp, batch, where, stream = self._batch(lhs)
        rp, rb, rwhere, _ = self._batch(rhs)
        if rb != batch or rwhere != where:
            raise Panic("lhs and rhs must have the same shape and live in the same memory")
        check(getattr(lib(), self._p + "mul_assign_normalize_batch")(self._h, lp, rp, batch, where, stream))

    def mul_ntt_batch(self, lhs, rhs_ntt):
        """Fused lhs <- inv(mul_assign_normalize(fwd(lhs), rhs_ntt)): same values as the three calls
        (src/prime64.rs:1254-1266), one pass over HBM for ntt_size <= 1024."""
        lp, batch, where, stream = self._batch(lhs)
        rp, rb, rwhere, _ = self._batch(rhs_ntt)
        if rb != batch or rwhere != where:
            raise Panic("lhs and rhs_ntt must have the same shape and live in the same memory")
        check(getattr(lib(), self._p + "mul_ntt_batch")(self._h, lp, rp, batch, where, stream))

    def external_product_batch(self, out, terms, key_ntt, nterms, nout, accumulate=False):
        """Fused mul_accumulate chain: out[b][o] (+)= inv(sum_j fwd(terms[b][j]) . key_ntt[j][o]) -- the values of
        fwd / mul_accumulate / inv (src/prime64.rs:794, :1085-1128, :872) called in sequence, in one pass over HBM."""
        op, ob, where, stream = self._batch(out)
        tp, tb, tw, _ = self._batch(terms)
        kp, kb, kw, _ = self._batch(key_ntt)
        if nout <= 0 or ob % nout or kb != nterms * nout or tb != (ob // nout) * nterms or tw != where or kw != where:
            raise Panic("out: batch*nout, terms: batch*nterms, key_ntt: nterms*nout polynomials in the same memory")
        check(getattr(lib(), self._p + "external_product_batch")(self._h, op, tp, kp, nterms, nout, ob // nout,
                                                                 1 if accumulate else 0, where, stream))

    def normalize_batch(self, values):
        vp, batch, where, stream = self._batch(values)
        check(getattr(lib(), self._p + "normalize_batch")(self._h, vp, batch, where, stream))

    def mul_accumulate_batch(self, acc, lhs, rhs):
        ap, batch, where, stream = self._batch(acc)
        lp, lb, lw, _ = self._batch(lhs)
        rp, rb, rw, _ = self._batch(rhs)
        if lb != batch or rb != batch or lw != where or rw != where:
            raise Panic("acc, lhs and rhs must have the same shape and live in the same memory")
        check(getattr(lib(), self._p + "mul_accumulate_batch")(self._h, ap, lp, rp, batch, where, stream))

    # -- programmable bootstrap mod p (include/cntt_prime_pbs.h): decomposition, modulus switch, blind rotation, extraction; the calls
    #    themselves: PbsMixin ------------------------------------------------------------------------------------------------------------
    _words = _arg

    def _fn(self, name):
        return getattr(lib(), self._p + name)

    def _bsk(self, bsk_ntt, where, lwe_dim, glwe_dim, levels):
        kp, kc, kw, _ = self._arg(bsk_ntt)
        if kw != where or kc != lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1) * self._n:
            raise Panic("bsk_ntt: lwe_dim*(glwe_dim+1)*levels*(glwe_dim+1) NTT-domain polynomials in the memory of the other buffers")
        return kp

    def blind_rotate_batch(self, acc, lut, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, workspace=None, lut_per_element=None):
        """acc[b] = X^rot_t[lwe_dim][b] * lut, then for i < lwe_dim: acc[b] += ExtProd(bsk_i, X^rot_t[i][b] acc[b] - acc[b]) mod p, in
        place: the words of gadget_decompose_batch(mode="cmux") + external_product_batch(accumulate=True) per iteration.  acc:
        batch*(glwe_dim+1) polynomials (written only); lut: glwe_dim+1 polynomials, or batch*(glwe_dim+1) (lut_per_element; None: told
        by the size); rot_t: (lwe_dim+1)*batch uint32 as lwe_modswitch_batch writes them; workspace: None (one allocation per call) or a
        buffer of pbs_workspace_bytes().  bsk_ntt: ONE buffer of lwe_dim*(glwe_dim+1)*levels*(glwe_dim+1) polynomials holding n^-1 *
        fwd(key) (fwd_batch, then normalize_batch)."""
        self._blind_rotate(acc, lut, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element)

    def bootstrap_batch(self, lwe_out, lwe_in, lut, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, workspace=None, lut_per_element=None):
        """lwe_modswitch_batch -> blind_rotate_batch -> sample_extract_batch(index=0) mod p in one call: lwe_in batch*(lwe_dim+1) words,
        lwe_out batch*(glwe_dim*n+1) words; rot_t and the accumulator live in the workspace (None: one allocation per call)."""
        self._bootstrap(lwe_out, lwe_in, lut, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element)

    # -- LWE keyswitch mod p, and keyswitch + bootstrap in one call (include/cntt_prime_keyswitch.h) -------------------------------------
    def ks_pbs_workspace_bytes(self, lwe_dim, glwe_dim, levels, batch):
        """Bytes of workspace keyswitch_bootstrap_batch needs: pbs_workspace_bytes() plus the batch*(lwe_dim+1) keyswitched words,
        rounded up to 256 bytes."""
        if min(lwe_dim, glwe_dim, levels, batch) < 0:
            raise Panic("lwe_dim, glwe_dim, levels and batch must not be negative")
        return self._fn("ks_pbs_workspace_bytes")(self._h, lwe_dim, glwe_dim, levels, batch)

    def _ksk(self, ksk, where, rows, lwe_dim_out, row_stride):
        """pointer of a keyswitch key of `rows` rows of row_stride words (None: packed), the last of which may end after its
        lwe_dim_out + 1 words; returns (pointer, row_stride)"""
        if row_stride is None:
            row_stride = lwe_dim_out + 1
        kp, kc, kw, _ = self._words(ksk)
        if row_stride < lwe_dim_out + 1:
            raise Panic("row_stride must be at least lwe_dim_out + 1 words")
        if kw != where or kc < (((rows - 1) * row_stride + lwe_dim_out + 1) if rows else 0):
            raise Panic("ksk: lwe_dim_in*levels rows of row_stride words in the memory of the other buffers")
        return kp, row_stride

    def keyswitch_batch(self, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, base_log, levels, row_stride=None):
        """lwe_out[b][c] = (lwe_in[b][lwe_dim_in] if c == lwe_dim_out) - sum_{i,l} digit_l(lwe_in[b][i]) * ksk[i*levels + l-1][c] mod p,
        the digits those of gadget_decompose_batch (balanced lift, top digit unmasked): lwe_in batch*(lwe_dim_in+1) words, lwe_out
        batch*(lwe_dim_out+1) words, ksk lwe_dim_in*levels rows of row_stride words (None: lwe_dim_out+1, packed), row (i, l) an LWE
        encryption under the output key of s_in[i] * 2^(W - base_log*l) mod p, body last; W = the bit length of p."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(lwe_out)
        if lwe_dim_in < 0 or lwe_dim_out < 0 or levels <= 0 or base_log <= 0 or ic % (lwe_dim_in + 1) or ow != where:
            raise Panic("lwe_in: batch*(lwe_dim_in+1) words; lwe_out in the same memory; base_log, levels >= 1")
        batch = ic // (lwe_dim_in + 1)
        if oc != batch * (lwe_dim_out + 1):
            raise Panic("lwe_out must hold batch*(lwe_dim_out+1) = %d words" % (batch * (lwe_dim_out + 1)))
        kp, row_stride = self._ksk(ksk, where, lwe_dim_in * levels, lwe_dim_out, row_stride)
        check(self._fn("keyswitch_batch")(self._h, op, ip, kp, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where, stream))

    def keyswitch_bootstrap_batch(self, lwe_out, lwe_in, ksk, ks_base_log, ks_levels, lut, bsk_ntt, lwe_dim, glwe_dim, base_log, levels,
                                  workspace=None, lut_per_element=None, row_stride=None):
        """keyswitch_batch from dimension glwe_dim*n to lwe_dim (digits ks_base_log, ks_levels) followed by bootstrap_batch, in one call
        and with the words of the two: lwe_in and lwe_out are both batch*(glwe_dim*n+1) words, so the call chains with itself.
        workspace: None (one allocation per call) or a buffer of ks_pbs_workspace_bytes()."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(lwe_out)
        big = glwe_dim * self._n if glwe_dim >= 0 else -1
        if lwe_dim < 0 or glwe_dim < 0 or min(levels, base_log, ks_levels, ks_base_log) <= 0 or ic % (big + 1) or ow != where or oc != ic:
            raise Panic("lwe_in and lwe_out: batch*(glwe_dim*n+1) words each in the same memory; base_log, levels >= 1")
        batch = ic // (big + 1)
        kp, row_stride = self._ksk(ksk, where, big * ks_levels, lwe_dim, row_stride)
        lp, per = self._lut(lut, lut_per_element, where, glwe_dim, batch)
        key = self._bsk(bsk_ntt, where, lwe_dim, glwe_dim, levels)
        wp, wb = self._workspace(workspace, where)
        check(self._fn("keyswitch_bootstrap_batch")(self._h, op, ip, kp, row_stride, ks_base_log, ks_levels, lp, per, key, lwe_dim, glwe_dim,
                                                    base_log, levels, batch, wp, wb, where, stream))

    # -- LWE-to-GLWE packing keyswitch through the NTT mod p (include/cntt_prime_pack.h) -------------------------------------------------
    def pack_workspace_bytes(self, lwe_dim_in, levels, batch):
        """Bytes of workspace pack_keyswitch_batch needs: the negated digit polynomials of one chunk of mask words, rounded up to 256
        bytes."""
        if min(lwe_dim_in, batch) < 0 or levels <= 0:
            raise Panic("lwe_dim_in and batch must not be negative, levels >= 1")
        return self._fn("pack_workspace_bytes")(self._h, lwe_dim_in, levels, batch)

    def pack_keyswitch_batch(self, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, workspace=None):
        """glwe_out[g][q] = (sum_t lwe_in[g][t][lwe_dim_in] X^t if q == glwe_dim) - sum_{i,l} D_{g,i,l} (*) K[i*levels + l-1][q] mod p,
        D_{g,i,l}[t] = digit_l(lwe_in[g][t][i]) for t < lwe_count, else 0, the digits those of gadget_decompose_batch: lwe_count LWE
        ciphertexts packed into one GLWE ciphertext whose coefficient t carries message t.  lwe_in: batch*lwe_count*(lwe_dim_in+1)
        words; glwe_out: batch*(glwe_dim+1) polynomials; pksk_ntt: ONE buffer of lwe_dim_in*levels*(glwe_dim+1) polynomials holding
        n^-1 * fwd(key) (fwd_batch, then normalize_batch), row (i, l) a GLWE encryption under the output key of the constant
        s_in[i] * 2^(W - base_log*l) mod p; workspace: None (one allocation per call) or a buffer of pack_workspace_bytes()."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if lwe_dim_in < 0 or glwe_dim < 0 or lwe_count <= 0 or levels <= 0 or base_log <= 0 or ic % (lwe_count * (lwe_dim_in + 1)) or ow != where:
            raise Panic("lwe_in: batch*lwe_count*(lwe_dim_in+1) words; glwe_out in the same memory; lwe_count, base_log, levels >= 1")
        batch = ic // (lwe_count * (lwe_dim_in + 1))
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        kp, kc, kw, _ = self._words(pksk_ntt)
        if kw != where or kc != lwe_dim_in * levels * (glwe_dim + 1) * n:
            raise Panic("pksk_ntt: lwe_dim_in*levels*(glwe_dim+1) NTT-domain polynomials in the memory of the other buffers")
        wp, wb = self._workspace(workspace, where)
        check(self._fn("pack_keyswitch_batch")(self._h, op, ip, kp, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, wp, wb, where,
                                               stream))

    # -- ring automorphism, Galois keyswitch and trace mod p (include/cntt_prime_automorphism.h) -------------------------------------------
    def _automorphism(self, name, out, inp, t):
        op, ob, where, stream = self._batch(out)
        ip, ib, iw, _ = self._batch(inp)
        if ob != ib or iw != where:
            raise Panic("out and in must hold the same number of polynomials in the same memory")
        check(self._fn(name)(self._h, op, ip, t, 1, ob, where, stream))

    def automorphism_batch(self, out, inp, t):
        """out = sigma_t(inp), f(X) -> f(X^t) in Z_p[X]/(X^n + 1), on every polynomial of inp; t odd, 1 <= t < 2n.  out is only written
        and may not overlap inp."""
        self._automorphism("automorphism_batch", out, inp, t)

    def automorphism_ntt_batch(self, out_ntt, in_ntt, t):
        """The same map on NTT-domain polynomials, a pure permutation: automorphism_ntt_batch(fwd f) = fwd(sigma_t f)."""
        self._automorphism("automorphism_ntt_batch", out_ntt, in_ntt, t)

    def glwe_automorphism_keyswitch_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_automorphism_keyswitch_batch needs: the negated digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return self._fn("glwe_automorphism_keyswitch_workspace_bytes")(self._h, glwe_dim, levels, batch)

    def glwe_trace_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_trace_batch needs: the digits of one step and the second ciphertext the steps alternate with."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return self._fn("glwe_trace_workspace_bytes")(self._h, glwe_dim, levels, batch)

    def _glwe_pair(self, glwe_out, glwe_in, ak_ntt, keys, glwe_dim, base_log, levels):
        op, oc, where, stream = self._words(glwe_out)
        ip, ic, iw, _ = self._words(glwe_in)
        per = (glwe_dim + 1) * self._n
        if glwe_dim < 0 or levels <= 0 or base_log <= 0 or keys < 0 or ic % per or oc != ic or iw != where:
            raise Panic("glwe_in and glwe_out: batch*(glwe_dim+1) polynomials each in the same memory; base_log, levels >= 1")
        kp = None
        if keys * glwe_dim:
            kp, kc, kw, _ = self._words(ak_ntt)
            if kw != where or kc != keys * glwe_dim * levels * per:
                raise Panic("ak_ntt: glwe_dim*levels*(glwe_dim+1) NTT-domain polynomials per key in the memory of the other buffers")
        return op, ip, kp, ic // per, where, stream

    def glwe_automorphism_keyswitch_batch(self, glwe_out, glwe_in, ak_ntt, t, glwe_dim, base_log, levels, add_input=False, workspace=None):
        """glwe_out[b] = AutoKS_t(glwe_in[b]) (+ glwe_in[b] with add_input): body sigma_t(body), minus the external product of the digits
        of the permuted mask polynomials with ak_ntt, whose row (r, l) is a GLWE encryption under S of sigma_t(S_r) * 2^(W - base_log*l),
        stored as n^-1 * fwd (fwd_batch, then normalize_batch).  The phase of the output is sigma_t of the phase of the input.
        workspace: None (one allocation per call) or a buffer of glwe_automorphism_keyswitch_workspace_bytes()."""
        op, ip, kp, batch, where, stream = self._glwe_pair(glwe_out, glwe_in, ak_ntt, 1, glwe_dim, base_log, levels)
        wp, wb = self._workspace(workspace, where)
        check(self._fn("glwe_automorphism_keyswitch_batch")(self._h, op, ip, kp, t, glwe_dim, base_log, levels, 1 if add_input else 0, batch,
                                                            wp, wb, where, stream))

    def glwe_trace_batch(self, glwe_out, glwe_in, ak_ntt, steps, glwe_dim, base_log, levels, workspace=None):
        """`steps` rounds of cur <- cur + AutoKS_(n/2^r + 1)(cur), r = 0 .. steps-1: coefficient i of the phase becomes 2^steps * phase[i]
        where 2^steps divides i and 0 elsewhere (scale by the inverse of 2^steps mod p afterwards).  ak_ntt: the `steps` keys back to
        back; workspace: None or a buffer of glwe_trace_workspace_bytes()."""
        if steps < 0:
            raise Panic("steps must not be negative")
        op, ip, kp, batch, where, stream = self._glwe_pair(glwe_out, glwe_in, ak_ntt, steps, glwe_dim, base_log, levels)
        wp, wb = self._workspace(workspace, where)
        check(self._fn("glwe_trace_batch")(self._h, op, ip, kp, steps, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- ring packing of LWE ciphertexts through automorphisms mod p (include/cntt_prime_ring_pack.h) -------------------------------------
    def glwe_merge_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_merge_batch needs: the negated digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return self._fn("glwe_merge_workspace_bytes")(self._h, glwe_dim, levels, batch)

    def ring_pack_workspace_bytes(self, lwe_count, glwe_dim, levels, batch):
        """Bytes of workspace ring_pack_batch needs: the digits of the widest stage (batch*max(lwe_count/2, 1) ciphertexts) and two
        ciphertext buffers of batch*max(lwe_count/2, 1) and batch*max(lwe_count/4, 1) ciphertexts, each rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0 or lwe_count <= 0:
            raise Panic("glwe_dim and batch must not be negative, lwe_count and levels >= 1")
        return self._fn("ring_pack_workspace_bytes")(self._h, lwe_count, glwe_dim, levels, batch)

    def glwe_embed_batch(self, glwe_out, lwe_in, glwe_dim):
        """The inverse of sample_extract_batch(index=0): glwe[q][0] = lwe[q*n], glwe[q][i] = -lwe[q*n + n - i] mod p, body
        (lwe[glwe_dim*n], 0, ..., 0).  lwe_in: batch*(glwe_dim*n + 1) words; glwe_out: batch*(glwe_dim + 1) polynomials, only written."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or ic % (glwe_dim * n + 1) or ow != where or oc != ic // (glwe_dim * n + 1) * (glwe_dim + 1) * n:
            raise Panic("lwe_in: batch*(glwe_dim*n+1) words; glwe_out: batch*(glwe_dim+1) polynomials in the same memory")
        check(self._fn("glwe_embed_batch")(self._h, op, ip, glwe_dim, ic // (glwe_dim * n + 1), where, stream))

    def glwe_merge_batch(self, glwe_out, glwe_even, glwe_odd, ak_ntt, shift, t, glwe_dim, base_log, levels, workspace=None):
        """One node of the packing tree: glwe_out[b] = a + AutoKS_t(d) with a = even[b] + X^shift odd[b], d = even[b] - X^shift odd[b];
        the words of the prefill (a, body plus sigma_t(d body)), the negated digits of sigma_t(d mask) and
        external_product_batch(accumulate=True) against the ONE key ak_ntt of glwe_automorphism_keyswitch_batch's layout.  0 <= shift <
        2n, t odd below 2n; workspace: None (one allocation per call) or a buffer of glwe_merge_workspace_bytes()."""
        op, ep, kp, batch, where, stream = self._glwe_pair(glwe_out, glwe_even, ak_ntt, 1, glwe_dim, base_log, levels)
        dp, dc, dw, _ = self._words(glwe_odd)
        if dw != where or dc != batch * (glwe_dim + 1) * self._n or shift < 0 or t < 0:
            raise Panic("glwe_odd: batch*(glwe_dim+1) polynomials in the memory of the other buffers; shift, t >= 0")
        wp, wb = self._workspace(workspace, where)
        check(self._fn("glwe_merge_batch")(self._h, op, ep, dp, kp, shift, t, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    def ring_pack_batch(self, glwe_out, lwe_in, ak_ntt, lwe_count, glwe_dim, base_log, levels, workspace=None):
        """Packs lwe_count (a power of two <= n) LWE ciphertexts of glwe_dim*n + 1 words, encrypted under the flattened GLWE key, into one
        GLWE ciphertext: glwe_embed_batch, log2(lwe_count) stages of glwe_merge_batch (shift n/2^s, t = 2^s + 1, key log2(n) - s) and
        glwe_trace_batch with log2(n) - log2(lwe_count) steps, word for word.  MESSAGE j SITS AT COEFFICIENT j*n/lwe_count (a strided
        layout) and carries the factor n: the phase there is n*phase(lwe_j) mod p and every other coefficient is 0 with noise-free keys;
        scale the INPUT words by n^-1 mod p to remove it.  lwe_in: batch*lwe_count*(glwe_dim*n + 1) words; glwe_out: batch*(glwe_dim+1)
        polynomials; ak_ntt: all log2(n) trace keys back to back (None when glwe_dim == 0); workspace: None or a buffer of
        ring_pack_workspace_bytes()."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or lwe_count <= 0 or levels <= 0 or base_log <= 0 or ic % (lwe_count * (glwe_dim * n + 1)) or ow != where:
            raise Panic("lwe_in: batch*lwe_count*(glwe_dim*n+1) words; glwe_out in the same memory; lwe_count, base_log, levels >= 1")
        batch = ic // (lwe_count * (glwe_dim * n + 1))
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        kp = None
        if glwe_dim:
            kp, kc, kw, _ = self._words(ak_ntt)
            if kw != where or kc != (n.bit_length() - 1) * glwe_dim * levels * (glwe_dim + 1) * n:
                raise Panic("ak_ntt: log2(n) keys of glwe_dim*levels*(glwe_dim+1) NTT-domain polynomials in the memory of the other buffers")
        wp, wb = self._workspace(workspace, where)
        check(self._fn("ring_pack_batch")(self._h, op, ip, kp, lwe_count, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- the CMux and the CMux tree against GGSW selectors mod p (include/cntt_prime_cmux.h) ------------------------------------------------
    def glwe_cmux_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_cmux_batch needs: the digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return self._fn("glwe_cmux_workspace_bytes")(self._h, glwe_dim, levels, batch)

    def cmux_tree_workspace_bytes(self, lut_count, glwe_dim, levels, batch):
        """Bytes of workspace cmux_tree_batch needs: the digits of the widest stage and two ciphertext buffers of batch*(lut_count/2) and
        batch*(lut_count/4) ciphertexts, each rounded up to 256 bytes (0 for lut_count == 1)."""
        if min(glwe_dim, batch) < 0 or levels <= 0 or lut_count <= 0:
            raise Panic("glwe_dim and batch must not be negative, lut_count and levels >= 1")
        return self._fn("cmux_tree_workspace_bytes")(self._h, lut_count, glwe_dim, levels, batch)

    def glwe_cmux_batch(self, glwe_out, glwe0, glwe1, ggsw_ntt, glwe_dim, base_log, levels, workspace=None):
        """glwe_out[b] = glwe0[b] + ExtProd(ggsw_ntt, glwe1[b] - glwe0[b]): glwe0[b] where the selector encrypts 0, glwe1[b] where it
        encrypts 1.  The words of the copy of glwe0, gadget_decompose_batch(mode="plain") of the difference (digits not negated) and
        external_product_batch(accumulate=True).  ggsw_ntt: ONE selector of (glwe_dim+1)*levels*(glwe_dim+1) NTT-domain polynomials in
        the layout of one iteration's slice of bsk_ntt, shared by the batch; workspace: None (one allocation per call) or a buffer of
        glwe_cmux_workspace_bytes()."""
        op, oc, where, stream = self._words(glwe_out)
        ap, ac, aw, _ = self._words(glwe0)
        bp, bc, bw, _ = self._words(glwe1)
        kp, kc, kw, _ = self._words(ggsw_ntt)
        per = (glwe_dim + 1) * self._n
        if glwe_dim < 0 or levels <= 0 or base_log <= 0 or ac % per or oc != ac or bc != ac or aw != where or bw != where:
            raise Panic("glwe0, glwe1 and glwe_out: batch*(glwe_dim+1) polynomials each in the same memory; base_log, levels >= 1")
        if kw != where or kc != (glwe_dim + 1) * levels * per:
            raise Panic("ggsw_ntt: (glwe_dim+1)*levels*(glwe_dim+1) NTT-domain polynomials in the memory of the other buffers")
        wp, wb = self._workspace(workspace, where)
        check(self._fn("glwe_cmux_batch")(self._h, op, ap, bp, kp, glwe_dim, base_log, levels, ac // per, wp, wb, where, stream))

    def cmux_tree_batch(self, glwe_out, lut_in, ggsw_ntt, lut_count, glwe_dim, base_log, levels, workspace=None):
        """Selects one of lut_count (a power of two) PLAIN table polynomials per batch element by log2(lut_count) GGSW selectors:
        glwe_out[b] = the trivial encryption of lut_in[b][a] plus noise, a = sum bit_i*2^i, selector i (address bit i, LSB first) at
        polynomial i*(glwe_dim+1)*levels*(glwe_dim+1) of ggsw_ntt.  Stage 1 takes the table entries as they are (zero masks are never
        decomposed), stages >= 2 are glwe_cmux_batch word for word; the top bit is consumed first.  lut_in: batch*lut_count
        polynomials; glwe_out: batch*(glwe_dim+1) polynomials; ggsw_ntt may be None when lut_count == 1; workspace: None or a buffer of
        cmux_tree_workspace_bytes()."""
        ip, ic, where, stream = self._words(lut_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or lut_count <= 0 or lut_count & (lut_count - 1) or levels <= 0 or base_log <= 0 or ic % (lut_count * n) or ow != where:
            raise Panic("lut_in: batch*lut_count polynomials; glwe_out in the same memory; lut_count a power of two; base_log, levels >= 1")
        batch = ic // (lut_count * n)
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        kp = None
        depth = lut_count.bit_length() - 1
        if depth:
            if ggsw_ntt is None:
                raise Panic("ggsw_ntt may be None only when lut_count == 1")
            kp, kc, kw, _ = self._words(ggsw_ntt)
            if kw != where or kc != depth * (glwe_dim + 1) * levels * (glwe_dim + 1) * n:
                raise Panic("ggsw_ntt: log2(lut_count) selectors of (glwe_dim+1)*levels*(glwe_dim+1) NTT-domain polynomials in the memory of "
                            "the other buffers")
        wp, wb = self._workspace(workspace, where)
        check(self._fn("cmux_tree_batch")(self._h, op, ip, kp, lut_count, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- the circuit bootstrap from LWE bits to GGSW selectors mod p (include/cntt_prime_cbs.h) --------------------------------------------
    def circuit_bootstrap_workspace_bytes(self, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch):
        """Bytes of workspace circuit_bootstrap_batch needs: rot_t, the tables, the digits of the rotation and the accumulators of the
        batch*cbs_levels bootstrap elements, their int32 keyswitch digits and the slab sums, each rounded up to 256 bytes."""
        return self._cbs_workspace_bytes("circuit_bootstrap_workspace_bytes", lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch)

    def _circuit_bootstrap(self, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels,
                           cbs_base_log, cbs_levels, workspace, log_lut_count=None):
        """circuit_bootstrap_batch, and with a log_lut_count circuit_bootstrap_manylut_batch."""
        one = () if log_lut_count is None else (log_lut_count,)
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(ggsw_ntt_out)
        n = self._n
        if min(lwe_dim, glwe_dim, *one) < 0 or min(pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels) <= 0 \
                or ic % (lwe_dim + 1) or ow != where:
            raise Panic("lwe_in: batch*(lwe_dim+1) words; ggsw_ntt_out in the same memory; every base_log and levels >= 1"
                        + ("; log_lut_count >= 0" if one else ""))
        batch = ic // (lwe_dim + 1)
        if oc != batch * (glwe_dim + 1) * cbs_levels * (glwe_dim + 1) * n:
            raise Panic("ggsw_ntt_out must hold batch*(glwe_dim+1)*cbs_levels*(glwe_dim+1) = %d polynomials"
                        % (batch * (glwe_dim + 1) * cbs_levels * (glwe_dim + 1)))
        if lwe_dim and bsk_ntt is None:
            raise Panic("bsk_ntt may be None only when lwe_dim == 0")
        kp = self._bsk(bsk_ntt, where, lwe_dim, glwe_dim, pbs_levels) if lwe_dim else None
        fp, fc, fw, _ = self._words(fpksk_ntt)
        if fw != where or fc != (glwe_dim + 1) * (glwe_dim * n + 1) * ks_levels * (glwe_dim + 1) * n:
            raise Panic("fpksk_ntt: (glwe_dim+1) keys of (glwe_dim*n+1)*ks_levels*(glwe_dim+1) NTT-domain polynomials in the memory of the "
                        "other buffers")
        wp, wb = self._workspace(workspace, where)
        call = self._fn("circuit_bootstrap_manylut_batch" if one else "circuit_bootstrap_batch")
        check(call(self._h, op, ip, kp, fp, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels, *one,
                   batch, wp, wb, where, stream))

    def circuit_bootstrap_batch(self, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                ks_levels, cbs_base_log, cbs_levels, workspace=None):
        """LWE encryptions of bits (phase bit*(p+1)/2 + e) -> GGSW selectors in the NTT domain, the ggsw_ntt argument of
        cmux_tree_batch: element b of lwe_in (batch*(lwe_dim+1) words) becomes selector b of ggsw_ntt_out
        (batch*(glwe_dim+1)*cbs_levels*(glwe_dim+1) polynomials).  One bootstrap per level against the constant table -H_l, then the
        functional keyswitch as a slot-wise digit x key sum against fpksk_ntt: glwe_dim+1 keys of
        (glwe_dim*n+1)*ks_levels*(glwe_dim+1) NTT-domain polynomials holding n^-1 * fwd(key).  bsk_ntt as in bootstrap_batch (None when
        lwe_dim == 0); workspace: None (one allocation per call) or a buffer of circuit_bootstrap_workspace_bytes()."""
        self._circuit_bootstrap(ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels,
                                cbs_base_log, cbs_levels, workspace)

    # -- the many-LUT bootstrap and the circuit bootstrap with one rotation per input bit mod p (include/cntt_prime_manylut.h) ------------
    #    lwe_modswitch_manylut_batch and sample_extract_many_batch are PbsMixin's
    def bootstrap_manylut_batch(self, lwe_out, lwe_in, lut, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count,
                                workspace=None, lut_per_element=None):
        """lwe_modswitch_manylut_batch -> blind_rotate_batch -> sample_extract_many_batch(count=lut_count) in one call: lut_count <=
        2^log_lut_count functions of every encrypted message for one rotation, function h at the coefficients m*2^log_lut_count + h of
        the table.  lwe_in: batch*(lwe_dim+1) words; lwe_out: batch*lut_count*(glwe_dim*n+1) words; workspace: None (one allocation per
        call) or a buffer of pbs_workspace_bytes()."""
        self._bootstrap_manylut(lwe_out, lwe_in, lut, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count, workspace,
                                lut_per_element)

    def circuit_bootstrap_manylut_workspace_bytes(self, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch):
        """Bytes of workspace circuit_bootstrap_manylut_batch needs: rot_t, the shared table, the digits of the rotation and the
        accumulators of the batch elements, the int32 keyswitch digits and the slab sums of the batch*cbs_levels selector rows, each
        rounded up to 256 bytes."""
        return self._cbs_workspace_bytes("circuit_bootstrap_manylut_workspace_bytes", lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels,
                                         batch)

    def circuit_bootstrap_manylut_batch(self, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels,
                                        ks_base_log, ks_levels, cbs_base_log, cbs_levels, log_lut_count, workspace=None):
        """circuit_bootstrap_batch with ONE blind rotation per input bit: the cbs_levels constants -H_l are interleaved in one shared
        table, the modulus switch clears the low log_lut_count bits, and level l is extracted at the index l - 1.  cbs_levels <=
        2^log_lut_count <= n/2.  The buffers are those of circuit_bootstrap_batch; workspace: None (one allocation per call) or a buffer
        of circuit_bootstrap_manylut_workspace_bytes()."""
        self._circuit_bootstrap(ggsw_ntt_out, lwe_in, bsk_ntt, fpksk_ntt, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels,
                                cbs_base_log, cbs_levels, workspace, log_lut_count)

    # -- multi-bit blind rotation and bootstrap mod p (include/cntt_prime_multibit.h) ------------------------------------------------------
    #    multibit_pbs_workspace_bytes is PbsMixin's: no scratch here, so it equals pbs_workspace_bytes
    def multibit_accumulate_batch(self, out_ntt, terms_ntt, rot_rows, key_group, nterms, nout, grouping):
        """out_ntt[b][o][c] = sum_{t < 2^grouping} fwd(X^e_t(b))[c] * sum_j terms_ntt[b][j][c] * key_group[t][j][o][c] mod p, exact for
        every prime; e_t(b) = the sum of rot_rows[i*batch + b] over the set bits i of t, mod 2n.  out_ntt: batch*nout polynomials
        (written only); terms_ntt: batch*nterms; key_group: 2^grouping*nterms*nout; rot_rows: grouping*batch uint32."""
        op, ob, where, stream = self._batch(out_ntt)
        tp, tb, tw, _ = self._batch(terms_ntt)
        kp, kb, kw, _ = self._batch(key_group)
        if nout <= 0 or nterms < 0 or grouping < 0 or ob % nout or tb != (ob // nout) * nterms or tw != where or kw != where:
            raise Panic("out_ntt: batch*nout, terms_ntt: batch*nterms polynomials in the same memory")
        batch = ob // nout
        rp, rc_ = self._rot(rot_rows, where, "rot_rows")
        if 1 <= grouping <= 4 and (kb != (nterms * nout) << grouping or rc_ != grouping * batch):
            raise Panic("key_group: 2^grouping*nterms*nout polynomials; rot_rows: grouping*batch uint32")
        check(self._fn("multibit_accumulate_batch")(self._h, op, tp, rp, kp, nterms, nout, grouping, batch, where, stream))

    def _bsk_mb(self, bsk_mb, where, lwe_dim, glwe_dim, levels, grouping):
        kp, kc, kw, _ = self._arg(bsk_mb)
        if kw != where:
            raise Panic("bsk_mb must live in the memory of the other buffers")
        # (a grouping the C call refuses is left to it: it names the argument)
        if 1 <= grouping <= 4 and lwe_dim % grouping == 0:
            if kc != ((lwe_dim // grouping) * (glwe_dim + 1) * levels * (glwe_dim + 1) << grouping) * self._n:
                raise Panic("bsk_mb: (lwe_dim/grouping)*2^grouping*(glwe_dim+1)*levels*(glwe_dim+1) NTT-domain polynomials")
        return kp

    def multibit_blind_rotate_batch(self, acc, lut, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, workspace=None,
                                    lut_per_element=None):
        """acc[b] = X^rot_t[lwe_dim][b] * lut, then for each group r of `grouping` mask words: acc[b] = sum_t X^e_t ExtProd(bsk_mb[r][t],
        acc[b]) mod p -- the words of gadget_decompose_batch(mode="plain"), fwd_batch, multibit_accumulate_batch and inv_batch per group.
        bsk_mb: ONE buffer of (lwe_dim/grouping)*2^grouping*(glwe_dim+1)*levels*(glwe_dim+1) polynomials holding n^-1 * fwd(key), key
        (r, t) the GGSW of prod_{i in t} s_{r*grouping+i} * prod_{i not in t} (1 - s_{r*grouping+i}).  The rest as blind_rotate_batch;
        workspace: None or a buffer of multibit_pbs_workspace_bytes()."""
        self._blind_rotate(acc, lut, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping)

    def multibit_bootstrap_batch(self, lwe_out, lwe_in, lut, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, workspace=None,
                                 lut_per_element=None):
        """lwe_modswitch_batch -> multibit_blind_rotate_batch -> sample_extract_batch(index=0) mod p in one call: lwe_in batch*(lwe_dim+1)
        words, lwe_out batch*(glwe_dim*n+1) words; rot_t and the accumulator live in the workspace (None: one allocation per call)."""
        self._bootstrap(lwe_out, lwe_in, lut, bsk_mb, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping)
