"""native32/64/128 and native_binary32/64/128 plans over the C ABI (shared implementation)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import Panic, buffer_info, check, lib
from ._pbs import PbsMixin
from .prime32 import Plan as _Plan32
from .prime64 import Plan as _Plan64


class NativePlan(PbsMixin):
    """Mirrors the reference's PlanNN types: try_new(n), ntt_size(), ntt_i(), fwd, fwd_binary, inv,
    negacyclic_polymul (e.g. src/native64.rs:930-1070).  Coefficients: numpy uint32 / uint64 arrays;
    u128 words are (lo, hi) uint64 pairs, i.e. arrays of 2n uint64 (16-byte little-endian)."""

    KIND = 1
    NPRIMES, WORD, RES = 5, 8, 4
    BINARY = False

    def __init__(self, handle):
        self._h = handle
        self._n = lib().cntt_native_ntt_size(handle)

    @classmethod
    def try_new(cls, n):
        out = ctypes.c_void_p()
        rc = lib().cntt_native_plan_new(cls.KIND, n, ctypes.byref(out))
        if rc == _lib.NONE:
            return None
        check(rc)
        return cls(out.value)

    def clone(self):
        return type(self)(lib().cntt_native_plan_clone(self._h))

    def __del__(self):
        try:
            if self._h:
                lib().cntt_native_plan_free(self._h)
        except Exception:
            pass

    def ntt_size(self):
        return self._n

    def ntt(self, i):
        """ntt_0() .. ntt_k(): borrowed prime sub-plan (src/native64.rs:950-969)."""
        if self.RES == 8:
            h = lib().cntt_native_ntt64(self._h, i)
            return _Plan64(h, owned=False, parent=self) if h else None
        h = lib().cntt_native_ntt32(self._h, i)
        return _Plan32(h, owned=False, parent=self) if h else None

    # -- helpers -----------------------------------------------------------------------------
    @property
    def word_dtype(self):
        return np.uint32 if self.WORD == 4 else np.uint64

    @property
    def res_dtype(self):
        return np.uint64 if self.RES == 8 else np.uint32

    def _words(self, buf):
        ptr, count, esz, where, stream = buffer_info(buf)
        if esz != min(self.WORD, 8):
            raise TypeError("expected %d-byte words" % self.WORD)
        return ptr, count // (2 if self.WORD == 16 else 1), where, stream

    def _res(self, residues, where, count):
        if len(residues) != self.NPRIMES:
            raise Panic("expected %d residue buffers" % self.NPRIMES)
        ptrs = []
        for r in residues:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or c != count:
                raise Panic("residue buffers must match the value buffer (size, memory)")
            ptrs.append(ptr)
        return (ctypes.c_void_p * self.NPRIMES)(*ptrs)

    # -- the reference's slice API (host memory: the C entry points take host pointers) -------------
    def _host_words(self, buf, what):
        ptr, count, where, _ = self._words(buf)
        if where != _lib.MEM_HOST:
            raise TypeError("%s() takes host slices; use %s_batch() for device tensors" % (what, what))
        return ptr, count, where

    def fwd(self, value, *residues):
        ptr, count, where = self._host_words(value, "fwd")
        check(lib().cntt_native_fwd(self._h, ptr, count, self._res(residues, where, count)))

    def fwd_binary(self, value, *residues):
        if not self.BINARY:
            raise AttributeError("fwd_binary exists only on native_binary* plans")
        ptr, count, where = self._host_words(value, "fwd")
        check(lib().cntt_native_fwd_binary(self._h, ptr, count, self._res(residues, where, count)))

    def inv(self, value, *residues):
        ptr, count, where = self._host_words(value, "inv")
        check(lib().cntt_native_inv(self._h, ptr, count, self._res(residues, where, count)))

    def negacyclic_polymul(self, prod, lhs, rhs):
        pp, pc, _ = self._host_words(prod, "negacyclic_polymul")
        lp, lc, _ = self._host_words(lhs, "negacyclic_polymul")
        rp, rc_, _ = self._host_words(rhs, "negacyclic_polymul")
        check(lib().cntt_native_negacyclic_polymul(self._h, pp, pc, lp, lc, rp, rc_))

    # -- batched --------------------------------------------------------------------------------
    def _batchn(self, buf):
        ptr, count, where, stream = self._words(buf)
        if count % self._n:
            raise Panic("buffer length is not a multiple of ntt_size")
        return ptr, count, count // self._n, where, stream

    def fwd_batch(self, value, residues, binary=False):
        ptr, count, batch, where, stream = self._batchn(value)
        fn = lib().cntt_native_fwd_binary_batch if binary else lib().cntt_native_fwd_batch
        check(fn(self._h, ptr, self._res(residues, where, count), batch, where, stream))

    def inv_batch(self, value, residues):
        ptr, count, batch, where, stream = self._batchn(value)
        check(lib().cntt_native_inv_batch(self._h, ptr, self._res(residues, where, count), batch, where, stream))

    def negacyclic_polymul_batch(self, prod, lhs, rhs):
        pp, pc, batch, where, stream = self._batchn(prod)
        lp, lc, _, lw, _ = self._batchn(lhs)
        rp, rc_, _, rw, _ = self._batchn(rhs)
        if lc != pc or rc_ != pc or lw != where or rw != where:
            raise Panic("prod, lhs and rhs must have the same shape and live in the same memory")
        check(lib().cntt_native_negacyclic_polymul_batch(self._h, pp, lp, rp, batch, where, stream))

    def reserve(self, batch):
        check(lib().cntt_native_reserve(self._h, batch))

    # -- external product (include/cntt_ext.h: a device extension, no counterpart in the reference) ------------------------------
    def max_terms(self):
        """Largest nterms for which external_product_batch stays inside the kind's exact CRT range (>= 1)."""
        return lib().cntt_native_max_terms(self._h)

    def external_product_batch(self, out, terms, key_residues, nterms, nout, accumulate=False):
        """out[b][o] (+)= sum_j terms[b][j] (*) key[j][o] in Z/2^w[X]/(X^n+1): the words of nterms*nout negacyclic_polymul calls
        summed mod 2^w.  out: batch*nout polynomials, terms: batch*nterms, key_residues: NPRIMES buffers of nterms*nout residue
        polynomials as fwd_batch (fwd_binary for the binary kinds) writes them for the nterms*nout key polynomials."""
        op, oc, where, stream = self._words(out)
        tp, tc, tw, _ = self._words(terms)
        n = self._n
        if nout <= 0 or nterms < 0 or oc % (n * nout) or tw != where:
            raise Panic("out: batch*nout polynomials; terms: batch*nterms polynomials in the same memory")
        batch = oc // (n * nout)
        if tc != batch * nterms * n:
            raise Panic("terms must hold batch*nterms = %d polynomials" % (batch * nterms))
        if len(key_residues) != self.NPRIMES:
            raise Panic("expected %d key residue buffers" % self.NPRIMES)
        kptrs = []
        for r in key_residues:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or c != nterms * nout * n:
                raise Panic("key residue buffers: nterms*nout residue polynomials in the memory of out")
            kptrs.append(ptr)
        keys = (ctypes.c_void_p * self.NPRIMES)(*kptrs)
        check(lib().cntt_native_external_product_batch(self._h, op, tp, keys, nterms, nout, batch, 1 if accumulate else 0, where,
                                                       stream))

    # -- rotation / CMux difference / signed gadget decomposition (include/cntt_gadget.h): gadget_decompose_batch is PbsMixin's -----------
    def external_product_decomposed_batch(self, out, polys, key_residues, base_log, levels, nout, rot=None, mode="plain",
                                          addend=None):
        """out[b][o] = (addend[b][o] if addend is given) + sum_{p,l} digit_l(source(polys[b][p])) (*) key[p*levels + l-1][o] mod 2^w:
        gadget_decompose_batch followed by external_product_batch, without the digits ever being stored.  out: batch*nout
        polynomials; polys: batch*npolys; key_residues: NPRIMES buffers of npolys*levels*nout residue polynomials; addend: None, out
        itself, polys (nout == npolys) or another buffer of out's shape.  out must not overlap polys."""
        pp, pc, where, stream, rp, m = self._src(polys, rot, mode)
        op, oc, ow, _ = self._words(out)
        n = self._n
        if nout <= 0 or levels <= 0 or base_log <= 0 or oc % (n * nout) or ow != where:
            raise Panic("out: batch*nout polynomials in the memory of polys; base_log, levels, nout >= 1")
        batch = oc // (n * nout)
        if (batch == 0 and pc) or (batch and pc % (batch * n)) or (rp and rp[1] != batch):
            raise Panic("polys must hold batch*npolys polynomials and rot one exponent per batch element")
        npolys = pc // (batch * n) if batch else 0
        ap = None
        if addend is not None:
            ap, ac, aw, _ = self._words(addend)
            if ac != oc or aw != where:
                raise Panic("addend must have the shape and the memory of out")
        if len(key_residues) != self.NPRIMES:
            raise Panic("expected %d key residue buffers" % self.NPRIMES)
        kptrs = []
        for r in key_residues:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or c != npolys * levels * nout * n:
                raise Panic("key residue buffers: npolys*levels*nout residue polynomials in the memory of out")
            kptrs.append(ptr)
        keys = (ctypes.c_void_p * self.NPRIMES)(*kptrs)
        check(lib().cntt_native_external_product_decomposed_batch(self._h, op, pp, rp[0] if rp else None, ap, keys, npolys, base_log,
                                                                  levels, m, nout, batch, where, stream))

    # -- programmable bootstrap (include/cntt_pbs.h): modulus switch, blind rotation in place, sample extraction; the calls themselves:
    #    PbsMixin ------------------------------------------------------------------------------------------------------------------------
    def _fn(self, name):
        return getattr(lib(), "cntt_native_" + name)

    def _bsk(self, bsk_residues, where, lwe_dim, glwe_dim, levels):
        if len(bsk_residues) != self.NPRIMES:
            raise Panic("expected %d key residue buffers" % self.NPRIMES)
        want = lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1) * self._n
        ptrs = []
        for r in bsk_residues:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or c != want:
                raise Panic("key residue buffers: lwe_dim*(glwe_dim+1)*levels*(glwe_dim+1) residue polynomials in the memory of the "
                            "other buffers")
            ptrs.append(ptr)
        return (ctypes.c_void_p * self.NPRIMES)(*ptrs)

    def blind_rotate_batch(self, acc, lut, rot_t, bsk_residues, lwe_dim, glwe_dim, base_log, levels, workspace=None,
                           lut_per_element=None):
        """acc[b] = X^rot_t[lwe_dim][b] * lut, then for i < lwe_dim: acc[b] += ExtProd(bsk_i, X^rot_t[i][b] acc[b] - acc[b]) mod 2^w, in
        place: the words of gadget_decompose_batch(mode="cmux") + external_product_batch(accumulate=True) per iteration.  acc:
        batch*(glwe_dim+1) polynomials (written only); lut: glwe_dim+1 polynomials, or batch*(glwe_dim+1) (lut_per_element; None: told
        by the size); rot_t: (lwe_dim+1)*batch uint32 as lwe_modswitch_batch writes them; workspace: None (one allocation per call) or a
        buffer of pbs_workspace_bytes().  bsk_residues: NPRIMES buffers of lwe_dim*(glwe_dim+1)*levels*(glwe_dim+1) residue polynomials
        as fwd_batch writes them for the key polynomials."""
        self._blind_rotate(acc, lut, rot_t, bsk_residues, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element)

    def bootstrap_batch(self, lwe_out, lwe_in, lut, bsk_residues, lwe_dim, glwe_dim, base_log, levels, workspace=None,
                        lut_per_element=None):
        """lwe_modswitch_batch -> blind_rotate_batch -> sample_extract_batch(index=0) mod 2^w in one call: lwe_in batch*(lwe_dim+1)
        words, lwe_out batch*(glwe_dim*n+1) words; rot_t and the accumulator live in the workspace (None: one allocation per call)."""
        self._bootstrap(lwe_out, lwe_in, lut, bsk_residues, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element)

    # -- LWE keyswitch, and keyswitch + bootstrap in one call (include/cntt_keyswitch.h) ------------------------------------------------
    def ks_pbs_workspace_bytes(self, lwe_dim, glwe_dim, levels, batch):
        """Bytes of workspace keyswitch_bootstrap_batch needs: pbs_workspace_bytes() plus the batch*(lwe_dim+1) keyswitched words,
        rounded up to 256 bytes."""
        if min(lwe_dim, glwe_dim, levels, batch) < 0:
            raise Panic("lwe_dim, glwe_dim, levels and batch must not be negative")
        return lib().cntt_native_ks_pbs_workspace_bytes(self._h, lwe_dim, glwe_dim, levels, batch)

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
        """lwe_out[b][c] = (lwe_in[b][lwe_dim_in] if c == lwe_dim_out) - sum_{i,l} digit_l(lwe_in[b][i]) * ksk[i*levels + l-1][c] mod 2^w:
        lwe_in batch*(lwe_dim_in+1) words, lwe_out batch*(lwe_dim_out+1) words, ksk lwe_dim_in*levels rows of row_stride words (None:
        lwe_dim_out+1, packed), row (i, l) an LWE encryption under the output key of s_in[i] * 2^(w - base_log*l), body last."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(lwe_out)
        if lwe_dim_in < 0 or lwe_dim_out < 0 or levels <= 0 or base_log <= 0 or ic % (lwe_dim_in + 1) or ow != where:
            raise Panic("lwe_in: batch*(lwe_dim_in+1) words; lwe_out in the same memory; base_log, levels >= 1")
        batch = ic // (lwe_dim_in + 1)
        if oc != batch * (lwe_dim_out + 1):
            raise Panic("lwe_out must hold batch*(lwe_dim_out+1) = %d words" % (batch * (lwe_dim_out + 1)))
        kp, row_stride = self._ksk(ksk, where, lwe_dim_in * levels, lwe_dim_out, row_stride)
        check(lib().cntt_native_keyswitch_batch(self._h, op, ip, kp, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where,
                                                stream))

    def keyswitch_bootstrap_batch(self, lwe_out, lwe_in, ksk, ks_base_log, ks_levels, lut, bsk_residues, lwe_dim, glwe_dim, base_log,
                                  levels, workspace=None, lut_per_element=None, row_stride=None):
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
        keys = self._bsk(bsk_residues, where, lwe_dim, glwe_dim, levels)
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_keyswitch_bootstrap_batch(self._h, op, ip, kp, row_stride, ks_base_log, ks_levels, lp, per, keys, lwe_dim,
                                                          glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- LWE-to-GLWE packing keyswitch through the NTT (include/cntt_pack.h) --------------------------------------------------------------
    def pack_workspace_bytes(self, lwe_dim_in, levels, batch):
        """Bytes of workspace pack_keyswitch_batch needs: the negated digit polynomials of one chunk of mask words, rounded up to 256
        bytes."""
        if min(lwe_dim_in, batch) < 0 or levels <= 0:
            raise Panic("lwe_dim_in and batch must not be negative, levels >= 1")
        return lib().cntt_native_pack_workspace_bytes(self._h, lwe_dim_in, levels, batch)

    def pack_keyswitch_batch(self, glwe_out, lwe_in, pksk_residues, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, workspace=None):
        """glwe_out[g][p] = (sum_t lwe_in[g][t][lwe_dim_in] X^t if p == glwe_dim) - sum_{i,l} D_{g,i,l} (*) K[i*levels + l-1][p] mod 2^w,
        D_{g,i,l}[t] = digit_l(lwe_in[g][t][i]) for t < lwe_count, else 0: lwe_count LWE ciphertexts packed into one GLWE ciphertext
        whose coefficient t carries message t.  lwe_in: batch*lwe_count*(lwe_dim_in+1) words; glwe_out: batch*(glwe_dim+1)
        polynomials; pksk_residues: NPRIMES buffers of lwe_dim_in*levels*(glwe_dim+1) residue polynomials as fwd_batch writes them for
        the key polynomials, row (i, l) a GLWE encryption under the output key of the constant s_in[i] * 2^(w - base_log*l);
        workspace: None (one allocation per call) or a buffer of pack_workspace_bytes()."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if lwe_dim_in < 0 or glwe_dim < 0 or lwe_count <= 0 or levels <= 0 or base_log <= 0 or ic % (lwe_count * (lwe_dim_in + 1)) or ow != where:
            raise Panic("lwe_in: batch*lwe_count*(lwe_dim_in+1) words; glwe_out in the same memory; lwe_count, base_log, levels >= 1")
        batch = ic // (lwe_count * (lwe_dim_in + 1))
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        if len(pksk_residues) != self.NPRIMES:
            raise Panic("expected %d key residue buffers" % self.NPRIMES)
        ptrs = []
        for r in pksk_residues:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or c != lwe_dim_in * levels * (glwe_dim + 1) * n:
                raise Panic("key residue buffers: lwe_dim_in*levels*(glwe_dim+1) residue polynomials in the memory of the other buffers")
            ptrs.append(ptr)
        keys = (ctypes.c_void_p * self.NPRIMES)(*ptrs)
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_pack_keyswitch_batch(self._h, op, ip, keys, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, wp, wb,
                                                     where, stream))

    # -- multi-bit blind rotation and bootstrap (include/cntt_multibit.h): Plan32 kinds --------------------------------------------------
    #    multibit_pbs_workspace_bytes is PbsMixin's: its scratch is the term planes and the output planes; 0 for a Plan52 kind
    def _planes(self, planes, where, count, what):
        """NPRIMES buffers of `count` residues each (count None: not checked) -> the pointer array of the C call"""
        if len(planes) != self.NPRIMES:
            raise Panic("expected %d %s residue buffers" % (self.NPRIMES, what))
        ptrs = []
        for r in planes:
            ptr, c, esz, w, _ = buffer_info(r)
            if esz != self.RES or w != where or (count is not None and c != count):
                raise Panic("%s residue buffers: %s residues each in the memory of the other buffers" % (what, count))
            ptrs.append(ptr)
        return (ctypes.c_void_p * self.NPRIMES)(*ptrs)

    def multibit_accumulate_batch(self, out_residues, terms_residues, rot_rows, key_residues, nterms, nout, grouping):
        """Per residue prime i: out[i][b][o][c] = n^-1 sum_{t < 2^grouping} fwd_i(X^e_t(b))[c] * sum_j terms[i][b][j][c] * key[i][t][j][o][c]
        mod P_i; e_t(b) = the sum of rot_rows[q*batch + b] over the set bits q of t, mod 2n.  inv_batch on out_residues then gives the
        coefficient-domain words.  out_residues: NPRIMES buffers of batch*nout residue polynomials (written only); terms_residues:
        batch*nterms each; key_residues: 2^grouping*nterms*nout each; rot_rows: grouping*batch uint32."""
        n = self._n
        if nout == 0:   # the header: nout == 0 does nothing
            return
        _, oc, _, where, stream = buffer_info(out_residues[0]) if len(out_residues) else (None, 0, 0, _lib.MEM_HOST, None)
        if nout < 0 or nterms < 0 or grouping < 0 or oc % (nout * n):
            raise Panic("out_residues: batch*nout residue polynomials per prime")
        batch = oc // (nout * n)
        outs = self._planes(out_residues, where, oc, "out")
        terms = self._planes(terms_residues, where, batch * nterms * n, "terms")
        keys = self._planes(key_residues, where, ((nterms * nout) << grouping) * n if 1 <= grouping <= 4 else None, "key")
        rp, rc_ = self._rot(rot_rows, where, "rot_rows")
        if 1 <= grouping <= 4 and rc_ != grouping * batch:
            raise Panic("rot_rows: grouping*batch uint32")
        check(lib().cntt_native_multibit_accumulate_batch(self._h, outs, terms, rp, keys, nterms, nout, grouping, batch, where, stream))

    def _bsk_mb(self, bsk_mb, where, lwe_dim, glwe_dim, levels, grouping):
        # (a grouping the C call refuses is left to it: it names the argument)
        want = None
        if 1 <= grouping <= 4 and lwe_dim % grouping == 0:
            want = ((lwe_dim // grouping) * (glwe_dim + 1) * levels * (glwe_dim + 1) << grouping) * self._n
        return self._planes(bsk_mb, where, want, "bsk_mb")

    def multibit_blind_rotate_batch(self, acc, lut, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, workspace=None,
                                    lut_per_element=None):
        """acc[b] = X^rot_t[lwe_dim][b] * lut, then for each group r of `grouping` mask words: acc[b] = sum_t X^e_t ExtProd(bsk_mb[r][t],
        acc[b]) mod 2^w -- the words of gadget_decompose_batch(mode="plain"), fwd_batch, multibit_accumulate_batch and inv_batch per
        group.  bsk_mb: NPRIMES buffers of (lwe_dim/grouping)*2^grouping*(glwe_dim+1)*levels*(glwe_dim+1) residue polynomials as
        fwd_batch writes them, key (r, t) the GGSW of prod_{i in t} s_{r*grouping+i} * prod_{i not in t} (1 - s_{r*grouping+i}).  The
        rest as blind_rotate_batch; workspace: None or a buffer of multibit_pbs_workspace_bytes()."""
        self._blind_rotate(acc, lut, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping)

    def multibit_bootstrap_batch(self, lwe_out, lwe_in, lut, bsk_mb, lwe_dim, glwe_dim, base_log, levels, grouping, workspace=None,
                                 lut_per_element=None):
        """lwe_modswitch_batch -> multibit_blind_rotate_batch -> sample_extract_batch(index=0) mod 2^w in one call: lwe_in
        batch*(lwe_dim+1) words, lwe_out batch*(glwe_dim*n+1) words; rot_t and the accumulator live in the workspace (None: one
        allocation per call)."""
        self._bootstrap(lwe_out, lwe_in, lut, bsk_mb, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping)

    # -- the CMux and the CMux tree against GGSW selectors (include/cntt_cmux.h) ---------------------------------------------------------
    def glwe_cmux_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_cmux_batch needs: the digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return lib().cntt_native_glwe_cmux_workspace_bytes(self._h, glwe_dim, levels, batch)

    def cmux_tree_workspace_bytes(self, lut_count, glwe_dim, levels, batch):
        """Bytes of workspace cmux_tree_batch needs: the digits of the widest stage and two ciphertext buffers of batch*(lut_count/2) and
        batch*(lut_count/4) ciphertexts, each rounded up to 256 bytes (0 for lut_count == 1)."""
        if min(glwe_dim, batch) < 0 or levels <= 0 or lut_count <= 0:
            raise Panic("glwe_dim and batch must not be negative, lut_count and levels >= 1")
        return lib().cntt_native_cmux_tree_workspace_bytes(self._h, lut_count, glwe_dim, levels, batch)

    def glwe_cmux_batch(self, glwe_out, glwe0, glwe1, ggsw_residues, glwe_dim, base_log, levels, workspace=None):
        """glwe_out[b] = glwe0[b] + ExtProd(ggsw, glwe1[b] - glwe0[b]) mod 2^w: glwe0[b] where the selector encrypts 0, glwe1[b] where it
        encrypts 1.  The words of the copy of glwe0, gadget_decompose_batch(mode="plain") of the difference and
        external_product_batch(accumulate=True).  ggsw_residues: ONE selector as NPRIMES buffers of (glwe_dim+1)*levels*(glwe_dim+1)
        residue polynomials as fwd_batch writes them, the layout of one iteration's slice of the bootstrapping key, shared by the batch;
        workspace: None (one allocation per call) or a buffer of glwe_cmux_workspace_bytes()."""
        op, oc, where, stream = self._words(glwe_out)
        ap, ac, aw, _ = self._words(glwe0)
        bp, bc, bw, _ = self._words(glwe1)
        per = (glwe_dim + 1) * self._n
        if glwe_dim < 0 or levels <= 0 or base_log <= 0 or ac % per or oc != ac or bc != ac or aw != where or bw != where:
            raise Panic("glwe0, glwe1 and glwe_out: batch*(glwe_dim+1) polynomials each in the same memory; base_log, levels >= 1")
        keys = self._planes(ggsw_residues, where, (glwe_dim + 1) * levels * per, "ggsw")
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_glwe_cmux_batch(self._h, op, ap, bp, keys, glwe_dim, base_log, levels, ac // per, wp, wb, where, stream))

    def cmux_tree_batch(self, glwe_out, lut_in, ggsw_residues, lut_count, glwe_dim, base_log, levels, workspace=None):
        """Selects one of lut_count (a power of two) PLAIN table polynomials per batch element by log2(lut_count) GGSW selectors:
        glwe_out[b] = the trivial encryption of lut_in[b][a] plus noise, a = sum bit_i*2^i, selector i (address bit i, LSB first) at
        residue polynomial i*(glwe_dim+1)*levels*(glwe_dim+1) of every buffer of ggsw_residues.  Stage 1 takes the table entries as they
        are (zero masks are never decomposed), stages >= 2 are glwe_cmux_batch word for word; the top bit is consumed first.  lut_in:
        batch*lut_count polynomials; glwe_out: batch*(glwe_dim+1) polynomials; ggsw_residues may be None when lut_count == 1; workspace:
        None or a buffer of cmux_tree_workspace_bytes()."""
        ip, ic, where, stream = self._words(lut_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or lut_count <= 0 or lut_count & (lut_count - 1) or levels <= 0 or base_log <= 0 or ic % (lut_count * n) or ow != where:
            raise Panic("lut_in: batch*lut_count polynomials; glwe_out in the same memory; lut_count a power of two; base_log, levels >= 1")
        batch = ic // (lut_count * n)
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        keys = None
        depth = lut_count.bit_length() - 1
        if depth:
            if ggsw_residues is None:
                raise Panic("ggsw_residues may be None only when lut_count == 1")
            keys = self._planes(ggsw_residues, where, depth * (glwe_dim + 1) * levels * (glwe_dim + 1) * n, "ggsw")
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_cmux_tree_batch(self._h, op, ip, keys, lut_count, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- ring automorphism, Galois keyswitch and trace (include/cntt_automorphism.h) -----------------------------------------------------
    def automorphism_batch(self, out, inp, t):
        """out = sigma_t(inp): X -> X^t on coefficient-domain polynomials mod 2^w, t odd and below 2n.  inp, out: the same number of
        polynomials in the same memory; out is only written and may not overlap inp."""
        op, oc, where, stream = self._words(out)
        ip, ic, iw, _ = self._words(inp)
        if oc % self._n or ic != oc or iw != where or t < 0:
            raise Panic("out and inp: the same whole number of polynomials in the same memory; t >= 0")
        check(lib().cntt_native_automorphism_batch(self._h, op, ip, t, 1, oc // self._n, where, stream))

    def automorphism_ntt_batch(self, out_residues, in_residues, t):
        """The same map as a slot permutation of every residue plane: NPRIMES buffers in, NPRIMES buffers out, each of the same whole
        number of residue polynomials.  inv_batch of the result is sigma_t of what the planes stand for."""
        if len(in_residues) != self.NPRIMES or len(out_residues) != self.NPRIMES:
            raise Panic("expected %d residue buffers in and out" % self.NPRIMES)
        _, count, _, where, stream = buffer_info(out_residues[0])
        if count % self._n or t < 0:
            raise Panic("residue buffers: a whole number of residue polynomials; t >= 0")
        outs = self._planes(out_residues, where, count, "out")
        ins = self._planes(in_residues, where, count, "in")
        check(lib().cntt_native_automorphism_ntt_batch(self._h, outs, ins, t, 1, count // self._n, where, stream))

    def glwe_automorphism_keyswitch_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_automorphism_keyswitch_batch needs: the negated digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return lib().cntt_native_glwe_automorphism_keyswitch_workspace_bytes(self._h, glwe_dim, levels, batch)

    def glwe_trace_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_trace_batch needs: the negated digit polynomials and a second ciphertext batch, each rounded up to 256
        bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return lib().cntt_native_glwe_trace_workspace_bytes(self._h, glwe_dim, levels, batch)

    def _autoks(self, glwe_out, glwe_in, ak_residues, keys_count, glwe_dim, base_log, levels):
        op, oc, where, stream = self._words(glwe_out)
        ip, ic, iw, _ = self._words(glwe_in)
        per = (glwe_dim + 1) * self._n
        if glwe_dim < 0 or levels <= 0 or base_log <= 0 or ic % per or oc != ic or iw != where:
            raise Panic("glwe_in and glwe_out: batch*(glwe_dim+1) polynomials each in the same memory; base_log, levels >= 1")
        keys = None
        if glwe_dim and keys_count:
            if ak_residues is None:
                raise Panic("ak_residues may be None only when glwe_dim == 0 (or steps == 0)")
            keys = self._planes(ak_residues, where, keys_count * glwe_dim * levels * per, "ak")
        return op, ip, keys, ic // per, where, stream

    def glwe_automorphism_keyswitch_batch(self, glwe_out, glwe_in, ak_residues, t, glwe_dim, base_log, levels, add_input=False, workspace=None):
        """The Galois keyswitch mod 2^w: glwe_out[b] = (glwe_in[b] if add_input) + the GLWE ciphertext under the same key of
        sigma_t(phase(glwe_in[b])).  The words of the prefill, automorphism_batch on the masks, gadget_decompose_batch(mode="plain"), the
        negation of the digits and external_product_batch(accumulate=True).  ak_residues: NPRIMES buffers of
        glwe_dim*levels*(glwe_dim+1) residue polynomials as fwd_batch writes them (None when glwe_dim == 0); workspace: None (one
        allocation per call) or a buffer of glwe_automorphism_keyswitch_workspace_bytes().  Not on the binary kinds."""
        if t < 0:
            raise Panic("t >= 0")
        op, ip, keys, batch, where, stream = self._autoks(glwe_out, glwe_in, ak_residues, 1, glwe_dim, base_log, levels)
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_glwe_automorphism_keyswitch_batch(self._h, op, ip, keys, t, glwe_dim, base_log, levels, 1 if add_input else 0, batch,
                                                                  wp, wb, where, stream))

    def glwe_trace_batch(self, glwe_out, glwe_in, ak_residues, steps, glwe_dim, base_log, levels, workspace=None):
        """`steps` <= log2 n stages cur <- cur + AutoKS_(n/2^r + 1)(cur): coefficient i of the phase becomes 2^steps*phase[i] mod 2^w where
        2^steps divides i and 0 elsewhere (plus keyswitch noise) -- 2^steps is not a unit mod 2^w, so encode with `steps` bits of headroom
        below the message.  ak_residues: NPRIMES buffers of steps*glwe_dim*levels*(glwe_dim+1) residue polynomials, key r at polynomial
        r*glwe_dim*levels*(glwe_dim+1); workspace: None or a buffer of glwe_trace_workspace_bytes()."""
        if steps < 0:
            raise Panic("steps >= 0")
        op, ip, keys, batch, where, stream = self._autoks(glwe_out, glwe_in, ak_residues, steps, glwe_dim, base_log, levels)
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_glwe_trace_batch(self._h, op, ip, keys, steps, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- ring packing of LWE ciphertexts through automorphisms (include/cntt_ring_pack.h) -------------------------------------------------
    def glwe_merge_workspace_bytes(self, glwe_dim, levels, batch):
        """Bytes of workspace glwe_merge_batch needs: the negated digit polynomials, rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0:
            raise Panic("glwe_dim and batch must not be negative, levels >= 1")
        return lib().cntt_native_glwe_merge_workspace_bytes(self._h, glwe_dim, levels, batch)

    def ring_pack_workspace_bytes(self, lwe_count, glwe_dim, levels, batch):
        """Bytes of workspace ring_pack_batch needs: the digits of the widest stage and two ciphertext buffers of
        batch*max(lwe_count/2, 1) and batch*max(lwe_count/4, 1) ciphertexts, each rounded up to 256 bytes."""
        if min(glwe_dim, batch) < 0 or levels <= 0 or lwe_count <= 0:
            raise Panic("glwe_dim and batch must not be negative, lwe_count and levels >= 1")
        return lib().cntt_native_ring_pack_workspace_bytes(self._h, lwe_count, glwe_dim, levels, batch)

    def glwe_embed_batch(self, glwe_out, lwe_in, glwe_dim):
        """The inverse of sample_extract_batch(index=0): glwe[q][0] = lwe[q*n], glwe[q][i] = -lwe[q*n + n - i] mod 2^w, body
        (lwe[glwe_dim*n], 0, ..., 0).  lwe_in: batch*(glwe_dim*n + 1) words; glwe_out: batch*(glwe_dim + 1) polynomials, only written.
        Every kind."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or ic % (glwe_dim * n + 1) or ow != where or oc != ic // (glwe_dim * n + 1) * (glwe_dim + 1) * n:
            raise Panic("lwe_in: batch*(glwe_dim*n+1) words; glwe_out: batch*(glwe_dim+1) polynomials in the same memory")
        check(lib().cntt_native_glwe_embed_batch(self._h, op, ip, glwe_dim, ic // (glwe_dim * n + 1), where, stream))

    def glwe_merge_batch(self, glwe_out, glwe_even, glwe_odd, ak_residues, shift, t, glwe_dim, base_log, levels, workspace=None):
        """One node of the packing tree: glwe_out[b] = a + AutoKS_t(d) with a = even[b] + X^shift odd[b], d = even[b] - X^shift odd[b]
        mod 2^w; the words of the prefill (a, body plus sigma_t(d body)), the negated digits of sigma_t(d mask) and
        external_product_batch(accumulate=True) against the ONE key ak_residues of glwe_automorphism_keyswitch_batch's layout (None when
        glwe_dim == 0).  0 <= shift < 2n, t odd below 2n; workspace: None (one allocation per call) or a buffer of
        glwe_merge_workspace_bytes().  Not on the binary kinds."""
        op, ep, keys, batch, where, stream = self._autoks(glwe_out, glwe_even, ak_residues, 1, glwe_dim, base_log, levels)
        dp, dc, dw, _ = self._words(glwe_odd)
        if dw != where or dc != batch * (glwe_dim + 1) * self._n or shift < 0 or t < 0:
            raise Panic("glwe_odd: batch*(glwe_dim+1) polynomials in the memory of the other buffers; shift, t >= 0")
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_glwe_merge_batch(self._h, op, ep, dp, keys, shift, t, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    def ring_pack_batch(self, glwe_out, lwe_in, ak_residues, lwe_count, glwe_dim, base_log, levels, workspace=None):
        """Packs lwe_count (a power of two <= n) LWE ciphertexts of glwe_dim*n + 1 words, encrypted under the flattened GLWE key, into one
        GLWE ciphertext: glwe_embed_batch, log2(lwe_count) stages of glwe_merge_batch (shift n/2^s, t = 2^s + 1, key log2(n) - s) and
        glwe_trace_batch with log2(n) - log2(lwe_count) steps, word for word.  MESSAGE j SITS AT COEFFICIENT j*n/lwe_count (a strided
        layout) and carries the factor n: the phase there is n*phase(lwe_j) mod 2^w and every other coefficient is 0 with noise-free keys.
        n is not a unit mod 2^w: encode with log2(n) bits of headroom below the message.  lwe_in: batch*lwe_count*(glwe_dim*n + 1) words;
        glwe_out: batch*(glwe_dim+1) polynomials; ak_residues: NPRIMES buffers of all log2(n) trace keys back to back (None when
        glwe_dim == 0); workspace: None or a buffer of ring_pack_workspace_bytes().  Not on the binary kinds."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(glwe_out)
        n = self._n
        if glwe_dim < 0 or lwe_count <= 0 or levels <= 0 or base_log <= 0 or ic % (lwe_count * (glwe_dim * n + 1)) or ow != where:
            raise Panic("lwe_in: batch*lwe_count*(glwe_dim*n+1) words; glwe_out in the same memory; lwe_count, base_log, levels >= 1")
        batch = ic // (lwe_count * (glwe_dim * n + 1))
        if oc != batch * (glwe_dim + 1) * n:
            raise Panic("glwe_out must hold batch*(glwe_dim+1) = %d polynomials" % (batch * (glwe_dim + 1)))
        keys = None
        if glwe_dim:
            if ak_residues is None:
                raise Panic("ak_residues may be None only when glwe_dim == 0")
            keys = self._planes(ak_residues, where, (n.bit_length() - 1) * glwe_dim * levels * (glwe_dim + 1) * n, "ak")
        wp, wb = self._workspace(workspace, where)
        check(lib().cntt_native_ring_pack_batch(self._h, op, ip, keys, lwe_count, glwe_dim, base_log, levels, batch, wp, wb, where, stream))

    # -- the circuit bootstrap from LWE bits to GGSW selectors (include/cntt_cbs.h) ------------------------------------------------------
    def circuit_bootstrap_workspace_bytes(self, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch):
        """Bytes of workspace circuit_bootstrap_batch needs: rot_t, the tables, the digits of the rotation and the accumulators of the
        batch*cbs_levels bootstrap elements, their int32 keyswitch digits, the slab sums and the selector words, each rounded up to 256
        bytes."""
        return self._cbs_workspace_bytes("circuit_bootstrap_workspace_bytes", lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch)

    def _circuit_bootstrap(self, ggsw_residues_out, lwe_in, bsk_residues, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                           ks_levels, cbs_base_log, cbs_levels, workspace, log_lut_count=None):
        """circuit_bootstrap_batch, and with a log_lut_count circuit_bootstrap_manylut_batch."""
        one = () if log_lut_count is None else (log_lut_count,)
        ip, ic, where, stream = self._words(lwe_in)
        n = self._n
        if min(lwe_dim, glwe_dim, *one) < 0 or min(pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels) <= 0 \
                or ic % (lwe_dim + 1):
            raise Panic("lwe_in: batch*(lwe_dim+1) words; every base_log and levels >= 1" + ("; log_lut_count >= 0" if one else ""))
        batch = ic // (lwe_dim + 1)
        outs = self._planes(ggsw_residues_out, where, batch * (glwe_dim + 1) * cbs_levels * (glwe_dim + 1) * n, "ggsw_residues_out")
        if lwe_dim and bsk_residues is None:
            raise Panic("bsk_residues may be None only when lwe_dim == 0")
        keys = self._bsk(bsk_residues, where, lwe_dim, glwe_dim, pbs_levels) if lwe_dim else None
        fp, fc, fw, _ = self._words(fpksk)
        if fw != where or fc != (glwe_dim + 1) * (glwe_dim * n + 1) * ks_levels * (glwe_dim + 1) * n:
            raise Panic("fpksk: (glwe_dim+1) keys of (glwe_dim*n+1)*ks_levels*(glwe_dim+1) polynomials of words in the memory of the other "
                        "buffers")
        wp, wb = self._workspace(workspace, where)
        call = self._fn("circuit_bootstrap_manylut_batch" if one else "circuit_bootstrap_batch")
        check(call(self._h, outs, ip, keys, fp, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log, ks_levels, cbs_base_log, cbs_levels,
                   *one, batch, wp, wb, where, stream))

    def circuit_bootstrap_batch(self, ggsw_residues_out, lwe_in, bsk_residues, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                ks_levels, cbs_base_log, cbs_levels, workspace=None):
        """LWE encryptions of bits (phase bit*2^(w-1) + e) -> GGSW selectors as residue planes, the ggsw_residues argument of
        cmux_tree_batch: element b of lwe_in (batch*(lwe_dim+1) words) becomes selector b of every buffer of ggsw_residues_out (NPRIMES
        buffers of batch*(glwe_dim+1)*cbs_levels*(glwe_dim+1) residue polynomials, written only).  One bootstrap per level against the
        constant table -H_l, then the functional keyswitch as a wrapping digit x key sum against fpksk: glwe_dim+1 keys of
        (glwe_dim*n+1)*ks_levels*(glwe_dim+1) polynomials of PLAIN words in the coefficient domain, 16-byte aligned; then fwd_batch.
        bsk_residues as in bootstrap_batch (None when lwe_dim == 0); workspace: None (one allocation per call) or a buffer of
        circuit_bootstrap_workspace_bytes().  Not on the binary kinds."""
        self._circuit_bootstrap(ggsw_residues_out, lwe_in, bsk_residues, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                ks_levels, cbs_base_log, cbs_levels, workspace)

    # -- the many-LUT bootstrap and the circuit bootstrap with one rotation per input bit (include/cntt_manylut.h) ----------------------
    #    lwe_modswitch_manylut_batch and sample_extract_many_batch are PbsMixin's
    def bootstrap_manylut_batch(self, lwe_out, lwe_in, lut, bsk_residues, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count,
                                workspace=None, lut_per_element=None):
        """lwe_modswitch_manylut_batch -> blind_rotate_batch -> sample_extract_many_batch(count=lut_count) in one call: lut_count <=
        2^log_lut_count functions of every encrypted message for one rotation, function h at the coefficients m*2^log_lut_count + h of
        the table.  lwe_in: batch*(lwe_dim+1) words; lwe_out: batch*lut_count*(glwe_dim*n+1) words; workspace: None (one allocation per
        call) or a buffer of pbs_workspace_bytes()."""
        self._bootstrap_manylut(lwe_out, lwe_in, lut, bsk_residues, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count, workspace,
                                lut_per_element)

    def circuit_bootstrap_manylut_workspace_bytes(self, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch):
        """Bytes of workspace circuit_bootstrap_manylut_batch needs: rot_t, the shared table, the digits of the rotation and the
        accumulators of the batch elements, the int32 keyswitch digits, the slab sums and the selector words of the batch*cbs_levels
        selector rows, each rounded up to 256 bytes."""
        return self._cbs_workspace_bytes("circuit_bootstrap_manylut_workspace_bytes", lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels,
                                         batch)

    def circuit_bootstrap_manylut_batch(self, ggsw_residues_out, lwe_in, bsk_residues, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels,
                                        ks_base_log, ks_levels, cbs_base_log, cbs_levels, log_lut_count, workspace=None):
        """circuit_bootstrap_batch with ONE blind rotation per input bit: the cbs_levels constants -H_l are interleaved in one shared
        table, the modulus switch clears the low log_lut_count bits, and level l is extracted at the index l - 1.  cbs_levels <=
        2^log_lut_count <= n/2.  The buffers are those of circuit_bootstrap_batch; workspace: None (one allocation per call) or a buffer
        of circuit_bootstrap_manylut_workspace_bytes().  Not on the binary kinds."""
        self._circuit_bootstrap(ggsw_residues_out, lwe_in, bsk_residues, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                ks_levels, cbs_base_log, cbs_levels, workspace, log_lut_count)


def _make(kind, nprimes, word, res, binary, doc):
    return type("Plan", (NativePlan,), {"KIND": kind, "NPRIMES": nprimes, "WORD": word, "RES": res,
                                        "BINARY": binary, "__doc__": doc})
