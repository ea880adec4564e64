"""Gadget decomposition and the programmable bootstrap over the C ABI, once for the native plans (include/cntt_pbs.h: the ring
Z/2^w[X]/(X^n+1), modulus switch rounding ties up) and the prime plans (include/cntt_prime_pbs.h: Z_p[X]/(X^n+1), digits of the balanced
lift stored canonically mod p, modulus switch exact).  The shape checks and the calls are the same; each plan class says how it differs."""
from ._lib import Panic, buffer_info, check


class PbsMixin:
    """What the host class supplies:
    _words(buf) -> (pointer, word count, memory, stream) of a buffer of the plan's words;
    _bsk(key, where, lwe_dim, glwe_dim, levels) -> the bootstrapping key as the C call takes it, its shape and memory checked;
    _bsk_mb(key, where, lwe_dim, glwe_dim, levels, grouping) -> the same for the multi-bit key;
    _fn(name) -> the C entry point `name` of the plan's family;
    blind_rotate_batch and bootstrap_batch, which name the key argument their way and pass on to _blind_rotate / _bootstrap, and their
    multibit_* forms, which pass a `grouping` as well; bootstrap_manylut_batch, which does the same with _bootstrap_manylut;
    the two circuit_bootstrap*_workspace_bytes, which say what their parts are and pass on to _cbs_workspace_bytes.  The circuit bootstrap
    itself stays with the plan classes: its output, its keys and every message about them differ."""

    SRC_MODES = {"plain": 0, "rotate": 1, "cmux": 2}

    def _rot(self, rot, where, what):
        rp, rc_, esz, rw, _ = buffer_info(rot)
        if esz != 4 or rw != where:
            raise Panic("%s: uint32 exponents in the memory of the other buffers" % what)
        return rp, rc_

    def _src(self, polys, rot, mode):
        """(polys pointer, word count, memory, stream, (rot pointer, length) or None, mode number) with the checks every call with a
        source polynomial shares."""
        if mode not in self.SRC_MODES:
            raise Panic("mode must be one of %s" % sorted(self.SRC_MODES))
        pp, pc, where, stream = self._words(polys)
        rp = None
        if rot is not None:
            rp = self._rot(rot, where, "rot")
        elif mode != "plain":
            raise Panic("mode %r needs rot" % mode)
        return pp, pc, where, stream, rp, self.SRC_MODES[mode]

    def gadget_decompose_batch(self, terms, polys, base_log, levels, rot=None, mode="plain"):
        """terms[b][q*levels + l-1] = signed digit l (of `levels`, base_log bits each, d_1 most significant) of the source polynomial of
        polys[b][q]: polys itself ("plain"), X^rot[b] * polys ("rotate") or X^rot[b] * polys - polys ("cmux") in the plan's ring.  Prime
        plans: the digits of the balanced lift, d_1 unmasked, stored canonically mod p.  polys: batch*npolys polynomials; terms:
        batch*npolys*levels; npolys is taken from len(rot) = batch when rot is given, else 1."""
        pp, pc, where, stream, rp, m = self._src(polys, rot, mode)
        tp, tc, tw, _ = self._words(terms)
        n = self._n
        if levels <= 0 or base_log <= 0 or pc % n or tw != where or tc != pc * levels:
            raise Panic("polys: batch*npolys polynomials; terms: levels times as many in the same memory; base_log, levels >= 1")
        batch = rp[1] if rp else pc // n
        if batch == 0 or (pc // n) % batch:
            if pc:
                raise Panic("polys must hold a whole number of polynomials per exponent in rot")
            batch = 0
        npolys = (pc // n) // batch if batch else 0
        check(self._fn("gadget_decompose_batch")(self._h, tp, pp, rp[0] if rp else None, npolys, base_log, levels, m, batch, where, stream))

    def pbs_workspace_bytes(self, lwe_dim, glwe_dim, levels, batch):
        """Bytes of workspace bootstrap_batch needs (digits + rot_t + accumulator, each 256-byte aligned); enough for
        blind_rotate_batch too."""
        if min(lwe_dim, glwe_dim, levels, batch) < 0:
            raise Panic("lwe_dim, glwe_dim, levels and batch must not be negative")
        return self._fn("pbs_workspace_bytes")(self._h, lwe_dim, glwe_dim, levels, batch)

    def _workspace(self, workspace, where):
        if workspace is None:
            return None, 0
        ptr, count, esz, w, _ = buffer_info(workspace)
        if w != where:
            raise Panic("workspace must live in the memory of the other buffers")
        return ptr, count * esz

    def _lut(self, lut, lut_per_element, where, glwe_dim, batch):
        lp, lc, lw, _ = self._words(lut)
        shared, each = (glwe_dim + 1) * self._n, batch * (glwe_dim + 1) * self._n
        if lut_per_element is None:
            lut_per_element = lc == each and lc != shared
        if lw != where or lc != (each if lut_per_element else shared):
            raise Panic("lut: glwe_dim+1 polynomials shared by the batch, or batch*(glwe_dim+1) with lut_per_element, in the memory "
                        "of the other buffers")
        return lp, 1 if lut_per_element else 0

    def lwe_modswitch_batch(self, rot_t, lwe, lwe_dim):
        """rot_t[i*batch + b] = round(lwe[b][i] * 2n / q) mod 2n for the lwe_dim mask words, and 2n minus that for the body in row
        lwe_dim; q = 2^w with ties rounded up (native plans), q = p, odd, so exact without ties (prime plans).  lwe: batch*(lwe_dim+1)
        words; rot_t: (lwe_dim+1)*batch uint32, transposed: row i is iteration i's rot."""
        lp, lc, where, stream = self._words(lwe)
        if lwe_dim < 0 or lc % (lwe_dim + 1):
            raise Panic("lwe: batch*(lwe_dim+1) words; rot_t: as many uint32 in the same memory")
        rp, rc_ = self._rot(rot_t, where, "rot_t")
        if rc_ != lc:
            raise Panic("lwe: batch*(lwe_dim+1) words; rot_t: as many uint32 in the same memory")
        check(self._fn("lwe_modswitch_batch")(self._h, rp, lp, lwe_dim, lc // (lwe_dim + 1), where, stream))

    def multibit_pbs_workspace_bytes(self, lwe_dim, glwe_dim, levels, grouping, batch):
        """Bytes of workspace multibit_bootstrap_batch needs (digits + the family's scratch + rot_t + accumulator, each 256-byte aligned:
        the plan class says what the scratch is); enough for multibit_blind_rotate_batch too."""
        if min(lwe_dim, glwe_dim, levels, grouping, batch) < 0:
            raise Panic("lwe_dim, glwe_dim, levels, grouping and batch must not be negative")
        return self._fn("multibit_pbs_workspace_bytes")(self._h, lwe_dim, glwe_dim, levels, grouping, batch)

    def _key_call(self, name, bsk, where, lwe_dim, glwe_dim, levels, grouping):
        """(the key as the C call takes it, the entry point, what it takes between levels and batch): the classic call, or with a
        `grouping` its multi-bit form."""
        if grouping is None:
            return self._bsk(bsk, where, lwe_dim, glwe_dim, levels), self._fn(name), ()
        return self._bsk_mb(bsk, where, lwe_dim, glwe_dim, levels, grouping), self._fn("multibit_" + name), (grouping,)

    def _blind_rotate(self, acc, lut, rot_t, bsk, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping=None):
        """blind_rotate_batch and multibit_blind_rotate_batch (`grouping` given) of the plan classes, which name and describe the key."""
        ap, ac, where, stream = self._words(acc)
        n = self._n
        if lwe_dim < 0 or glwe_dim < 0 or levels <= 0 or base_log <= 0 or (grouping or 0) < 0 or ac % ((glwe_dim + 1) * n):
            raise Panic("acc: batch*(glwe_dim+1) polynomials; base_log, levels >= 1")
        batch = ac // ((glwe_dim + 1) * n)
        rp, rc_ = self._rot(rot_t, where, "rot_t")
        if rc_ != (lwe_dim + 1) * batch:
            raise Panic("rot_t: (lwe_dim+1)*batch uint32 in the memory of acc")
        lp, per = self._lut(lut, lut_per_element, where, glwe_dim, batch)
        key, call, g = self._key_call("blind_rotate_batch", bsk, where, lwe_dim, glwe_dim, levels, grouping)
        wp, wb = self._workspace(workspace, where)
        check(call(self._h, ap, lp, per, rp, key, lwe_dim, glwe_dim, base_log, levels, *g, batch, wp, wb, where, stream))

    def sample_extract_batch(self, lwe_out, glwe, glwe_dim, index=0):
        """lwe_out[b] = the LWE ciphertext (glwe_dim*n mask words, body last) of coefficient `index` of glwe[b] (glwe_dim+1 polynomials),
        negations in the plan's ring."""
        gp, gc, where, stream = self._words(glwe)
        op, oc, ow, _ = self._words(lwe_out)
        n = self._n
        if glwe_dim < 0 or index < 0 or gc % ((glwe_dim + 1) * n) or ow != where or oc != gc // ((glwe_dim + 1) * n) * (glwe_dim * n + 1):
            raise Panic("glwe: batch*(glwe_dim+1) polynomials; lwe_out: batch*(glwe_dim*n+1) words in the same memory")
        check(self._fn("sample_extract_batch")(self._h, op, gp, glwe_dim, index, gc // ((glwe_dim + 1) * n), where, stream))

    def _bootstrap(self, lwe_out, lwe_in, lut, bsk, lwe_dim, glwe_dim, base_log, levels, workspace, lut_per_element, grouping=None):
        """bootstrap_batch and multibit_bootstrap_batch (`grouping` given) of the plan classes, which name the key."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(lwe_out)
        n = self._n
        if lwe_dim < 0 or glwe_dim < 0 or levels <= 0 or base_log <= 0 or (grouping or 0) < 0 or ic % (lwe_dim + 1) or ow != where:
            raise Panic("lwe_in: batch*(lwe_dim+1) words; lwe_out in the same memory; base_log, levels >= 1")
        batch = ic // (lwe_dim + 1)
        if oc != batch * (glwe_dim * n + 1):
            raise Panic("lwe_out must hold batch*(glwe_dim*n+1) = %d words" % (batch * (glwe_dim * n + 1)))
        lp, per = self._lut(lut, lut_per_element, where, glwe_dim, batch)
        key, call, g = self._key_call("bootstrap_batch", bsk, where, lwe_dim, glwe_dim, levels, grouping)
        wp, wb = self._workspace(workspace, where)
        check(call(self._h, op, ip, lp, per, key, lwe_dim, glwe_dim, base_log, levels, *g, batch, wp, wb, where, stream))

    # -- the many-LUT calls (include/cntt_manylut.h, cntt_prime_manylut.h) ----------------------------------------------------------------
    def lwe_modswitch_manylut_batch(self, rot_t, lwe, lwe_dim, log_lut_count):
        """lwe_modswitch_batch with the coarse rule: every exponent is round(lwe[b][i] * 2n' / q) mod 2n' for n' = n / 2^log_lut_count
        (q = 2^w with ties rounded up on the native plans, q = p on the prime plans), shifted left by log_lut_count, so its low
        log_lut_count bits are clear; the body row negated mod 2n.  log_lut_count = 0 is lwe_modswitch_batch word for word."""
        lp, lc, where, stream = self._words(lwe)
        if lwe_dim < 0 or log_lut_count < 0 or lc % (lwe_dim + 1):
            raise Panic("lwe: batch*(lwe_dim+1) words; rot_t: as many uint32 in the same memory; log_lut_count >= 0")
        rp, rc_ = self._rot(rot_t, where, "rot_t")
        if rc_ != lc:
            raise Panic("lwe: batch*(lwe_dim+1) words; rot_t: as many uint32 in the same memory")
        check(self._fn("lwe_modswitch_manylut_batch")(self._h, rp, lp, lwe_dim, log_lut_count, lc // (lwe_dim + 1), where, stream))

    def sample_extract_many_batch(self, lwe_out, glwe, glwe_dim, count):
        """lwe_out[b][h] = sample_extract_batch(glwe[b], index=h) for h < count, from one read of glwe: lwe_out holds
        batch*count*(glwe_dim*n+1) words, glwe batch*(glwe_dim+1) polynomials; 1 <= count <= n."""
        gp, gc, where, stream = self._words(glwe)
        op, oc, ow, _ = self._words(lwe_out)
        n = self._n
        if glwe_dim < 0 or count <= 0 or gc % ((glwe_dim + 1) * n) or ow != where \
                or oc != gc // ((glwe_dim + 1) * n) * count * (glwe_dim * n + 1):
            raise Panic("glwe: batch*(glwe_dim+1) polynomials; lwe_out: batch*count*(glwe_dim*n+1) words in the same memory; count >= 1")
        check(self._fn("sample_extract_many_batch")(self._h, op, gp, glwe_dim, count, gc // ((glwe_dim + 1) * n), where, stream))

    def _bootstrap_manylut(self, lwe_out, lwe_in, lut, bsk, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count, workspace,
                           lut_per_element):
        """bootstrap_manylut_batch of the plan classes, which name the key."""
        ip, ic, where, stream = self._words(lwe_in)
        op, oc, ow, _ = self._words(lwe_out)
        n = self._n
        if lwe_dim < 0 or glwe_dim < 0 or levels <= 0 or base_log <= 0 or log_lut_count < 0 or lut_count <= 0 or ic % (lwe_dim + 1) \
                or ow != where:
            raise Panic("lwe_in: batch*(lwe_dim+1) words; lwe_out in the same memory; base_log, levels, lut_count >= 1; log_lut_count >= 0")
        batch = ic // (lwe_dim + 1)
        if oc != batch * lut_count * (glwe_dim * n + 1):
            raise Panic("lwe_out must hold batch*lut_count*(glwe_dim*n+1) = %d words" % (batch * lut_count * (glwe_dim * n + 1)))
        lp, per = self._lut(lut, lut_per_element, where, glwe_dim, batch)
        kp = self._bsk(bsk, where, lwe_dim, glwe_dim, levels)
        wp, wb = self._workspace(workspace, where)
        check(self._fn("bootstrap_manylut_batch")(self._h, op, ip, lp, per, kp, lwe_dim, glwe_dim, base_log, levels, log_lut_count, lut_count,
                                                  batch, wp, wb, where, stream))

    def _cbs_workspace_bytes(self, name, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch):
        """circuit_bootstrap_workspace_bytes and circuit_bootstrap_manylut_workspace_bytes (`name`) of the plan classes, which say what
        the parts are."""
        if min(lwe_dim, glwe_dim, batch) < 0 or min(pbs_levels, ks_levels, cbs_levels) <= 0:
            raise Panic("lwe_dim, glwe_dim and batch must not be negative, pbs_levels, ks_levels and cbs_levels >= 1")
        return self._fn(name)(self._h, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch)
