// The host side of what works on LWE ciphertexts around the bootstrap, once for the native plans (include/cntt_keyswitch.h, cntt_pack.h;
// host_native_ext.hip) and the prime plans (include/cntt_prime_keyswitch.h, cntt_prime_pack.h; host_prime.hip): the LWE keyswitch, the
// keyswitch + bootstrap call and the LWE-to-GLWE packing keyswitch -- argument checks, the workspace layout and the chunk loop, each
// call on one path for device pointers and host slices through Staging (host_common.hpp).  Internal, never installed.  Templates over a family F as in pbs_host.hpp, which this file builds on: the bootstrap
// family plus the members the second half of NativePbs (host_native_ext.hip) and PrimeKs<T> / PrimePack<T> (host_prime_keyswitch.inc,
// host_prime_pack.inc) show.
#pragma once
#include "pbs_host.hpp"

#pragma GCC visibility push(hidden)

// ---------------------------------------------------------------------------------------------
// LWE keyswitch
// ---------------------------------------------------------------------------------------------
// the digit and stride checks the two calls share; `pre` = "" or "ks_": how the combined call names the keyswitch's digit arguments.
// F::KS_ROWS_GUARD: the family's kernel indexes the key rows in 32 bits
template <class F>
int ks_check(const typename F::Plan *pl, size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels,
             const char *pre) {
    if (int rc = digits_check<F>(pl, pre, base_log, levels)) return rc;
    if (base_log > 31) return fail(CNTT_EINVAL, "%sbase_log = %u exceeds 31: the keyswitch keeps a digit in one 32-bit register", pre, base_log);
    if (row_stride < lwe_dim_out + 1)
        return fail(CNTT_EINVAL, "row_stride = %zu is below lwe_dim_out + 1 = %zu words", row_stride, lwe_dim_out + 1);
    if (F::KS_ROWS_GUARD && (u128)lwe_dim_in * levels >= ((u128)1 << 32))
        return fail(CNTT_EINVAL, "lwe_dim_in * %slevels = %zu * %u is not below 2^32 key rows", pre, lwe_dim_in, levels);
    return CNTT_OK;
}
// bytes of a key of `rows` rows: the last row needs its lwe_dim_out + 1 words only
template <class F> size_t ksk_bytes(const typename F::Plan *pl, size_t rows, size_t lwe_dim_out, size_t row_stride) {
    return rows ? ((rows - 1) * row_stride + lwe_dim_out + 1) * F::word(pl) : 0;
}
template <class F>
int keyswitch_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *in, const typename F::Word *ksk, size_t lin,
                     size_t lout, size_t row_stride, unsigned base_log, unsigned levels, size_t batch, hipStream_t st) {
    const hipError_t e = F::launch_keyswitch(pl, out, in, ksk, lin, lout, row_stride, base_log, levels, batch, st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_keyswitch_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    return CNTT_OK;
}

template <class F>
int keyswitch(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *ksk,
              size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride, unsigned base_log, unsigned levels, size_t batch, cntt_mem_t where,
              hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = ks_check<F>(pl, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, "")) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim_in && !ksk) return fail(CNTT_EINVAL, "ksk is NULL");
    const size_t w = F::word(pl), ob = batch * (lwe_dim_out + 1) * w, ib = batch * (lwe_dim_in + 1) * w;
    const size_t kb = ksk_bytes<F>(pl, lwe_dim_in * levels, lwe_dim_out, row_stride);
    if (ranges_overlap(lwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "lwe_out overlaps lwe_in");
    if (ranges_overlap(lwe_out, ob, ksk, kb)) return fail(CNTT_EINVAL, "lwe_out overlaps ksk");
    Staging s(where, st);
    W *dout = (W *)s.out(lwe_out, ob);
    const W *din = (const W *)s.in(lwe_in, ib), *dk = (const W *)s.in(ksk, kb);
    if (int rc = s.status()) return rc;
    if (int rc = keyswitch_device<F>(pl, dout, din, dk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, st)) return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------
// keyswitch from dimension k n to lwe_dim, then the bootstrap, in one call
// ---------------------------------------------------------------------------------------------
// The workspace holds the bootstrap's part (PbsSizes) first and the batch x (lwe_dim + 1) keyswitched ciphertexts behind it.
template <class F> size_t ks_pbs_workspace_bytes(const typename F::Plan *pl, size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) {
    return pl ? pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch).total() + up256(batch * (lwe_dim + 1) * F::word(pl)) : 0;
}

template <class F>
int keyswitch_bootstrap(const typename F::Plan *pl, typename F::Word *lwe_out, const typename F::Word *lwe_in, const typename F::Word *ksk,
                        size_t row_stride, unsigned ks_base_log, unsigned ks_levels, const typename F::Word *lut, int lut_per_element,
                        typename F::Key bsk, size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                        size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    // the rows guard reads the dimension: with it, glwe_dim is bounded before it is multiplied; without, pbs_check below is the first to
    if (F::KS_ROWS_GUARD && glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    const size_t big = glwe_dim * pl->n;   // the dimension of both ends
    if (int rc = ks_check<F>(pl, big, lwe_dim, row_stride, ks_base_log, ks_levels, "ks_")) return rc;
    const PbsSizes Z = pbs_sizes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    const size_t need = ks_pbs_workspace_bytes<F>(pl, lwe_dim, glwe_dim, levels, batch);
    if (int rc = pbs_check<F>(pl, bsk, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, need)) return rc;
    if (batch == 0) return CNTT_OK;
    if (!lwe_out) return fail(CNTT_EINVAL, "lwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (!lut) return fail(CNTT_EINVAL, "lut is NULL");
    if (big && !ksk) return fail(CNTT_EINVAL, "ksk is NULL");
    const size_t eb = batch * (big + 1) * F::word(pl), kb = ksk_bytes<F>(pl, big * ks_levels, lwe_dim, row_stride);
    const size_t lb = lut_per_element ? Z.acc : Z.acc / batch;
    if (ranges_overlap(lwe_out, eb, lwe_in, eb)) return fail(CNTT_EINVAL, "lwe_out overlaps lwe_in");
    if (ranges_overlap(lwe_out, eb, ksk, kb)) return fail(CNTT_EINVAL, "lwe_out overlaps ksk");
    if (ranges_overlap(lwe_out, eb, lut, lb)) return fail(CNTT_EINVAL, "lwe_out overlaps lut");
    if (workspace) {
        if (ranges_overlap(lwe_out, eb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_out overlaps workspace");
        if (ranges_overlap(lwe_in, eb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_in overlaps workspace");
        if (ranges_overlap(ksk, kb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "ksk overlaps workspace");
        if (ranges_overlap(lut, lb, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lut overlaps workspace");
    }
    const size_t bb = F::key_bytes(pl, lwe_dim * (glwe_dim + 1) * levels * (glwe_dim + 1));
    Staging s(where, st);
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim ? F::key_in(pl, s, bsk, bb, ks) : typename F::Key{};
    const W *din = (const W *)s.in(lwe_in, eb), *dk = (const W *)s.in(ksk, kb), *dlut = (const W *)s.in(lut, lb);
    W *dout = (W *)s.out(lwe_out, eb);
    char *dws = (char *)s.workspace(workspace, need);   // one block for the whole call
    if (int rc = s.status()) return rc;
    // keyswitch into the tail of the workspace, bootstrap from there with the head
    W *lwe_mid = static_cast<W *>(static_cast<void *>(dws + Z.total()));
    if (int rc = keyswitch_device<F>(pl, lwe_mid, din, dk, big, lwe_dim, row_stride, ks_base_log, ks_levels, batch, st)) return rc;
    if (int rc = bootstrap_device<F>(pl, dout, lwe_mid, dlut, lut_per_element != 0, dkey, lwe_dim, glwe_dim, base_log, levels, batch, Z, dws, st))
        return rc;
    return s.finish();
}

// ---------------------------------------------------------------------------------------------
// LWE-to-GLWE packing keyswitch through the NTT
// ---------------------------------------------------------------------------------------------
// mask words of one external product: C of the headers, capped at lin (levels >= 1)
template <class F> size_t pack_chunk(const typename F::Plan *pl, size_t lin, unsigned levels) {
    return std::min(std::max<size_t>(1, F::pack_chunk_terms(pl) / levels), lin);
}
template <class F> size_t pack_workspace_bytes(const typename F::Plan *pl, size_t lin, unsigned levels, size_t batch) {
    return pl && levels ? up256(batch * pack_chunk<F>(pl, lin, levels) * levels * pl->n * F::word(pl)) : 0;
}

// out = the body polynomial, then per chunk of mask words the negated digit polynomials into `terms` and the external product
// accumulating into out.  In place is sound as in blind_rotate_device (pbs_host.hpp): a chunk's terms are complete before its product starts
// and rewritten only after it (stream order), and the product reads only the terms and the key.
template <class F>
int pack_device(const typename F::Plan *pl, typename F::Word *out, const typename F::Word *in, typename F::Key pksk, size_t lin, size_t m,
                size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, typename F::Word *terms, hipStream_t st) {
    const size_t npolys = glwe_dim + 1, chunk = pack_chunk<F>(pl, lin, levels);
    const size_t row = F::key_bytes(pl, levels * npolys);   // one mask word's key rows
    hipError_t e = F::launch_pack_body(pl, out, in, glwe_dim, lin, m, batch, ew_grid(batch * npolys * pl->n), st);
    if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_pack_body_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
    typename F::KeyStore ks;
    for (size_t i0 = 0; i0 < lin; i0 += chunk) {
        const size_t nw = std::min(chunk, lin - i0);
        e = F::launch_pack_decompose(pl, terms, in, base_log, levels, lin, m, i0, nw, batch, st);
        if (e != hipSuccess) return fail(CNTT_EDEVICE, "%s_pack_decompose_kernel launch failed: %s", F::NAME, hipGetErrorString(e));
        if (int rc = F::ext_product(pl, out, terms, F::key_at(pl, pksk, i0 * row, ks), nw * levels, npolys, batch, true, st)) return rc;
    }
    return CNTT_OK;
}

// The family's refusals keep the places they have in each header's list: F::pack_check_levels before the counts, F::pack_check_sizes
// (what must hold before a byte count is formed) after them, F::pack_key_overlaps among the overlap checks.
template <class F>
int pack_keyswitch(const typename F::Plan *pl, typename F::Word *glwe_out, const typename F::Word *lwe_in, typename F::Key pksk_ntt,
                   size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace,
                   size_t workspace_bytes, cntt_mem_t where, hipStream_t st) {
    using W = typename F::Word;
    if (!pl) return fail(CNTT_EINVAL, "plan is NULL");
    if (int rc = gadget_check<F>(pl, base_log, levels, CNTT_SRC_PLAIN, nullptr)) return rc;
    if (int rc = F::pack_check_levels(pl, levels)) return rc;
    if (lwe_count == 0 || lwe_count > pl->n)
        return fail(CNTT_EINVAL, "lwe_count = %zu is not in 1 .. ntt_size = %zu", lwe_count, pl->n);
    if (glwe_dim + 1 >= ((size_t)1 << 32)) return fail(CNTT_EINVAL, "glwe_dim too large");
    if (int rc = F::pack_check_sizes(pl, lwe_dim_in, lwe_count, glwe_dim, levels, batch)) return rc;
    if (batch == 0) return CNTT_OK;
    if (!glwe_out) return fail(CNTT_EINVAL, "glwe_out is NULL");
    if (!lwe_in) return fail(CNTT_EINVAL, "lwe_in is NULL");
    if (lwe_dim_in)
        if (int rc = F::key_check(pl, pksk_ntt, "pksk_ntt")) return rc;
    const size_t n = pl->n, w = F::word(pl), ob = batch * (glwe_dim + 1) * n * w, ib = batch * lwe_count * (lwe_dim_in + 1) * w;
    const size_t kb = F::key_bytes(pl, lwe_dim_in * levels * (glwe_dim + 1)), need = pack_workspace_bytes<F>(pl, lwe_dim_in, levels, batch);
    if (ranges_overlap(glwe_out, ob, lwe_in, ib)) return fail(CNTT_EINVAL, "glwe_out overlaps lwe_in");
    if (F::pack_key_overlaps(glwe_out, ob, pksk_ntt, kb)) return fail(CNTT_EINVAL, "glwe_out overlaps pksk_ntt");
    if (workspace) {
        if (int rc = check_workspace(workspace, workspace_bytes, need)) return rc;
        if (ranges_overlap(glwe_out, ob, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "glwe_out overlaps workspace");
        if (ranges_overlap(lwe_in, ib, workspace, workspace_bytes)) return fail(CNTT_EINVAL, "lwe_in overlaps workspace");
    }
    Staging s(where, st);
    typename F::KeyStore ks;
    const typename F::Key dkey = lwe_dim_in ? F::key_in(pl, s, pksk_ntt, kb, ks) : typename F::Key{};
    const W *din = (const W *)s.in(lwe_in, ib);
    W *dout = (W *)s.out(glwe_out, ob), *dterms = (W *)s.workspace(workspace, need, lwe_dim_in != 0);   // one block for the whole call
    if (int rc = s.status()) return rc;
    if (int rc = pack_device<F>(pl, dout, din, dkey, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, dterms, st)) return rc;
    return s.finish();
}

#pragma GCC visibility pop
