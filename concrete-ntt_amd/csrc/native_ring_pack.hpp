// Ring packing of LWE ciphertexts through automorphisms on the native plans (include/cntt_ring_pack.h), two kernels on the walk of
// native_automorphism.hpp:
//     native_glwe_embed_kernel   glwe[q][0] = lwe[q n], glwe[q][i] = -lwe[q n + n - i] mod 2^w (q < k), glwe[k] = (lwe[k n], 0, ..., 0): the
//                                inverse of sample extraction at index 0; W = u32 / u64 / Word128
//     native_ring_merge_kernel   the hot one: one tree node of PackLWEs.  Per output ciphertext ONE pass over the two sources E and O that
//                                writes the prefilled output  a = E + X^shift O  (body: + sigma_t(d))  and the k * levels negated digit
//                                polynomials of sigma_t(d), d = E - X^shift O.  a, d, the rotation and the permutation exist in registers
//                                only.
// The external product after the second is host code (host_native_ring_pack.inc) over native_ext_device.  The kernels are instantiated in
// native_ring_pack.hip; host_native_ext.hip sees the launchers only.
//
// The walk is that of native_automorphism_gadget_kernel: one 256-thread workgroup per output polynomial, grid-stride; a thread owns 16
// bytes of consecutive destination coefficients (NV = 4 / 2 / 1 words) and every store is a coalesced 16-byte one.  Destination
// coefficient j needs four source words: E[j] and O[j - shift] for a, E[u] and O[u - shift] with u = j tinv mod 2n for sigma_t(d) --
// indices mod n, signs from bit log2 n.  No address depends on a data word.
//
// LDS (the switch of native_automorphism.hpp).  With LDS = true the workgroup stages polynomial q of BOTH sources into LDS first --
// possible while 2 n sizeof(W) <= 64 KiB (NATIVE_AUTOM_LDS_BYTES): Word128 up to n = 2048, u64 up to 4096, u32 up to 8192 -- so that
// global memory sees each source word once, and gathers from there; with LDS = false the same code gathers from global memory, which is
// what larger polynomials always take.  The rotated reads are consecutive words from an unaligned start and the permuted ones are
// NV tinv words apart per lane, the bank pattern native_automorphism.hpp derives; neither form is conflict-free below 128-bit words.
//
// The two source forms (LEAF).  false: E and O are GLWE ciphertexts of k + 1 polynomials; output ciphertext c = g h + j (j < h) takes
// ciphertext g gs + j of `even` and of `odd` (one tree stage of a batch: gs = 2 h and odd = even + h ciphertexts; the public merge:
// h = gs = 1).  true: E and O are LWE rows of k n + 1 words, read through the embed rule above, so the first tree stage never writes
// the embedded ciphertexts; a row starts at a multiple of k n + 1 words, which is 16-byte aligned for Word128 only, so the staging loads
// are one word each there.
//
// The digits are those of native_automorphism_gadget_kernel through the same WordOps and GadgetConst: y = sigma_t(d) + off, then per level
// the field (y >> sh) & mask; the kernel stores half - field, the NEGATED digit, as a wrapping w-bit word.
#pragma once
#include <algorithm>

#include "native_automorphism.hpp"

namespace cntt {

// Workgroups of the two kernels for `polys` output polynomials of 2^logn words of word_bytes: the rule of native_automorphism_grid with the
// LDS footprint of the merge (two staged polynomials): one per polynomial up to 8 per CU, fewer where 160 KiB of LDS hold fewer pairs, a
// grid-stride walk beyond.  An ASSUMPTION about what fills the chip, not a measured optimum and not an A/B.  cntt_native_ring_pack_grid
// exports it; it does not depend on the LDS switch.
inline unsigned native_ring_pack_grid(size_t polys, int logn, size_t word_bytes) {
    const size_t bytes = (2 * word_bytes) << logn;
    size_t per_cu = 8;
    if (bytes <= NATIVE_AUTOM_LDS_BYTES && bytes > 0) per_cu = std::min<size_t>(8, std::max<size_t>(1, ((size_t)160 << 10) / bytes));
    const size_t cap = per_cu * NATIVE_AUTOM_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

// coefficient i of polynomial q of the embedding of the LWE row `row` (k n + 1 words)
template <class W> __device__ __forceinline__ W native_ring_leaf_word(const W *__restrict__ row, uint32_t q, uint32_t i, uint32_t logn, uint32_t k) {
    const size_t base = (size_t)q << logn;
    if (q == k) return i == 0 ? row[base] : W{};
    return i == 0 ? row[base] : WordOps<W>::neg_if(row[base + (1u << logn) - i], true);
}

// lwe: batch rows of k n + 1 words; glwe: batch x (k + 1) polynomials
template <class W>
__global__ __launch_bounds__(256) void native_glwe_embed_kernel(W *__restrict__ glwe, const W *__restrict__ lwe, uint32_t logn, uint32_t k,
                                                                size_t batch) {
    constexpr int NV = NativeAutomVec<W>::NV, LOGV = NativeAutomVec<W>::LOGV;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t nvec = 1u << (logn - (uint32_t)LOGV);
    const size_t npoly_total = batch * ((size_t)k + 1), row_words = ((size_t)k << logn) + 1;
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t b = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - b * (k + 1u));
        const W *row = lwe + b * row_words;
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            union {
                W w[NV];
                V v;
            } d;
#pragma unroll
            for (int c = 0; c < NV; ++c) d.w[c] = native_ring_leaf_word<W>(row, q, j0 + (uint32_t)c, logn, k);
            *reinterpret_cast<V *>(glwe + (i << logn) + j0) = d.v;
        }
    }
}

// (X^shift f)[i] for f read through `at`
template <class W, class F> __device__ __forceinline__ W native_ring_rot(F at, uint32_t i, uint32_t shift, uint32_t n) {
    const uint32_t r = (i - shift) & (2u * n - 1u);
    return WordOps<W>::neg_if(at(r & (n - 1u)), (r & n) != 0);
}

// terms: nct x k * levels polynomials; out: nct x (k + 1) polynomials; even, odd: the sources in the form LEAF says (above); nct = the
// number of output ciphertexts, a multiple of h.  Polynomial (c, q):
//   q < k   out[c][q] = a[q],  terms[c][q levels + l - 1] = -d_l(sigma_t(d[q])) mod 2^w
//   q = k   out[c][k] = a[k] + sigma_t(d[k]) mod 2^w
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once (the output keeps the default policy: the external
// product reads it back next).  G: off, mask, half, base_log and levels are read; the source fields of GadgetConst are not.
template <class W, bool STREAM, bool LDS, bool LEAF>
__global__ __launch_bounds__(256) void native_ring_merge_kernel(W *__restrict__ terms, W *__restrict__ out, const W *__restrict__ even,
                                                                const W *__restrict__ odd, const GadgetConst<W> G, uint32_t tinv, uint32_t shift,
                                                                uint32_t logn, uint32_t k, size_t h, size_t gs, size_t nct) {
    using O = WordOps<W>;
    constexpr int NV = NativeAutomVec<W>::NV, LOGV = NativeAutomVec<W>::LOGV;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char native_ring_lds[];
    W *lds_e = reinterpret_cast<W *>(native_ring_lds), *lds_o = lds_e + ((size_t)1 << logn);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - (uint32_t)LOGV);
    const size_t npoly_total = nct * ((size_t)k + 1);
    const size_t src_words = LEAF ? ((size_t)k << logn) + 1 : ((size_t)k + 1) << logn;   // one source ciphertext
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t c = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - c * (k + 1u));
        const size_t src = ((c / h) * gs + c % h) * src_words;
        const W *ce = even + src, *co = odd + src;   // the source ciphertexts; their polynomial q when not LEAF
        if constexpr (!LEAF) {
            ce += (size_t)q << logn;
            co += (size_t)q << logn;
        }
        auto ge = [&](uint32_t j) -> W {
            if constexpr (LEAF) return native_ring_leaf_word<W>(ce, q, j, logn, k);
            else return ce[j];
        };
        auto go = [&](uint32_t j) -> W {
            if constexpr (LEAF) return native_ring_leaf_word<W>(co, q, j, logn, k);
            else return co[j];
        };
        if constexpr (LDS) {
            __syncthreads();   // the previous trip's reads
            if constexpr (LEAF) {
                for (uint32_t j = threadIdx.x; j < n; j += 256u) {
                    lds_e[j] = ge(j);
                    lds_o[j] = go(j);
                }
            } else {
                for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
                    reinterpret_cast<V *>(lds_e)[v] = reinterpret_cast<const V *>(ce)[v];
                    reinterpret_cast<V *>(lds_o)[v] = reinterpret_cast<const V *>(co)[v];
                }
            }
            __syncthreads();
        }
        auto e_at = [&](uint32_t j) -> W {
            if constexpr (LDS) return lds_e[j];
            else return ge(j);
        };
        auto o_at = [&](uint32_t j) -> W {
            if constexpr (LDS) return lds_o[j];
            else return go(j);
        };
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            W x[NV];
            union {
                W w[NV];
                V v;
            } d, a;
#pragma unroll
            for (int c2 = 0; c2 < NV; ++c2) {
                const uint32_t j = j0 + (uint32_t)c2, u = (j * tinv) & m2n, ui = u & (n - 1u);
                a.w[c2] = O::add(e_at(j), native_ring_rot<W>(o_at, j, shift, n));
                x[c2] = O::neg_if(O::sub(e_at(ui), native_ring_rot<W>(o_at, ui, shift, n)), (u & n) != 0);
            }
            V *o = reinterpret_cast<V *>(out + (i << logn) + j0);
            if (q == k) {   // (the same for the whole workgroup) the body: a + sigma_t(d)
#pragma unroll
                for (int c2 = 0; c2 < NV; ++c2) d.w[c2] = O::add(a.w[c2], x[c2]);
                *o = d.v;
                continue;
            }
            *o = a.v;
            W *dst = terms + (((c * k + q) * G.levels) << logn) + j0;
#pragma unroll
            for (int c2 = 0; c2 < NV; ++c2) x[c2] = O::add(x[c2], G.off);   // y
            uint32_t sh = (uint32_t)O::BITS;
            for (uint32_t l = 0; l < G.levels; ++l, dst += (size_t)1 << logn) {
                sh -= G.base_log;
#pragma unroll
                for (int c2 = 0; c2 < NV; ++c2) d.w[c2] = O::sub(G.half, O::band(O::shr(x[c2], sh), G.mask));   // -(field - half)
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launchers (native_ring_pack.hip).  word = 4 / 8 / 16 bytes; lds: stage through LDS where the two polynomials fit (the caller's wish; the
// launcher falls back to the global gather above NATIVE_AUTOM_LDS_BYTES); stream: the STREAM_BYTES policy decided by the caller; off = the
// word gadget_offset gives (host_native_ext.hip), in two halves
hipError_t launch_native_glwe_embed(int word, void *glwe, const void *lwe, int logn, size_t glwe_dim, size_t batch, hipStream_t st);
hipError_t launch_native_ring_merge(int word, void *terms, void *out, const void *even, const void *odd, bool leaf, uint64_t off_lo,
                                    uint64_t off_hi, unsigned base_log, unsigned levels, uint32_t t, uint32_t shift, int logn, size_t glwe_dim,
                                    size_t h, size_t gs, size_t nct, bool stream, bool lds, hipStream_t st);

}  // namespace cntt
