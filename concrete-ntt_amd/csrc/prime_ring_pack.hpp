// Ring packing of LWE ciphertexts through automorphisms on the prime plans (include/cntt_prime_ring_pack.h), two kernels on the walk of
// prime_automorphism.hpp:
//     prime_glwe_embed_kernel   glwe[q][0] = lwe[q n], glwe[q][i] = -lwe[q n + n - i] (q < k), glwe[k] = (lwe[k n], 0, ..., 0): the
//                               inverse of sample extraction at index 0
//     prime_ring_merge_kernel   the hot one: one tree node of PackLWEs.  Per output ciphertext ONE pass over the two sources E and O that
//                               writes the prefilled output  a = E + X^shift O  (body: + sigma_t(d))  and the k * levels negated digit
//                               polynomials of sigma_t(d), d = E - X^shift O.  a, d, the rotation and the permutation exist in registers
//                               only.
// The external product after the second is host code (host_prime_ring_pack.inc) over external_product_device.  The kernels are
// instantiated in prime_ring_pack.hip; host_prime.hip sees the launchers only.
//
// The walk is that of prime_automorphism_gadget_kernel: one 256-thread workgroup per output polynomial, grid-stride; a thread owns 16
// bytes of consecutive destination coefficients and every store is a coalesced 16-byte one.  Destination coefficient j needs four source
// words: E[j] and O[j - shift] for a, E[u] and O[u - shift] with u = j tinv mod 2n for sigma_t(d) -- indices mod n, signs from bit n.
//
// LDS (the switch of prime_automorphism.hpp).  With LDS = true the workgroup stages polynomial q of BOTH sources into LDS first -- possible
// while 2 n sizeof(T) <= 64 KiB (AUTOM_LDS_BYTES) -- so that global memory sees each source word once, and gathers from there; with
// LDS = false the same code gathers from global memory, which is what larger polynomials always take.  The rotated reads are
// consecutive words from an unaligned start and the permuted ones are NV tinv words apart per lane, the 2-way to 4-way bank conflict
// prime_automorphism.hpp describes; neither form is conflict-free.
//
// The two source forms (LEAF).  false: E and O are GLWE ciphertexts of k + 1 polynomials; output ciphertext c = g h + j (j < h) takes
// ciphertext g gs + j of `even` and of `odd` (one tree stage of a batch: gs = 2 h and odd = even + h ciphertexts; the public merge:
// h = gs = 1).  true: E and O are LWE rows of k n + 1 words, read through the embed rule above, so the first tree stage never writes
// the embedded ciphertexts; a row starts at a multiple of k n + 1 words, which is not 16-byte aligned in general, so the staging loads
// are one word each there.
//
// The digits are those of prime_automorphism_gadget_kernel (PrimePackConst, prime_pack.hpp), restated here word for word: y = x' + off,
// the bit `neg`, a shift per level, and the two selects that store -d mod p.  Words >= p are not reduced; no address depends on a
// data word.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "prime_automorphism.hpp"

namespace cntt {

// Workgroups of the two kernels for `polys` output polynomials of 2^logn words of word_bytes: the rule of prime_automorphism_grid with the
// LDS footprint of the merge (two staged polynomials): one per polynomial up to 8 per CU, fewer where 160 KiB of LDS hold fewer pairs, a
// grid-stride walk beyond.  An ASSUMPTION about what fills the chip, not a measured optimum.  cntt_prime_ring_pack_grid exports it.
inline unsigned prime_ring_pack_grid(size_t polys, int logn, size_t word_bytes) {
    const size_t bytes = (2 * word_bytes) << logn;
    size_t per_cu = 8;
    if (bytes <= AUTOM_LDS_BYTES && bytes > 0) per_cu = std::min<size_t>(8, std::max<size_t>(1, ((size_t)160 << 10) / bytes));
    const size_t cap = per_cu * AUTOM_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

// coefficient i of polynomial q of the embedding of the LWE row `row` (k n + 1 words)
template <class T> __device__ __forceinline__ T ring_leaf_word(const T *__restrict__ row, uint32_t q, uint32_t i, uint32_t logn, uint32_t k, T p) {
    const size_t base = (size_t)q << logn;
    if (q == k) return i == 0 ? row[base] : (T)0;
    return i == 0 ? row[base] : prime_neg_if<T>(row[base + (1u << logn) - i], true, p);
}

// x + y, x - y mod p for canonical words (the sum of two words may pass the word)
template <class T> __device__ __forceinline__ T ring_add(T x, T y, T p) {
    const T s = (T)(x + y);
    return s < x || s >= p ? (T)(s - p) : s;
}
template <class T> __device__ __forceinline__ T ring_sub(T x, T y, T p) { return (T)(x - y + (x < y ? p : (T)0)); }

// lwe: batch rows of k n + 1 words; glwe: batch x (k + 1) polynomials
template <class T>
__global__ __launch_bounds__(256) void prime_glwe_embed_kernel(T *__restrict__ glwe, const T *__restrict__ lwe, T p, uint32_t logn, uint32_t k,
                                                               size_t batch) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t nvec = 1u << (logn - LOGV);
    const size_t npoly_total = batch * ((size_t)k + 1), row_words = ((size_t)k << logn) + 1;
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t b = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - b * (k + 1u));
        const T *row = lwe + b * row_words;
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            union {
                T w[NV];
                V v;
            } d;
#pragma unroll
            for (int c = 0; c < NV; ++c) d.w[c] = ring_leaf_word<T>(row, q, j0 + (uint32_t)c, logn, k, p);
            *reinterpret_cast<V *>(glwe + (i << logn) + j0) = d.v;
        }
    }
}

// (X^shift f)[i] for f read through `at`
template <class T, class F> __device__ __forceinline__ T ring_rot(F at, uint32_t i, uint32_t shift, uint32_t n, T p) {
    const uint32_t r = (i - shift) & (2u * n - 1u);
    return prime_neg_if<T>(at(r & (n - 1u)), (r & n) != 0, p);
}

// terms: nct x k * levels polynomials; out: nct x (k + 1) polynomials; even, odd: the sources in the form LEAF says (above); nct = the
// number of output ciphertexts, a multiple of h.  Polynomial (c, q):
//   q < k   out[c][q] = a[q],  terms[c][q levels + l - 1] = -d_l(sigma_t(d[q])) mod p
//   q = k   out[c][k] = a[k] + sigma_t(d[k]) mod p
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once.
template <class T, bool STREAM, bool LDS, bool LEAF>
__global__ __launch_bounds__(256) void prime_ring_merge_kernel(T *__restrict__ terms, T *__restrict__ out, const T *__restrict__ even,
                                                               const T *__restrict__ odd, const PrimePackConst<T> G, uint32_t tinv, uint32_t shift,
                                                               uint32_t logn, uint32_t k, size_t h, size_t gs, size_t nct) {
    using S = typename std::make_signed<T>::type;
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char ring_lds[];
    T *lds_e = reinterpret_cast<T *>(ring_lds), *lds_o = lds_e + ((size_t)1 << logn);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - LOGV);
    const size_t npoly_total = nct * ((size_t)k + 1);
    const size_t src_words = LEAF ? ((size_t)k << logn) + 1 : ((size_t)k + 1) << logn;   // one source ciphertext
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t c = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - c * (k + 1u));
        const size_t src = ((c / h) * gs + c % h) * src_words;
        const T *ce = even + src, *co = odd + src;   // the source ciphertexts; their polynomial q when not LEAF
        if constexpr (!LEAF) {
            ce += (size_t)q << logn;
            co += (size_t)q << logn;
        }
        auto ge = [&](uint32_t j) -> T {
            if constexpr (LEAF) return ring_leaf_word<T>(ce, q, j, logn, k, G.p);
            else return ce[j];
        };
        auto go = [&](uint32_t j) -> T {
            if constexpr (LEAF) return ring_leaf_word<T>(co, q, j, logn, k, G.p);
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
        auto e_at = [&](uint32_t j) -> T {
            if constexpr (LDS) return lds_e[j];
            else return ge(j);
        };
        auto o_at = [&](uint32_t j) -> T {
            if constexpr (LDS) return lds_o[j];
            else return go(j);
        };
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            T x[NV];
            union {
                T w[NV];
                V v;
            } d, a;
#pragma unroll
            for (int c2 = 0; c2 < NV; ++c2) {
                const uint32_t j = j0 + (uint32_t)c2, u = (j * tinv) & m2n, ui = u & (n - 1u);
                a.w[c2] = ring_add<T>(e_at(j), ring_rot<T>(o_at, j, shift, n, G.p), G.p);
                x[c2] = prime_neg_if<T>(ring_sub<T>(e_at(ui), ring_rot<T>(o_at, ui, shift, n, G.p), G.p), (u & n) != 0, G.p);
            }
            V *o = reinterpret_cast<V *>(out + (i << logn) + j0);
            if (q == k) {   // (the same for the whole workgroup) the body: a + sigma_t(d)
#pragma unroll
                for (int c2 = 0; c2 < NV; ++c2) d.w[c2] = ring_add<T>(a.w[c2], x[c2], G.p);
                *o = d.v;
                continue;
            }
            *o = a.v;
            T y[NV];
            bool neg[NV];
            T *dst = terms + (((c * k + q) * G.levels) << logn) + j0;
#pragma unroll
            for (int c2 = 0; c2 < NV; ++c2) {
                const bool hi = x[c2] >= (T)(G.p - x[c2]);
                y[c2] = (T)(x[c2] + G.off - (hi ? G.p : (T)0));
                neg[c2] = hi && (S)y[c2] < 0;
                // -d_1: |d_1| of a negative top digit as it stands, p - d_1 of a positive one
                const T d1 = neg[c2] ? (T)(0 - (T)((S)y[c2] >> G.sh1)) : (T)(y[c2] >> G.sh1);
                d.w[c2] = neg[c2] || d1 == 0 ? d1 : (T)(G.p - d1);
            }
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
            else *reinterpret_cast<V *>(dst) = d.v;
            uint32_t sh = G.sh1;
            for (uint32_t l = 1; l < G.levels; ++l) {
                sh -= G.base_log;
                dst += n;
#pragma unroll
                for (int c2 = 0; c2 < NV; ++c2) {
                    const T f = (T)((y[c2] >> sh) & G.mask);   // the digit + B / 2
                    d.w[c2] = f <= G.half ? (T)(G.half - f) : (T)(G.p - f + G.half);
                }
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launchers (prime_ring_pack.hip), T = uint32_t / uint64_t.  lds: stage through LDS where the two polynomials fit (the caller's wish; the
// launcher falls back to the global gather above AUTOM_LDS_BYTES); stream: the STREAM_BYTES policy decided by the caller
template <class T> hipError_t launch_prime_glwe_embed(T *glwe, const T *lwe, T p, int logn, size_t glwe_dim, size_t batch, hipStream_t st);
template <class T>
hipError_t launch_prime_ring_merge(T *terms, T *out, const T *even, const T *odd, bool leaf, const PrimePackConst<T> &G, uint32_t t, uint32_t shift,
                                   int logn, size_t glwe_dim, size_t h, size_t gs, size_t nct, bool stream, bool lds, hipStream_t st);

}  // namespace cntt
