// The multi-bit blind rotation of the prime plans (include/cntt_prime_multibit.h): one group of g mask words is absorbed by ONE external
// product against a key bundled from 2^g GGSW ciphertexts.  The bundle  sum_t X^(e_t) BSK[r][t]  differs per batch element and is never
// formed: in the NTT domain the monomial is a pointwise factor, so
//     out[b][o][c] = sum_{t < 2^g} M(e_t(b))[c] * ( sum_{j < nterms} terms_ntt[b][j][c] * key[t][j][o][c] )   mod p, canonical
// which is prime_multibit_accumulate_kernel, the only kernel of this file.  The transforms around it are the stand-alone ones and the digits
// those of prime_gadget_kernel (prime_pbs.hpp); the loop is host code (multibit_host.hpp; its step: host_prime_multibit.inc).  Instantiated in prime_multibit.hip.
//
// The monomial.  With psi the plan's primitive 2n-th root (the forward twiddle at bitrev(1)), fwd(X^e)[c] = psi^(e (2 bitrev_logn(c) + 1)):
//     M(e)[c] = +-psi^(m mod n),   m = e (2 bitrev(c) + 1) mod 2n,   minus when m >= n        (psi^n = -1)
// one gather from a table of n powers of psi.  2 bitrev(c) + 1 depends on c alone: a thread forms it once per word it owns.
//
// Exact products.  Every product is mont_mul (ntt_arith.hpp): exact for every odd p below 2^B when one factor is canonical, so unlike the
// mul_acc of the other external products this one equals the big-integer value for the strict-range primes too.  Placement of R = 2^B:
// a product of a term and a key word carries R^-1, the product of the inner sum and the monomial another one, and the table holds
// psi^m R^2 -- one mont_mul per (term, key word) and one per (pattern, word), no third one.  The table's words are never 0, so -x = p - x.
//
// Loop order: the pattern t outermost, one running sum per thread.  A thread owns one 16-byte vector of one (b, o) output polynomial, as
// in ext_accumulate_kernel (aux_kernels.hpp); it reads its nterms term vectors once per pattern (the same 16 bytes each time: first-level
// cache) and every key vector it needs once.  The alternative, j outermost with 2^g running sums, needs the pattern count at compile time
// to stay in registers; g is a runtime value here and there is one instance per word type, so it was not built and there is no A/B of
// the two orders.  The table is gathered from L2 (n words per plan); the LDS-staged variant was not built either.
// What the measurement says (profiles/r17_prime_multibit.txt): the kernel runs at 3 - 10 % of the HBM roofline on its terms and
// outputs, so it is bound by its 2^g nterms Montgomery products per word and by the L2 key reads, not by HBM or by the table
// gathers (2^g per word against 2^g nterms key loads).  The alternative the products invite on 64-bit words -- a lazy 128-bit sum of
// plain 64 x 64 products with one reduction per pattern, a third of the 32-bit multiplies of a mont_mul per term -- was weighed and not
// built: for p above 2^62 the sum of nterms products passes 128 bits, so it needs a third word or a fold every few terms, and the
// exactness for every prime is what the call is for.  It is the first thing to try next.
#pragma once
#include "ntt_arith.hpp"

namespace cntt {

constexpr unsigned PRIME_MULTIBIT_MAX_GROUPING = 4;
// The grid: 256 threads per 256 vectors of output, at most this many workgroups and a grid-stride loop beyond.  2048 is eight
// workgroups per CU of a 256-CU part, i.e. the 8 waves per SIMD the register count allows -- an ASSUMPTION about what fills the chip,
// not a measured optimum: no A/B against an uncapped grid (ew_grid, host_common.hpp) has been run.  cntt_prime_multibit_grid exports the
// rule (tests derive a second trip from it).
constexpr unsigned PRIME_MULTIBIT_MAX_BLOCKS = 2048;
inline unsigned prime_multibit_grid(size_t vectors) {
    const size_t blocks = (vectors + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > PRIME_MULTIBIT_MAX_BLOCKS ? PRIME_MULTIBIT_MAX_BLOCKS : blocks);
}

// rot_rows: g rows of `batch` exponents (taken mod 2n); key: 2^g * nterms * nout polynomials, pattern-major; tab[m] = psi^m 2^(2B) mod p,
// m < n.  n = 2^logn >= 16.  out may not overlap an input.
template <class T>
__global__ __launch_bounds__(256) void prime_multibit_accumulate_kernel(T *__restrict__ out, const T *__restrict__ terms,
                                                                        const uint32_t *__restrict__ rot_rows, const T *__restrict__ key,
                                                                        const T *__restrict__ tab, T p, T pinv_neg, uint32_t logn,
                                                                        uint32_t nterms, uint32_t nout, uint32_t g, size_t batch) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(NV))) T;
    const uint32_t lv = logn - LOGV;   // log2 vectors per polynomial
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, npat = 1u << g;
    const size_t total = (batch * nout) << lv, stride = (size_t)gridDim.x * blockDim.x;
    const size_t kstep = (size_t)nout << lv;   // vectors from key[t][j][o] to key[t][j + 1][o]
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i & (((size_t)1 << lv) - 1), bo = i >> lv;
        const size_t b = bo / nout, o = bo - b * nout;
        uint32_t a[PRIME_MULTIBIT_MAX_GROUPING], idx[NV];
#pragma unroll
        for (uint32_t q = 0; q < PRIME_MULTIBIT_MAX_GROUPING; ++q) a[q] = q < g ? rot_rows[(size_t)q * batch + b] & m2n : 0u;
#pragma unroll
        for (int k = 0; k < NV; ++k) idx[k] = 2u * (__brev(((uint32_t)v << LOGV) + (uint32_t)k) >> (32u - logn)) + 1u;
        const V *tv = reinterpret_cast<const V *>(terms) + ((b * nterms) << lv) + v;
        const V *kv = reinterpret_cast<const V *>(key) + (o << lv) + v;
        V acc;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = 0;
        for (uint32_t t = 0; t < npat; ++t) {
            uint32_t e = 0;
#pragma unroll
            for (uint32_t q = 0; q < PRIME_MULTIBIT_MAX_GROUPING; ++q) e += (t >> q) & 1u ? a[q] : 0u;
            V s;
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k] = 0;
            for (uint32_t j = 0; j < nterms; ++j) {
                const V x = tv[(size_t)j << lv];
                const V y = kv[(size_t)j * kstep];
#pragma unroll
                for (int k = 0; k < NV; ++k) s[k] = add_mod<T>(s[k], mont_mul(x[k], y[k], p, pinv_neg), p);
            }
            kv += (size_t)nterms * kstep;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const uint32_t m = (e * idx[k]) & m2n;   // e (2 bitrev(c) + 1) mod 2n: the wrap of 32 bits is a multiple of 2n
                const T w = tab[m & (n - 1u)];
                acc[k] = add_mod<T>(acc[k], mont_mul(s[k], m & n ? (T)(p - w) : w, p, pinv_neg), p);
            }
        }
        reinterpret_cast<V *>(out)[i] = acc;
    }
}

// launcher (prime_multibit.hip), T = uint32_t / uint64_t
template <class T>
hipError_t launch_prime_multibit_accumulate(T *out, const T *terms, const uint32_t *rot_rows, const T *key, const T *tab, T p, T pinv_neg,
                                            int logn, size_t nterms, size_t nout, unsigned grouping, size_t batch, hipStream_t st);

}  // namespace cntt
