// The ring automorphism X -> X^t of the prime plans (include/cntt_prime_automorphism.h), three kernels on one walk:
//     prime_automorphism_kernel          out[j] = +-in[j t^-1 mod 2n]: the coefficient-domain map, gather form
//     prime_automorphism_ntt_kernel      out[c] = in[c'] with 2 brev(c') + 1 = t (2 brev(c) + 1) mod 2n: the same map on NTT-domain words,
//                                        a pure permutation (slot c holds the evaluation at psi^(2 brev(c) + 1))
//     prime_automorphism_gadget_kernel   the hot one: per Galois keyswitch ONE pass over the input ciphertext that writes the k * levels
//                                        negated digit polynomials of the permuted mask polynomials and the prefilled output
// The external product after the third is host code (host_prime_automorphism.inc) over external_product_device.  The kernels are
// instantiated in prime_automorphism.hip; host_prime.hip sees the launchers only.
//
// The walk.  One 256-thread workgroup per polynomial, grid-stride over the polynomials; a thread owns 16 bytes of consecutive destination
// coefficients (NV = 2 / 4 words) and takes the vectors tid, tid + 256, ... of its polynomial, so every store is a coalesced 16-byte
// one.  The sources of one vector are NV gathers: j -> u = j tinv mod 2n advances by tinv per coefficient.
//
// LDS (the compile-time switch).  With LDS = true the workgroup first stages the whole source polynomial into LDS with coalesced
// 16-byte loads -- possible while n sizeof(T) <= 64 KiB (AUTOM_LDS_BYTES) -- and gathers from there; with LDS = false the same code
// gathers from global memory (the form of prime_source, prime_pbs.hpp), which is what larger polynomials always take.  Word k of the
// vectors of consecutive lanes is NV * tinv words apart: tinv is odd, so the lanes of a group fall on 64 / (2 NV) (8-byte words) or
// 32 / NV (4-byte words) distinct bank positions -- a 2-way to 4-way conflict, not a conflict-free read.  Which form is faster at
// n = 1024 ... 4096, where the polynomial is L2-resident either way, is a measurement: profiles/r19_prime_automorphism.txt.
//
// The digits are those of prime_pack.hpp (PrimePackConst): y = x' + off, the bit `neg`, a shift per level, and the two selects that
// store -d mod p.  A word x = 0 gives all-zero digits.  Words >= p are not reduced; no address depends on a data word.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "prime_pack.hpp"
#include "prime_pbs.hpp"

namespace cntt {

constexpr size_t AUTOM_LDS_BYTES = (size_t)64 << 10;   // the largest polynomial that is staged
constexpr unsigned AUTOM_CUS = 256;                      // CUs of the part the grid rule is written for
// Workgroups of the three kernels for `polys` polynomials of 2^logn words of word_bytes: one per polynomial up to what is resident at
// once -- 8 workgroups per CU (the 32-wave cap), fewer where the staged polynomial limits it (160 KiB of LDS per CU) -- and a grid-stride
// walk beyond.  An ASSUMPTION about what fills the chip, not a measured optimum.  cntt_prime_automorphism_grid exports the rule (tests
// derive a second trip from it); it does not depend on the LDS switch.
inline unsigned prime_automorphism_grid(size_t polys, int logn, size_t word_bytes) {
    const size_t bytes = word_bytes << logn;
    size_t per_cu = 8;
    if (bytes <= AUTOM_LDS_BYTES && bytes > 0) per_cu = std::min<size_t>(8, std::max<size_t>(1, ((size_t)160 << 10) / bytes));
    const size_t cap = per_cu * AUTOM_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

// stages polynomial f (n = 2^logn words, n * sizeof(T) <= AUTOM_LDS_BYTES) into LDS; the barrier before it protects the previous trip's reads
template <class T> __device__ __forceinline__ void autom_stage(T *lds, const T *__restrict__ f, uint32_t logn) {
    constexpr int LOGV = sizeof(T) == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t nvec = 1u << (logn - LOGV);
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < nvec; v += 256u) reinterpret_cast<V *>(lds)[v] = reinterpret_cast<const V *>(f)[v];
    __syncthreads();
}

// sigma_t(f)[j] for the running index u = j tinv mod 2n
template <class T> __device__ __forceinline__ T autom_word(const T *f, uint32_t u, uint32_t n, T p) {
    return prime_neg_if<T>(f[u & (n - 1u)], (u & n) != 0, p);
}

// out[q] = sigma_t(in[q]) (NTT = false, tinv = t^-1 mod 2n) or the slot permutation (NTT = true, tinv is t itself) for q < npoly_total
template <class T, bool STREAM, bool LDS, bool NTT>
__device__ __forceinline__ void autom_walk(T *__restrict__ out, const T *__restrict__ in, T p, uint32_t tinv, uint32_t logn, size_t npoly_total) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char autom_lds[];
    T *lds = reinterpret_cast<T *>(autom_lds);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - LOGV);
    for (size_t q = blockIdx.x; q < npoly_total; q += gridDim.x) {
        const T *f = in + (q << logn);
        if constexpr (LDS) autom_stage<T>(lds, f, logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            union {
                T w[NV];
                V v;
            } d;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const uint32_t j = j0 + (uint32_t)k;
                if constexpr (NTT) {
                    const uint32_t e = (tinv * (2u * (__brev(j) >> (32u - logn)) + 1u)) & m2n;   // odd
                    const uint32_t c = __brev(e >> 1) >> (32u - logn);
                    if constexpr (LDS) d.w[k] = lds[c];
                    else d.w[k] = f[c];
                } else {
                    const uint32_t u = (j * tinv) & m2n;
                    if constexpr (LDS) d.w[k] = autom_word<T>(lds, u, n, p);
                    else d.w[k] = autom_word<T>(f, u, n, p);
                }
            }
            V *dst = reinterpret_cast<V *>(out + (q << logn) + j0);
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, dst);
            else *dst = d.v;
        }
    }
}

template <class T, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void prime_automorphism_kernel(T *__restrict__ out, const T *__restrict__ in, T p, uint32_t tinv, uint32_t logn,
                                                                 size_t npoly_total) {
    autom_walk<T, STREAM, LDS, false>(out, in, p, tinv, logn, npoly_total);
}
template <class T, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void prime_automorphism_ntt_kernel(T *__restrict__ out, const T *__restrict__ in, uint32_t t, uint32_t logn,
                                                                     size_t npoly_total) {
    autom_walk<T, STREAM, LDS, true>(out, in, (T)0, t, logn, npoly_total);
}

// in, out: batch x (k + 1) polynomials; terms: batch x k * levels polynomials.  Polynomial (b, q):
//   q < k   terms[b][q levels + l - 1] = -d_l(sigma_t(in[b][q])) mod p,   out[b][q] = add ? in[b][q] : 0
//   q = k   out[b][k] = sigma_t(in[b][k]) (+ in[b][k] mod p when add)
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once (the output keeps the default policy: the external
// product reads it back next).
template <class T, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void prime_automorphism_gadget_kernel(T *__restrict__ terms, T *__restrict__ out, const T *__restrict__ in,
                                                                        const PrimePackConst<T> G, uint32_t tinv, uint32_t logn, uint32_t k,
                                                                        uint32_t add, size_t batch) {
    using S = typename std::make_signed<T>::type;
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char autom_lds[];
    T *lds = reinterpret_cast<T *>(autom_lds);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - LOGV);
    const size_t npoly_total = batch * ((size_t)k + 1);
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t b = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - b * (k + 1u));
        const T *f = in + (i << logn);
        if constexpr (LDS) autom_stage<T>(lds, f, logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            T x[NV];
            union {
                T w[NV];
                V v;
            } d, own;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const uint32_t u = ((j0 + (uint32_t)c) * tinv) & m2n;
                if constexpr (LDS) x[c] = autom_word<T>(lds, u, n, G.p);
                else x[c] = autom_word<T>(f, u, n, G.p);
            }
            if (add) {
                if constexpr (LDS) own.v = reinterpret_cast<const V *>(lds)[v];
                else own.v = reinterpret_cast<const V *>(f)[v];
            } else {
                own.v = V{0u, 0u, 0u, 0u};
            }
            V *o = reinterpret_cast<V *>(out + (i << logn) + j0);
            if (q == k) {   // (the same for the whole workgroup) the body: sigma_t(in) (+ in)
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const T s = (T)(x[c] + own.w[c]);
                    d.w[c] = s < x[c] || s >= G.p ? (T)(s - G.p) : s;
                }
                *o = d.v;
                continue;
            }
            *o = own.v;
            T y[NV];
            bool neg[NV];
            T *dst = terms + (((b * k + q) * G.levels) << logn) + j0;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const bool hi = x[c] >= (T)(G.p - x[c]);
                y[c] = (T)(x[c] + G.off - (hi ? G.p : (T)0));
                neg[c] = hi && (S)y[c] < 0;
                // -d_1: |d_1| of a negative top digit as it stands, p - d_1 of a positive one
                const T d1 = neg[c] ? (T)(0 - (T)((S)y[c] >> G.sh1)) : (T)(y[c] >> G.sh1);
                d.w[c] = neg[c] || d1 == 0 ? d1 : (T)(G.p - d1);
            }
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
            else *reinterpret_cast<V *>(dst) = d.v;
            uint32_t sh = G.sh1;
            for (uint32_t l = 1; l < G.levels; ++l) {
                sh -= G.base_log;
                dst += n;
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    const T e = (T)((y[c] >> sh) & G.mask);   // the digit + B / 2
                    d.w[c] = e <= G.half ? (T)(G.half - e) : (T)(G.p - e + G.half);
                }
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launchers (prime_automorphism.hip), T = uint32_t / uint64_t.  lds: stage through LDS where the polynomial fits (the caller's wish; the
// launcher falls back to the global gather above AUTOM_LDS_BYTES); stream: the STREAM_BYTES policy decided by the caller
template <class T>
hipError_t launch_prime_automorphism(T *out, const T *in, T p, uint32_t t, bool ntt, int logn, size_t npoly_total, bool stream, bool lds,
                                     hipStream_t st);
template <class T>
hipError_t launch_prime_automorphism_gadget(T *terms, T *out, const T *in, const PrimePackConst<T> &G, uint32_t t, int logn, size_t glwe_dim,
                                            bool add_input, size_t batch, bool stream, bool lds, hipStream_t st);

}  // namespace cntt
