// The circuit bootstrap of the prime plans (include/cntt_prime_cbs.h): LWE encryptions of bits in, GGSW selectors out.  Four kernels
// around the unchanged blind rotation (blind_rotate_device of pbs_host.hpp), E = batch * cbs_levels bootstrap elements, element
// e = b * cbs_levels + (l - 1):
//     prime_cbs_setup_kernel     one launch: the rot_t rows of the E elements (the modulus switch of lwe_in[b] with Q4 added to the body,
//                                replicated over the levels) and the E per-element tables, trivial GLWE ciphertexts whose body is the
//                                constant p - H_l
//     prime_cbs_extract_kernel   reads the E accumulators once: sample extraction at index 0 and + H_l on the body in registers, then the
//                                R = (k n + 1) ks_levels SIGNED digits of every word as int32 -- plain integers, not residues.  The LWE
//                                ciphertexts u are never stored.
//     prime_cbs_ks_kernel        the hot one, the functional keyswitch as a product: per key q an E x R matrix of int32 digits times an
//                                R x (k + 1) n matrix of NTT-domain key words, cut into slabs of rows; every slab sum leaves reduced mod p
//     prime_cbs_sum_kernel       adds the slabs mod p, negates, stores in the selector layout
// The kernels are instantiated in prime_cbs.hip; host_prime.hip sees the launchers only.
//
// The digits are those of prime_gadget_kernel (prime_pbs.hpp) in the form of PrimePackConst (prime_pack.hpp), restated here: y = x' + off,
// the bit `neg`, a shift per level, the top digit unmasked -- but kept SIGNED: d_1 = the arithmetic (neg) or logical shift of y, the lower
// levels ((y >> sh) & mask) - B / 2.  ks_base_log <= 31, so |d| <= 2^30 fits an int32, the top digit's +-B / 2 included.
//
// The product.  A 256-thread workgroup owns CBS_ET = 8 elements x 256 vectors of 16 bytes of consecutive key columns x one slab of rows
// of one key.  A thread keeps one wide accumulator per (element, slot) in registers and reads every key word of its columns ONCE for the
// eight elements.  The digit is the same for the whole workgroup: the tile's digits are parked in LDS, CBS_CH rows at a time, as
// [row][element], and every lane reads the same 32 bytes (a broadcast, no bank conflict); __builtin_amdgcn_readfirstlane then moves the
// digit to a scalar register, so the sign test is a scalar branch and the multiplier a scalar operand.
// Lazy accumulation: no reduction inside a slab.
//   64-bit words: |d| <= 2^30, key word < 2^64, at most 2^32 - 1 rows: |sum| < 2^126, held by a two's-complement 128-bit accumulator
//                 (the product |d| w < 2^94 is two v_mad_u64_u32).
//   32-bit words: |d| <= 2^(ks_base_log - 1) <= 2^30, key word < 2^W <= 2^32: |sum| <= R 2^(W + ks_base_log - 1) < 2^32 2^62 = 2^94, held
//                 by a two's-complement 96-bit accumulator (64 low bits + 32 high bits); a 64-bit one would hold two rows at the edge.
// Once per slab the accumulator is reduced mod p bit by bit from the top (r = 2 r + bit, one conditional subtraction: exact for every
// prime, W = 64 included, where the carry out of the shift is the 65th bit); `bits` bounds the magnitude: W + ks_base_log - 1 + the bit
// length of the slab's rows.  A negative sum gives p - r.  Slabs exist because at k = 1, n = 1024 a key has 4096 columns = 8 workgroups
// per E-tile: too few to pull HBM bandwidth.  The sums are exact mod p, so the result does not depend on the slab count.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "prime_pack.hpp"
#include "prime_pbs.hpp"

namespace cntt {

constexpr unsigned CBS_CUS = 256;    // CUs of the part the grid rule is written for
constexpr unsigned CBS_ET = 8;       // elements of one tile of the product
constexpr unsigned CBS_CH = 128;     // rows of digits parked in LDS at a time
constexpr unsigned CBS_SLAB_MIN = 64;   // a slab has at least this many rows (the last one may have fewer)

// Workgroups of prime_cbs_ks_kernel for `items` work items (key x E-tile x column block x slab): one per item up to 8 per CU, a
// grid-stride walk beyond.  An ASSUMPTION carried over from prime_cmux_grid, not a measured optimum.  cntt_prime_cbs_grid exports it.
inline unsigned prime_cbs_grid(size_t items, int /*logn*/, size_t /*word_bytes*/) {
    const size_t cap = (size_t)8 * CBS_CUS;
    return (unsigned)(items < 1 ? 1 : items > cap ? cap : items);
}

// the shape of the product: column blocks per key, E-tiles, rows per slab, slabs (the header states the rule)
struct CbsShape {
    size_t cols, tiles, rows, slabs;
    __host__ __device__ size_t items(size_t k) const { return (k + 1) * cols * tiles * slabs; }
};
inline CbsShape prime_cbs_shape(size_t n, size_t word_bytes, size_t k, size_t r, size_t e) {
    const size_t cap = (size_t)8 * CBS_CUS, per_block = 256 * (16 / word_bytes);
    CbsShape s;
    s.cols = ((k + 1) * n + per_block - 1) / per_block;
    s.tiles = (e + CBS_ET - 1) / CBS_ET;
    const size_t base = (k + 1) * s.cols * (s.tiles ? s.tiles : 1);
    size_t s0 = cap / base;                                              // slabs that still fit one trip of the grid
    const size_t most = (r + CBS_SLAB_MIN - 1) / CBS_SLAB_MIN;
    s0 = s0 > most ? most : s0;
    s0 = s0 < 1 ? 1 : s0;
    s.rows = (r + s0 - 1) / s0;
    s.slabs = (r + s.rows - 1) / s.rows;
    return s;
}

// constants of the set-up kernel
template <class T> struct PrimeCbsSetup {
    T p, q4, half_inv;            // modulus, floor((p + 2) / 4), 2^-1 mod p = (p + 1) / 2
    uint32_t logn, k, wbits, cbs_base_log, cbs_levels;
};

// H_l = 2^(W - cbs_base_log l) 2^-1 mod p: 2^(sh - 1) for sh >= 1, (p + 1) / 2 for sh = 0
template <class T> __host__ __device__ __forceinline__ T prime_cbs_h(uint32_t wbits, uint32_t base_log, uint32_t l, T half_inv) {
    const uint32_t sh = wbits - base_log * l;
    return sh ? (T)((T)1 << (sh - 1)) : half_inv;
}

// rot_t: (L + 1) x E uint32, rot_t[i E + e] = ms(lwe'[b][i]), the body row negated mod 2n;  table: E x (k + 1) polynomials, masks zero, the
// body polynomial the constant p - H_l.  One grid-stride walk over the (L + 1) E exponents and then the table's 16-byte vectors.
template <class T>
__global__ __launch_bounds__(256) void prime_cbs_setup_kernel(uint32_t *__restrict__ rot_t, T *__restrict__ table, const T *__restrict__ lwe,
                                                              const PrimeCbsSetup<T> C, size_t lwe_dim, size_t elements) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const size_t nrot = (lwe_dim + 1) * elements, nvec = (elements * (C.k + 1u)) << (C.logn - LOGV);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t mask = (2u << C.logn) - 1u;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nrot + nvec; t += stride) {
        if (t < nrot) {
            const size_t i = t / elements, e = t - i * elements, b = e / C.cbs_levels;
            T x = lwe[b * (lwe_dim + 1) + i];
            if (i == lwe_dim) x = (T)(x + C.q4 - (x >= (T)(C.p - C.q4) ? C.p : (T)0));
            uint32_t m = prime_ms<T>(x, C.p, C.logn + 2u, mask);
            if (i == lwe_dim) m = (0u - m) & mask;
            rot_t[t] = m;
        } else {
            const size_t v = t - nrot, poly = v >> (C.logn - LOGV), e = poly / (C.k + 1u);
            const uint32_t q = (uint32_t)(poly - e * (C.k + 1u)), l = (uint32_t)(e % C.cbs_levels) + 1u;
            const T c = q == C.k ? (T)(C.p - prime_cbs_h<T>(C.wbits, C.cbs_base_log, l, C.half_inv)) : (T)0;
            union {
                T w[NV];
                V v;
            } d;
#pragma unroll
            for (int j = 0; j < NV; ++j) d.w[j] = c;
            reinterpret_cast<V *>(table)[v] = d.v;
        }
    }
}

// digits[e R + i Lk + j - 1] = d_j(u[e][i]) for i <= Lin = k n, where u[e] is the sample extraction at index 0 of acc[e] with H_l added
// to the body:  u[q n + t] = acc[q][0] (t = 0), -acc[q][n - t] mod p (t > 0);  u[k n] = acc[k][0] + H_l mod p.  One thread per word of u.
template <class T>
__global__ __launch_bounds__(256) void prime_cbs_extract_kernel(int32_t *__restrict__ digits, const T *__restrict__ acc, const PrimePackConst<T> G,
                                                                const PrimeCbsSetup<T> C, size_t elements) {
    using S = typename std::make_signed<T>::type;
    const size_t n = (size_t)1 << C.logn, lin = (size_t)C.k << C.logn, row = lin + 1, total = elements * row;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t e = t / row, i = t - e * row;
        const T *g = acc + ((e * (C.k + 1u)) << C.logn);
        T x;
        if (i == lin) {
            const T h = prime_cbs_h<T>(C.wbits, C.cbs_base_log, (uint32_t)(e % C.cbs_levels) + 1u, C.half_inv);
            x = g[lin];
            x = (T)(x + h - (x >= (T)(C.p - h) ? C.p : (T)0));
        } else {
            const size_t pos = i & (n - 1);
            x = pos ? prime_neg_if<T>(g[i - pos + (n - pos)], true, C.p) : g[i];
        }
        const bool hi = x >= (T)(G.p - x);
        const T y = (T)(x + G.off - (hi ? G.p : (T)0));
        const bool neg = hi && (S)y < 0;
        int32_t *dst = digits + (e * row + i) * G.levels;
        dst[0] = neg ? (int32_t)((S)y >> G.sh1) : (int32_t)(y >> G.sh1);   // d_1, unmasked: [-B / 2, B / 2]
        uint32_t sh = G.sh1;
        for (uint32_t l = 1; l < G.levels; ++l) {
            sh -= G.base_log;
            dst[l] = (int32_t)((y >> sh) & G.mask) - (int32_t)G.half;
        }
    }
}

// the wide accumulator of one (element, slot): two's complement, 128 bits on 64-bit words, 96 bits on 32-bit words (bounds at the top)
template <class T> struct CbsAcc;
template <> struct CbsAcc<uint64_t> {
    unsigned __int128 a;
    __device__ __forceinline__ void zero() { a = 0; }
    __device__ __forceinline__ void add(uint32_t m, uint64_t w, bool neg) {   // +- m w, m <= 2^30
        const uint64_t lo = (uint64_t)m * (uint32_t)w, hi = (uint64_t)m * (uint32_t)(w >> 32) + (lo >> 32);
        const unsigned __int128 pr = ((unsigned __int128)hi << 32) | (uint32_t)lo;
        a = neg ? a - pr : a + pr;
    }
    __device__ __forceinline__ __int128 value() const { return (__int128)a; }
};
template <> struct CbsAcc<uint32_t> {
    uint64_t lo;
    uint32_t hi;
    __device__ __forceinline__ void zero() { lo = 0, hi = 0; }
    __device__ __forceinline__ void add(uint32_t m, uint32_t w, bool neg) {   // +- m w < 2^62
        const uint64_t pr = (uint64_t)m * w;
        if (neg) {
            hi -= lo < pr;
            lo -= pr;
        } else {
            lo += pr;
            hi += lo < pr;
        }
    }
    __device__ __forceinline__ __int128 value() const { return (__int128)(((unsigned __int128)(uint64_t)(int64_t)(int32_t)hi << 64) | lo); }
};

// v mod p, canonical, for |v| < 2^bits (bits <= 127): bit by bit from the top, r < p throughout
template <class T> __device__ __forceinline__ T prime_cbs_reduce(__int128 v, T p, uint32_t bits) {
    const bool neg = v < 0;
    const unsigned __int128 m = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    T r = 0;
    for (uint32_t i = bits; i-- > 0;) {
        const bool carry = (r >> (sizeof(T) * 8 - 1)) != 0;
        r = (T)((T)(r << 1) | (T)((uint64_t)(m >> i) & 1u));
        if (carry || r >= p) r = (T)(r - p);
    }
    return neg && r != 0 ? (T)(p - r) : r;
}

// part[((s (k + 1) + q) E + e) C + col] = sum over the rows r of slab s of digits[e R + r] * key[(q R + r) C + col] mod p, C = (k + 1) n
// columns.  Work item = (slab, key, E-tile, column block), the column blocks of one (slab, key, tile) next to each other; grid-stride.
// Every bound is checked: rows past R and elements past E take the digit 0 and are not stored, vectors past C are neither read nor stored.
template <class T>
__global__ __launch_bounds__(256) void prime_cbs_ks_kernel(T *__restrict__ part, const int32_t *__restrict__ digits, const T *__restrict__ key, T p,
                                                           uint32_t logn, uint32_t k, size_t rows_total, size_t elements, CbsShape Z, uint32_t bits) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    __shared__ __attribute__((aligned(16))) int32_t dig[CBS_CH][CBS_ET];
    const size_t cvec = ((size_t)(k + 1u) << logn) >> LOGV;   // 16-byte vectors of one key row
    const size_t items = Z.items(k);
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const size_t cb = it % Z.cols, t1 = it / Z.cols, tile = t1 % Z.tiles, t2 = t1 / Z.tiles, q = t2 % (k + 1u), slab = t2 / (k + 1u);
        const size_t e0 = tile * CBS_ET, r0 = slab * Z.rows, r1 = r0 + Z.rows < rows_total ? r0 + Z.rows : rows_total;
        const size_t v = cb * 256 + threadIdx.x;
        const bool live = v < cvec;
        const V *kq = reinterpret_cast<const V *>(key) + q * rows_total * cvec + v;
        CbsAcc<T> acc[CBS_ET][NV];
#pragma unroll
        for (unsigned e = 0; e < CBS_ET; ++e)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[e][j].zero();
        for (size_t rc = r0; rc < r1; rc += CBS_CH) {
            const uint32_t nr = (uint32_t)(r1 - rc < CBS_CH ? r1 - rc : CBS_CH);
            __syncthreads();   // the chunk before has been read
            for (uint32_t x = threadIdx.x; x < CBS_CH * CBS_ET; x += 256u) {
                const uint32_t rr = x % CBS_CH, ee = x / CBS_CH;
                dig[rr][ee] = rr < nr && e0 + ee < elements ? digits[(e0 + ee) * rows_total + rc + rr] : 0;
            }
            __syncthreads();
            if (live) {
                for (uint32_t rr = 0; rr < nr; ++rr) {
                    union {
                        T w[NV];
                        V v;
                    } kw;
                    kw.v = kq[(rc + rr) * cvec];
#pragma unroll
                    for (unsigned e = 0; e < CBS_ET; ++e) {
                        const int32_t d = __builtin_amdgcn_readfirstlane(dig[rr][e]);
                        const uint32_t m = d < 0 ? 0u - (uint32_t)d : (uint32_t)d;
#pragma unroll
                        for (int j = 0; j < NV; ++j) acc[e][j].add(m, kw.w[j], d < 0);
                    }
                }
            }
        }
        if (live) {
#pragma unroll
            for (unsigned e = 0; e < CBS_ET; ++e) {
                if (e0 + e >= elements) break;
                union {
                    T w[NV];
                    V v;
                } o;
#pragma unroll
                for (int j = 0; j < NV; ++j) o.w[j] = prime_cbs_reduce<T>(acc[e][j].value(), p, bits);
                reinterpret_cast<V *>(part)[((slab * (k + 1u) + q) * elements + e0 + e) * cvec + v] = o.v;
            }
        }
    }
}

// out[b][(q Lc + l - 1) (k + 1) + o][c] = -sum_s part[s][q][e][o n + c] mod p, e = b Lc + l - 1: one thread per 16 bytes, grid-stride
template <class T>
__global__ __launch_bounds__(256) void prime_cbs_sum_kernel(T *__restrict__ out, const T *__restrict__ part, T p, uint32_t logn, uint32_t k,
                                                            uint32_t cbs_levels, size_t elements, size_t slabs) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const size_t cvec = ((size_t)(k + 1u) << logn) >> LOGV, per_slab = (k + 1u) * elements * cvec;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < per_slab; t += stride) {
        const size_t v = t % cvec, qe = t / cvec, e = qe % elements, q = qe / elements, b = e / cbs_levels, l1 = e - b * cbs_levels;
        union {
            T w[NV];
            V v;
        } s, a;
        s.v = reinterpret_cast<const V *>(part)[t];
        for (size_t i = 1; i < slabs; ++i) {
            a.v = reinterpret_cast<const V *>(part)[i * per_slab + t];
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const T x = (T)(s.w[j] + a.w[j]);
                s.w[j] = x < a.w[j] || x >= p ? (T)(x - p) : x;   // both below p: the sum wraps a word only when W = the word's bits
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) s.w[j] = s.w[j] ? (T)(p - s.w[j]) : (T)0;
        reinterpret_cast<V *>(out)[((b * (k + 1u) + q) * cbs_levels + l1) * cvec + v] = s.v;
    }
}

// launchers (prime_cbs.hip), T = uint32_t / uint64_t
template <class T>
hipError_t launch_prime_cbs_setup(uint32_t *rot_t, T *table, const T *lwe, const PrimeCbsSetup<T> &C, size_t lwe_dim, size_t elements, unsigned grid,
                                  hipStream_t st);
template <class T>
hipError_t launch_prime_cbs_extract(int32_t *digits, const T *acc, const PrimePackConst<T> &G, const PrimeCbsSetup<T> &C, size_t elements,
                                    unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_cbs_ks(T *part, const int32_t *digits, const T *key, T p, int logn, size_t glwe_dim, size_t rows, size_t elements,
                               const CbsShape &Z, unsigned bits, hipStream_t st);
template <class T>
hipError_t launch_prime_cbs_sum(T *out, const T *part, T p, int logn, size_t glwe_dim, unsigned cbs_levels, size_t elements, size_t slabs,
                                unsigned grid, hipStream_t st);

}  // namespace cntt
