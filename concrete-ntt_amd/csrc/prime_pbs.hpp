// The programmable bootstrap of the prime plans around the fused mul_accumulate chain (include/cntt_prime_pbs.h):
//     prime_gadget_kernel            rotation, CMux difference and signed gadget decomposition mod p; polys read once, `levels` term
//                                    polynomials written (the hot one: once per blind-rotation iteration over the whole accumulator)
//     prime_lwe_modswitch_kernel     LWE words -> exponents below 2n, round(x 2n / p), transposed so that every iteration's `rot` is contiguous
//     prime_pbs_init_kernel          acc[b][q] = X^(rot[b]) lut[q] mod p
//     prime_sample_extract_kernel    GLWE -> LWE of dimension k n
// The loop between them is host code (host_prime_pbs.inc) over prime_gadget_kernel and external_product_device (host_prime.hip), which
// this file does not touch.  The kernels are instantiated in prime_pbs.hip; host_prime_pbs.inc sees the launchers only.
//
// The digits without a carry chain.  T = the word type (TB bits), W = bit length of p, s = W - base_log levels, B = 2^base_log,
// x' = the balanced lift of x, K' = sum_{l >= 2} (B/2) B^(levels-l).  The integer
//     y = x' + 2^(s-1) + K' 2^s                                 [s = 0: no rounding term]
// holds digit l >= 2, offset by B/2, in its bits [W - base_log l, W - base_log (l-1)), and floor(y / 2^(W - base_log)) IS the top digit
// (it is not offset, so it is not masked either).  off = 2^(s-1) + K' 2^s < 2^(W-1) < p, hence -2^(W-1) < y < 2^W: one bit more than
// a word when W = TB.  The kernel keeps y mod 2^TB and the one bit `neg` (x > (p-1)/2 and x < p - off), which only the top digit needs:
// its value is (y mod 2^TB) >> (W - base_log), minus 2^(TB - (W - base_log)) when neg.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace cntt {

// constants of one decomposition call (PrimeGadgetConst::make in host_prime_pbs.inc)
template <class T> struct PrimeGadgetConst {
    T p, hp, off, thr;         // modulus, (p - 1) / 2, 2^(s-1) + K' 2^s, p - off
    T mask, half, pmh, topsub; // B - 1, B / 2, p - B / 2, 2^(TB - sh1) (0 when sh1 = 0)
    uint32_t sh1;              // W - base_log: position of the top digit
    uint32_t base_log, levels, npolys, rotated, cmux;
};

// -x mod p with 0 staying 0
template <class T> __device__ __forceinline__ T prime_neg_if(T x, bool n, T p) { return n && x != 0 ? (T)(p - x) : x; }

// coefficient `pos` of the source polynomial of f (n = 2^logn canonical words) for the exponent a < 2n (0 for the PLAIN mode), mod p
template <class T>
__device__ __forceinline__ T prime_source(const T *__restrict__ f, uint32_t pos, uint32_t a, uint32_t logn, bool cmux, T p) {
    const uint32_t n = 1u << logn, t = (pos - a) & (2 * n - 1);
    T x = prime_neg_if<T>(f[t & (n - 1)], (t & n) != 0, p);
    if (cmux) {
        const T y = f[pos];
        x = (T)(x - y + (x < y ? p : (T)0));
    }
    return x;
}

// terms[b][q * levels + l - 1] = digit l of source(polys[b][q], rot[b]), stored canonically mod p: one thread per 16 bytes of destination
// coefficients of one polynomial, grid-stride over batch * npolys polynomials; STREAM: the terms are larger than STREAM_BYTES and pass
// through once
template <class T, bool STREAM>
__global__ __launch_bounds__(256) void prime_gadget_kernel(T *__restrict__ terms, const T *__restrict__ polys, const uint32_t *__restrict__ rot,
                                                           const PrimeGadgetConst<T> G, uint32_t logn, size_t npoly_total) {
    using S = typename std::make_signed<T>::type;
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;   // 16 bytes of either word type
    const uint32_t lv = logn - LOGV;   // log2 vectors per polynomial (n >= 16)
    const size_t total = npoly_total << lv, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t q = i >> lv;   // b * npolys + polynomial
        const uint32_t pos0 = (uint32_t)(i & (((size_t)1 << lv) - 1)) << LOGV;
        const uint32_t a = G.rotated ? rot[q / G.npolys] & ((2u << logn) - 1u) : 0u;
        const T *f = polys + (q << logn);
        T y[NV];
        union {
            T w[NV];
            V v;
        } d;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const T x = prime_source<T>(f, pos0 + (uint32_t)k, a, logn, G.cmux != 0, G.p);
            const bool hi = x > G.hp;
            y[k] = (T)(x + G.off - (hi ? G.p : (T)0));
            // the top digit: signed, unmasked; canonical residue of a negative one is p + d
            const T t = (T)((y[k] >> G.sh1) - (hi && x < G.thr ? G.topsub : (T)0));
            d.w[k] = (T)(t + ((S)t < 0 ? G.p : (T)0));
        }
        T *dst = terms + ((q * G.levels) << logn) + pos0;
        if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
        else *reinterpret_cast<V *>(dst) = d.v;
        uint32_t sh = G.sh1;
        for (uint32_t l = 1; l < G.levels; ++l) {
            sh -= G.base_log;
            dst += (size_t)1 << logn;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const T e = (T)((y[k] >> sh) & G.mask);   // the digit + B / 2
                d.w[k] = e >= G.half ? (T)(e - G.half) : (T)(e + G.pmh);
            }
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
            else *reinterpret_cast<V *>(dst) = d.v;
        }
    }
}

constexpr int PRIME_PBS_TILE = 32;   // transpose tile: 32 x 32 exponents through LDS, 256 threads as 32 x 8

// round(x 2n / p) mod 2n, exact: `steps` = logn + 2 rounds of doubling with a conditional subtraction leave q = floor(x 4n / p)
// (r < p throughout for canonical x; the bit shifted out of r is the carry of the comparison), then (q + 1) >> 1.  p is odd: no ties.
template <class T> __device__ __forceinline__ uint32_t prime_ms(T x, T p, uint32_t steps, uint32_t mask) {
    T r = x;
    uint32_t q = 0;
    for (uint32_t i = 0; i < steps; ++i) {
        const bool carry = (r >> (sizeof(T) * 8 - 1)) != 0;
        r = (T)(r << 1);
        q <<= 1;
        if (carry || r >= p) {
            r = (T)(r - p);
            q |= 1u;
        }
    }
    return ((q + 1u) >> 1) & mask;
}

// rot_t[i * batch + b] = ms(lwe[b][i]) (i < L),  rot_t[L * batch + b] = 2n - ms(lwe[b][L]) mod 2n.  Rows of the tile are read along i (the
// LWE words of one element are contiguous) and written along b (row i of rot_t is contiguous): both sides coalesced.  Grid-stride over
// the tiles; every bound is checked per word.
template <class T>
__global__ __launch_bounds__(256) void prime_lwe_modswitch_kernel(uint32_t *__restrict__ rot_t, const T *__restrict__ lwe, T p, uint32_t logn,
                                                                  size_t lwe_dim, size_t batch) {
    __shared__ uint32_t tile[PRIME_PBS_TILE][PRIME_PBS_TILE + 1];
    const size_t row = lwe_dim + 1, ti = (row + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE, tb = (batch + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE,
                 tiles = ti * tb;
    const uint32_t tx = threadIdx.x & (PRIME_PBS_TILE - 1), ty = threadIdx.x / PRIME_PBS_TILE;   // ty < 8
    const uint32_t mask = (2u << logn) - 1u;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t i0 = (t % ti) * PRIME_PBS_TILE, b0 = (t / ti) * PRIME_PBS_TILE;
#pragma unroll
        for (uint32_t r = ty; r < PRIME_PBS_TILE; r += 8) {
            const size_t b = b0 + r, i = i0 + tx;
            if (b < batch && i < row) {
                uint32_t m = prime_ms<T>(lwe[b * row + i], p, logn + 2u, mask);
                if (i == lwe_dim) m = (0u - m) & mask;
                tile[r][tx] = m;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = ty; r < PRIME_PBS_TILE; r += 8) {
            const size_t i = i0 + r, b = b0 + tx;
            if (i < row && b < batch) rot_t[i * batch + b] = tile[tx][r];
        }
        __syncthreads();
    }
}

// acc[b][q] = X^(rot[b]) lut[q] (lut_stride == 0: shared by the batch) or X^(rot[b]) lut[b][q] (lut_stride = npolys): one thread per 16
// bytes of destination, grid-stride over batch * npolys polynomials; STREAM as prime_gadget_kernel
template <class T, bool STREAM>
__global__ __launch_bounds__(256) void prime_pbs_init_kernel(T *__restrict__ acc, const T *__restrict__ lut, const uint32_t *__restrict__ rot,
                                                             T p, uint32_t logn, uint32_t npolys, uint32_t lut_stride, size_t npoly_total) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t lv = logn - LOGV;
    const size_t total = npoly_total << lv, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t q = i >> lv, b = q / npolys, c = q - b * npolys;
        const uint32_t pos0 = (uint32_t)(i & (((size_t)1 << lv) - 1)) << LOGV;
        const uint32_t a = rot[b] & ((2u << logn) - 1u);
        const T *f = lut + ((b * lut_stride + c) << logn);
        union {
            T w[NV];
            V v;
        } d;
#pragma unroll
        for (int k = 0; k < NV; ++k) d.w[k] = prime_source<T>(f, pos0 + (uint32_t)k, a, logn, false, p);
        V *dst = reinterpret_cast<V *>(acc + (q << logn) + pos0);
        if constexpr (STREAM) __builtin_nontemporal_store(d.v, dst);
        else *dst = d.v;
    }
}

// lwe_out[b][q n + j] = glwe[b][q][h - j], negated mod p past the wrap (j > h) -- coefficient h of X^j glwe[b][q], the same gather -- and
// the body lwe_out[b][k n] = glwe[b][k][h].  One thread per output word (an element has k n + 1 of them: no 16-byte alignment to rely on).
template <class T>
__global__ __launch_bounds__(256) void prime_sample_extract_kernel(T *__restrict__ lwe_out, const T *__restrict__ glwe, T p, uint32_t logn,
                                                                   size_t glwe_dim, uint32_t h, size_t batch) {
    const size_t kn = glwe_dim << logn, row = kn + 1, total = batch * row, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / row, r = i - b * row;
        const T *g = glwe + ((b * (glwe_dim + 1)) << logn);
        if (r == kn) lwe_out[i] = g[kn + h];
        else lwe_out[i] = prime_source<T>(g + ((r >> logn) << logn), h, (uint32_t)(r & (((size_t)1 << logn) - 1)), logn, false, p);
    }
}

// launchers (prime_pbs.hip), T = uint32_t / uint64_t; grid from ew_grid, stream = the STREAM_BYTES policy decided by the caller
template <class T>
hipError_t launch_prime_gadget(T *terms, const T *polys, const uint32_t *rot, const PrimeGadgetConst<T> &G, int logn, size_t npoly_total,
                               bool stream, unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_lwe_modswitch(uint32_t *rot_t, const T *lwe, T p, int logn, size_t lwe_dim, size_t batch, unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_pbs_init(T *acc, const T *lut, const uint32_t *rot, T p, int logn, uint32_t npolys, bool per_element, size_t batch,
                                 bool stream, unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_sample_extract(T *lwe_out, const T *glwe, T p, int logn, size_t glwe_dim, uint32_t index, size_t batch, unsigned grid,
                                       hipStream_t st);

}  // namespace cntt
