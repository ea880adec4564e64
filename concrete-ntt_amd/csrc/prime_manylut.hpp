// The many-LUT bootstrap of the prime plans and the circuit bootstrap with one rotation per input bit (include/cntt_prime_manylut.h).
// Three kernels around the unchanged blind rotation (blind_rotate_device of pbs_host.hpp) and the unchanged functional keyswitch
// (prime_cbs_ks_kernel, prime_cbs_sum_kernel of prime_cbs.hpp), t = log_lut_count, n' = n / 2^t:
//     prime_modswitch_manylut_kernel     the tiled transpose of prime_lwe_modswitch_kernel with the coarse rule ms_t(x) = ms_{n'}(x) << t;
//                                        the CBS variant adds Q4 to the body on the way and writes the one shared table of the circuit
//                                        bootstrap, v[m 2^t + h] = p - H_(h+1) for h < Lc and 0 above
//     prime_sample_extract_many_kernel   the extraction at the indices 0 .. count - 1 from ONE read of the accumulator (below)
//     prime_cbs_manylut_extract_kernel   the circuit bootstrap's extraction at the indices l - 1, + H_l on the body and the R Lc signed
//                                        int32 digits in the layout prime_cbs_ks_kernel reads; u is never stored
// The kernels are instantiated in prime_manylut.hip; host_prime.hip sees the launchers only.
//
// The window of prime_sample_extract_many_kernel.  Row h of an element takes, for the mask polynomial f and the destination word j,
// the source f[h - j] (negated past the wrap).  A thread owns the NV = 16 / sizeof(T) destination words j .. j + NV - 1 of a chunk of at
// most EXM_ROWS = 8 rows h0 .. h0 + 7: its sources f[h - j - i] are the EXM_ROWS + NV - 1 consecutive words from h0 - j - NV + 1 on,
// reversed.  j and h0 are multiples of NV, so the window is covered by 1 + EXM_ROWS / NV whole vectors of NV words starting at
// h0 - j - NV, and n is a multiple of NV, so a vector never straddles the wrap: one sign per vector.  Every load is 16 bytes, every
// store 16 bytes along the row.  A row of the output has k n + 1 words, so its vectors are aligned to the word only, and so is a
// caller's glwe: both sides use a vector type aligned to sizeof(T) (global memory takes such an access whole).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "prime_cbs.hpp"

namespace cntt {

constexpr uint32_t EXM_ROWS = 8;   // rows of one chunk of the extraction: the window stays in registers

// 16 bytes at the alignment of a word of `Bytes` bytes
typedef uint32_t ExmVec __attribute__((ext_vector_type(4)));
template <size_t Bytes> struct ExmWordAligned;
template <> struct ExmWordAligned<4> {
    typedef ExmVec type __attribute__((aligned(4)));
};
template <> struct ExmWordAligned<8> {
    typedef ExmVec type __attribute__((aligned(8)));
};

// rot_t[i batch + b] = ms_t(lwe[b][i]) (i < L), rot_t[L batch + b] = 2n - ms_t(lwe'[b][L]) mod 2n; CBS: lwe' = lwe + Q4 on the body, and
// the blocks past the tiles write the table's (k + 1) n words (16-byte vectors, 256 per block and trip).  Tiles as
// prime_lwe_modswitch_kernel: read along i, written along b, every bound checked per word.  C.cbs_levels <= 2^t (the launcher checks).
template <class T, bool CBS>
__global__ __launch_bounds__(256) void prime_modswitch_manylut_kernel(uint32_t *__restrict__ rot_t, T *__restrict__ table, const T *__restrict__ lwe,
                                                                      const PrimeCbsSetup<T> C, uint32_t log_lut, size_t lwe_dim, size_t batch) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    __shared__ uint32_t tile[PRIME_PBS_TILE][PRIME_PBS_TILE + 1];
    const size_t row = lwe_dim + 1, ti = (row + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE, tb = (batch + PRIME_PBS_TILE - 1) / PRIME_PBS_TILE,
                 tiles = ti * tb;
    const size_t nvec = CBS ? ((size_t)(C.k + 1u) << (C.logn - LOGV)) : 0, vblocks = (nvec + 255) / 256;
    const uint32_t tx = threadIdx.x & (PRIME_PBS_TILE - 1), ty = threadIdx.x / PRIME_PBS_TILE;   // ty < 8
    const uint32_t mask = (2u << C.logn) - 1u, steps = C.logn + 2u - log_lut, cmask = (2u << (C.logn - log_lut)) - 1u;
    for (size_t t = blockIdx.x; t < tiles + vblocks; t += gridDim.x) {
        if (t >= tiles) {   // CBS only: one block of table vectors (uniform per block: no barrier is skipped by part of a block)
            const size_t v = (t - tiles) * 256 + threadIdx.x;
            if (v < nvec) {
                const uint32_t q = (uint32_t)(v >> (C.logn - LOGV)), pos0 = (uint32_t)(v & (((size_t)1 << (C.logn - LOGV)) - 1)) << LOGV;
                union {
                    T w[NV];
                    V v;
                } d;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const uint32_t h = (pos0 + (uint32_t)j) & ((1u << log_lut) - 1u);
                    d.w[j] = q == C.k && h < C.cbs_levels ? (T)(C.p - prime_cbs_h<T>(C.wbits, C.cbs_base_log, h + 1u, C.half_inv)) : (T)0;
                }
                reinterpret_cast<V *>(table)[v] = d.v;
            }
            continue;
        }
        const size_t i0 = (t % ti) * PRIME_PBS_TILE, b0 = (t / ti) * PRIME_PBS_TILE;
#pragma unroll
        for (uint32_t r = ty; r < PRIME_PBS_TILE; r += 8) {
            const size_t b = b0 + r, i = i0 + tx;
            if (b < batch && i < row) {
                T x = lwe[b * row + i];
                if (CBS && i == lwe_dim) x = (T)(x + C.q4 - (x >= (T)(C.p - C.q4) ? C.p : (T)0));
                uint32_t m = prime_ms<T>(x, C.p, steps, cmask) << log_lut;
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

// lwe_out[b][h][q n + j] = glwe[b][q][h - j], negated mod p past the wrap (j > h), and lwe_out[b][h][k n] = glwe[b][k][h], for h < count.
// Work item = (element, mask polynomial, chunk of EXM_ROWS rows, vector of NV destination words), the vectors of one row next to each
// other; the batch * count body words are the tail of the same grid-stride walk.  Rows past count are neither formed nor stored, and
// the vectors of the window that only they would read are not loaded.  STREAM: the output is larger than STREAM_BYTES.
template <class T, bool STREAM>
__global__ __launch_bounds__(256) void prime_sample_extract_many_kernel(T *__restrict__ lwe_out, const T *__restrict__ glwe, T p, uint32_t logn,
                                                                        size_t glwe_dim, size_t count, size_t batch) {
    constexpr int NV = 16 / sizeof(T), LOGV = NV == 4 ? 2 : 1, NW = 1 + (int)EXM_ROWS / NV;   // vectors of the window
    using V4 = ExmVec;
    using V = typename ExmWordAligned<sizeof(T)>::type;
    const uint32_t lv = logn - LOGV, n = 1u << logn;
    const size_t kn = glwe_dim << logn, row = kn + 1, chunks = (count + EXM_ROWS - 1) / EXM_ROWS;
    const size_t nmask = (batch * glwe_dim * chunks) << lv, total = nmask + batch * count, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t >= nmask) {   // the body words
            const size_t e = t - nmask, b = e / count, h = e - b * count;
            lwe_out[e * row + kn] = glwe[((b * (glwe_dim + 1)) << logn) + kn + h];
            continue;
        }
        const uint32_t j = (uint32_t)(t & (((size_t)1 << lv) - 1)) << LOGV;
        const size_t t1 = t >> lv, c = t1 % chunks, t2 = t1 / chunks, q = t2 % glwe_dim, b = t2 / glwe_dim;
        const uint32_t h0 = (uint32_t)c * EXM_ROWS, rows = (uint32_t)(count - h0 < EXM_ROWS ? count - h0 : EXM_ROWS);
        const T *f = glwe + ((b * (glwe_dim + 1) + q) << logn);
        // win[r] = the source at h0 - j - NV + r with its sign; row h0 + hh takes win[hh - i + NV] for the destination word j + i
        T win[NW * NV];
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            if ((uint32_t)(m * NV) <= rows - 1u + (uint32_t)NV) {   // else only rows past `rows` would read it
                const uint32_t s = (h0 - j - (uint32_t)NV + (uint32_t)(m * NV)) & (2u * n - 1u);
                union {
                    T w[NV];
                    V4 v;
                } x;
                x.v = *reinterpret_cast<const V *>(f + (s & (n - 1u)));
#pragma unroll
                for (int i = 0; i < NV; ++i) win[m * NV + i] = prime_neg_if<T>(x.w[i], (s & n) != 0, p);
            }
        }
        T *dst = lwe_out + ((b * count + h0) * row + (q << logn) + j);
#pragma unroll
        for (uint32_t hh = 0; hh < EXM_ROWS; ++hh) {
            if (hh < rows) {
                union {
                    T w[NV];
                    V4 v;
                } d;
#pragma unroll
                for (int i = 0; i < NV; ++i) d.w[i] = win[(int)hh - i + NV];
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst + hh * row));
                else *reinterpret_cast<V *>(dst + hh * row) = d.v;
            }
        }
    }
}

// digits[(e R') + i Lk + j - 1] = d_j(u[b][l][i]), e = b Lc + l - 1, R' = (k n + 1) Lk, where u[b][l] is the extraction at the index l - 1
// of acc[b] with H_l added to the body.  One thread per word i of an element b: its sources for the Lc levels are the Lc consecutive
// words f[l - 1 - pos] (pos = i mod n; negated past the wrap), read in one walk.  Lc <= n / 2.  The digit rule is that of
// prime_cbs_extract_kernel, restated.
template <class T>
__global__ __launch_bounds__(256) void prime_cbs_manylut_extract_kernel(int32_t *__restrict__ digits, const T *__restrict__ acc,
                                                                        const PrimePackConst<T> G, const PrimeCbsSetup<T> C, size_t batch) {
    using S = typename std::make_signed<T>::type;
    const uint32_t n = 1u << C.logn;
    const size_t lin = (size_t)C.k << C.logn, row = lin + 1, total = batch * row;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t b = t / row, i = t - b * row;
        const T *g = acc + ((b * (C.k + 1u)) << C.logn);
        const uint32_t pos = (uint32_t)(i & (n - 1u));
        const T *f = g + (i - pos);   // the polynomial of word i; the body polynomial for i == lin (pos = 0)
        for (uint32_t l1 = 0; l1 < C.cbs_levels; ++l1) {
            T x;
            if (i == lin) {
                const T h = prime_cbs_h<T>(C.wbits, C.cbs_base_log, l1 + 1u, C.half_inv);
                x = f[l1];
                x = (T)(x + h - (x >= (T)(C.p - h) ? C.p : (T)0));
            } else {
                const uint32_t s = (l1 - pos) & (2u * n - 1u);
                x = prime_neg_if<T>(f[s & (n - 1u)], (s & n) != 0, C.p);
            }
            const bool hi = x >= (T)(G.p - x);
            const T y = (T)(x + G.off - (hi ? G.p : (T)0));
            const bool neg = hi && (S)y < 0;
            int32_t *dst = digits + ((b * C.cbs_levels + l1) * row + i) * G.levels;
            dst[0] = neg ? (int32_t)((S)y >> G.sh1) : (int32_t)(y >> G.sh1);   // d_1, unmasked: [-B / 2, B / 2]
            uint32_t sh = G.sh1;
            for (uint32_t l = 1; l < G.levels; ++l) {
                sh -= G.base_log;
                dst[l] = (int32_t)((y >> sh) & G.mask) - (int32_t)G.half;
            }
        }
    }
}

// launchers (prime_manylut.hip), T = uint32_t / uint64_t; grid from ew_grid, stream = the STREAM_BYTES policy decided by the caller
template <class T>
hipError_t launch_prime_modswitch_manylut(uint32_t *rot_t, const T *lwe, T p, int logn, unsigned log_lut, size_t lwe_dim, size_t batch,
                                          unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_cbs_manylut_setup(uint32_t *rot_t, T *table, const T *lwe, const PrimeCbsSetup<T> &C, unsigned log_lut, size_t lwe_dim,
                                          size_t batch, unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_sample_extract_many(T *lwe_out, const T *glwe, T p, int logn, size_t glwe_dim, size_t count, size_t batch, bool stream,
                                            unsigned grid, hipStream_t st);
template <class T>
hipError_t launch_prime_cbs_manylut_extract(int32_t *digits, const T *acc, const PrimePackConst<T> &G, const PrimeCbsSetup<T> &C, size_t batch,
                                            unsigned grid, hipStream_t st);

}  // namespace cntt
