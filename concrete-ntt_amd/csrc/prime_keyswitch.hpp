// LWE keyswitch of the prime plans (include/cntt_prime_keyswitch.h): a tiled integer GEMM mod p on the VALU,
//     out[b][c] = (c == Lout ? in[b][Lin] : 0) - sum_{i < Lin} sum_{l = 1..levels} d_l(in[b][i]) ksk[(i levels + l - 1) row_stride + c]   mod p
// with d_1 .. d_levels the digits of cntt_prime_pbs.h (balanced lift, top digit unmasked).  The kernel is instantiated in
// prime_keyswitch.hip; host_prime.hip sees the launcher only.
//
// Tiling: that of native_keyswitch.hpp.  A 256-thread workgroup owns BM = 4 TB batch elements x BN = 64 TC columns: wave v the batch
// elements v TB .. v TB + TB - 1, lane x the columns x, x + 64, ...  A key load of a wave is 64 consecutive words of one key row; a digit
// is the same LDS word for all 64 lanes (a broadcast read).  The Lin mask words are walked in chunks; a chunk's words are loaded ONCE per
// workgroup and their digits staged in LDS as 32-bit numbers; there is no digits buffer in memory.
//
// Digits.  The rule of prime_pbs.hpp (PrimeGadgetConst): y = x' + off holds digit l >= 2, offset by B/2, in its bits
// [W - base_log l, W - base_log (l-1)), and the top digit is floor(y / 2^(W - base_log)), signed and unmasked, in [-B/2, B/2].  The staged
// number is u = d + B/2: the bit field as it stands below the top, the top digit plus B/2 at the top -- in [0, B], NOT [0, B), so
// u <= 2^31 for base_log <= 31.  The surplus (B/2) sum_r ksk[r][c] mod p does not depend on the batch element: every thread sums the key
// words it loads anyway and the epilogue takes it off:  out = body + (B/2) ksum - acc  mod p.
//
// Nothing wraps.  u k < 2^(base_log + 32) for a 32-bit half k of a key word, so a 64-bit sum of such products holds
// 2^(32 - base_log) rows.  A thread keeps one such lazy sum per (element, column) for u32 words and two (the halves of the key word) for
// u64 words -- one v_mad_u64_u32 each per row -- and folds them at every chunk boundary into a running total of 96 / 128 bits with plain
// carry adds.  A chunk is min(KS_ROWS, 2^(32 - base_log)) rows rounded down to whole words (2^(32 - b) >= floor(64 / b) >= levels for
// every b <= 31: at least one word).  The total stays below rows 2^63 < 2^95 (u32 words), rows 2^95 < 2^127 (u64 words) for
// rows = Lin levels < 2^32, and the key-word sums below rows 2^32 resp. rows 2^64.  ONE reduction mod p per output word, in the
// epilogue: every limb x of the total (any word, not canonical) goes through mont_mul(x, R^(j+1) mod p) = x R^j mod p
// (ntt_arith.hpp; exact for every odd p below the word), R = 2^32 / 2^64 -- no division anywhere on the device.
//
// Registers per accumulator: 2 + 3 (u32 words), 4 + 4 (u64 words), against 1 / 3 of the native kernel; with the 8 x 2 tile below the
// kernels have no scratch and no spilled register (gfx950: 140 VGPRs on u32 words, 190 on u64 words -- DESIGN.md, "Prime keyswitch").
// The scalar file is what runs full (about 100 SGPRs of loop invariants), hence the few constants of PrimeKsConst.
#pragma once
#include <cstddef>
#include <type_traits>

#include "ntt_arith.hpp"

namespace cntt {

constexpr int PKS_ROWS = 128;   // digit rows (one per (word, level)) of one chunk in LDS at most; >= the largest `levels` (64: base_log 1, W 64)

// rows of one chunk: what a lazy 64-bit sum holds, and what LDS holds
__host__ __device__ constexpr uint32_t prime_ks_chunk_rows(uint32_t base_log) {
    return base_log <= 25 ? (uint32_t)PKS_ROWS : 1u << (32u - base_log);
}

// register tile of one thread: TB batch elements x TC columns, for both word types.  An accumulator is 5 (u32 words) or 8 (u64 words)
// registers against 1 and 3 of the native kernel, whose 16 x 2 tile would leave one wave per SIMD here (262 registers on u32 words)
template <class T> struct PrimeKsTile {
    static constexpr int TB = 8, TC = 2;
};

// constants of one call (prime_ks_const in host_prime_keyswitch.inc)
template <class T> struct PrimeKsConst {
    T p, off;      // modulus; 2^(s-1) + K' 2^s of prime_pbs.hpp (PrimeGadgetConst::off)
    uint32_t sh1;  // W - base_log: position of the top digit
    uint32_t base_log, levels;
    T pinv_neg;    // -p^-1 mod R
    T r2;          // R^2 mod p
};

// what the epilogue's reductions multiply by, derived from r2 on the device (once per tile, in vector registers: the scalar file is full)
template <class T> struct PrimeKsRed {
    T p, pinv_neg;
    T r[3];        // R, R^2, R^3 mod p
    T half_r;      // (B/2) R mod p
    __device__ __forceinline__ PrimeKsRed(const PrimeKsConst<T> &K) : p(K.p), pinv_neg(K.pinv_neg) {
        r[1] = K.r2;
        r[0] = mont_mul(r[1], (T)1, p, pinv_neg);
        r[2] = mont_mul(r[1], r[1], p, pinv_neg);
        half_r = mont_mul((T)((T)1 << (K.base_log - 1u)), r[1], p, pinv_neg);
    }
    // x R^j mod p for ANY word x
    __device__ __forceinline__ T red(T x, int j) const { return mont_mul(x, r[j], p, pinv_neg); }
};

// The accumulator of one (batch element, column) pair: lazy sums, the running total, and the one reduction.
template <class T> struct PrimeKsAcc;
template <> struct PrimeKsAcc<uint32_t> {
    uint64_t lazy = 0, lo = 0;
    uint32_t hi = 0;   // total = hi 2^64 + lo
    __device__ __forceinline__ void mad(uint32_t u, uint32_t k) { lazy += (uint64_t)u * k; }
    __device__ __forceinline__ void fold() {
        lo += lazy;
        hi += lo < lazy;
        lazy = 0;
    }
    __device__ __forceinline__ uint32_t value(const PrimeKsRed<uint32_t> &K) const {
        const uint32_t p = K.p;
        return add_mod(add_mod(K.red((uint32_t)lo, 0), K.red((uint32_t)(lo >> 32), 1), p),
                       K.red(hi, 2), p);
    }
};
template <> struct PrimeKsAcc<uint64_t> {
    using A = unsigned __int128;
    uint64_t lazy_lo = 0, lazy_hi = 0;   // sums of u * (low / high half of k)
    A total = 0;
    __device__ __forceinline__ void mad(uint32_t u, uint64_t k) {
        lazy_lo += (uint64_t)u * (uint32_t)k;
        lazy_hi += (uint64_t)u * (uint32_t)(k >> 32);
    }
    __device__ __forceinline__ void fold() {
        total += (A)lazy_lo + ((A)lazy_hi << 32);
        lazy_lo = lazy_hi = 0;
    }
    __device__ __forceinline__ uint64_t value(const PrimeKsRed<uint64_t> &K) const {
        return add_mod(K.red((uint64_t)total, 0), K.red((uint64_t)(total >> 64), 1), K.p);
    }
};

// the sum of the key words of one column: below rows 2^32 (u32 words), rows 2^64 (u64 words)
template <class T> struct PrimeKsSum;
template <> struct PrimeKsSum<uint32_t> {
    uint64_t v = 0;
    __device__ __forceinline__ void add(uint32_t k) { v += k; }
    __device__ __forceinline__ uint32_t value(const PrimeKsRed<uint32_t> &K) const {
        return add_mod(K.red((uint32_t)v, 0), K.red((uint32_t)(v >> 32), 1), K.p);
    }
};
template <> struct PrimeKsSum<uint64_t> {
    uint64_t lo = 0;
    uint32_t hi = 0;
    __device__ __forceinline__ void add(uint64_t k) {
        lo += k;
        hi += lo < k;
    }
    __device__ __forceinline__ uint64_t value(const PrimeKsRed<uint64_t> &K) const {
        return add_mod(K.red(lo, 0), K.red((uint64_t)hi, 1), K.p);
    }
};

// row_stride >= lout + 1, in words; levels <= the chunk rows, base_log <= 31, lin levels < 2^32, fewer than 2^32 - 2^24 tiles (the launcher
// refuses the rest).
// Grid-stride over the tiles, column tiles of one batch tile next to each other; every bound is checked per word.
template <class T>
__global__ __launch_bounds__(256) void prime_keyswitch_kernel(T *__restrict__ out, const T *__restrict__ in, const T *__restrict__ ksk,
                                                              const PrimeKsConst<T> K, uint32_t lin, size_t lout, size_t row_stride, size_t batch) {
    using S = typename std::make_signed<T>::type;
    constexpr int TB = PrimeKsTile<T>::TB, TC = PrimeKsTile<T>::TC, BM = 4 * TB, BN = 64 * TC;
    static_assert(TB % 4 == 0, "a thread reads its digits sixteen bytes at a time");
    __shared__ __attribute__((aligned(16))) uint32_t dig[PKS_ROWS][BM];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // uniform: the batch bounds of the epilogue are scalar branches
    const uint32_t base_log = K.base_log, levels = K.levels;
    const size_t ncol = lout + 1;
    const uint32_t ct = (uint32_t)((ncol + BN - 1) / BN), bt = (uint32_t)((batch + BM - 1) / BM);
    const uint32_t kc = prime_ks_chunk_rows(base_log) / levels;   // words per chunk
    const uint32_t mask = (1u << base_log) - 1u, half = 1u << (base_log - 1u);
    for (uint32_t t = blockIdx.x; t < ct * bt; t += gridDim.x) {   // the launcher keeps the tile count below 2^32
        const size_t c0 = (size_t)(t % ct) * BN, b0 = (size_t)(t / ct) * BM;
        PrimeKsAcc<T> acc[TB][TC];
        PrimeKsSum<T> ksum[TC];
        size_t col[TC];   // a column past the row reads the row's last word instead: loaded, summed, never stored
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            const size_t c = c0 + lane + 64u * (uint32_t)j;
            col[j] = c < ncol ? c : lout;
        }
        for (uint32_t i0 = 0, nw; i0 < lin; i0 += nw) {   // (i0 + nw <= lin: no wrap)
            nw = lin - i0 < kc ? lin - i0 : kc;
            __syncthreads();   // the previous chunk's digits have been read
            // uniform trip counts throughout: only the stores are predicated
            const uint32_t ne = nw * BM;
            for (uint32_t e0 = 0; e0 < ne; e0 += 256u) {
                const uint32_t e = e0 + threadIdx.x, ii = e / BM, bb = e % BM;
                const size_t b = b0 + bb;
                // a batch element past the end: the digits of zero, whose products are never stored
                const T x = e < ne && b < batch ? in[b * ((size_t)lin + 1) + i0 + ii] : (T)0;
                // the digit rule of prime_gadget_kernel with fewer constants (the scalar file is full): x > (p - 1) / 2 is x >= p - x for odd p; and
                // with hi, y = x' + off < 2^(W-1) is negative exactly when the top bit of y mod 2^TB is set (-2^(W-1) < y), where an
                // arithmetic shift is the floor that the logical one minus topsub is
                const bool hi = x >= (T)(K.p - x);
                const T y = (T)(x + K.off - (hi ? K.p : (T)0));
                const bool neg = hi && (S)y < 0;
                if (e < ne) {
                    uint32_t *d = &dig[ii * levels][bb];
                    // the top digit, signed and unmasked, plus B/2: in [0, B], so its low 32 bits are the number
                    *d = (uint32_t)(neg ? (T)((S)y >> K.sh1) : (T)(y >> K.sh1)) + half;
                    uint32_t sh = K.sh1;
                    for (uint32_t l = 1; l < levels; ++l) {
                        sh -= base_log;
                        d += BM;
                        *d = (uint32_t)(y >> sh) & mask;   // the digit + B/2
                    }
                }
            }
            __syncthreads();
            const uint32_t nr = nw * levels;
            const T *krow = ksk + (size_t)(i0 * levels) * row_stride;
#pragma unroll 2
            for (uint32_t rr = 0; rr < nr; ++rr, krow += row_stride) {
                T k[TC];
#pragma unroll
                for (int j = 0; j < TC; ++j) k[j] = krow[col[j]];
                uint32_t u[TB];
#pragma unroll
                for (int q = 0; q < TB / 4; ++q) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(&dig[rr][wave * TB + 4 * q]);
                    u[4 * q] = v.x, u[4 * q + 1] = v.y, u[4 * q + 2] = v.z, u[4 * q + 3] = v.w;
                }
#pragma unroll
                for (int j = 0; j < TC; ++j) {
                    ksum[j].add(k[j]);
#pragma unroll
                    for (int i = 0; i < TB; ++i) acc[i][j].mad(u[i], k[j]);
                }
            }
            // the lazy sums are full after this many rows at the most
#pragma unroll
            for (int j = 0; j < TC; ++j)
#pragma unroll
                for (int i = 0; i < TB; ++i) acc[i][j].fold();
        }
        // out = body + (B/2) ksum - acc  mod p
        const PrimeKsRed<T> R(K);
        T corr[TC];
#pragma unroll
        for (int j = 0; j < TC; ++j) corr[j] = mont_mul(ksum[j].value(R), R.half_r, K.p, K.pinv_neg);
#pragma unroll
        for (int i = 0; i < TB; ++i) {
            const size_t b = b0 + wave * TB + (uint32_t)i;
            if (b >= batch) break;
            const T body = in[b * ((size_t)lin + 1) + lin];
#pragma unroll
            for (int j = 0; j < TC; ++j) {
                const size_t c = c0 + lane + 64u * (uint32_t)j;
                if (c >= ncol) continue;
                T v = sub_mod(corr[j], acc[i][j].value(R), K.p);
                if (c == lout) v = add_mod(v, body, K.p);
                out[b * ncol + c] = v;
            }
        }
    }
}

// launcher (prime_keyswitch.hip), T = uint32_t / uint64_t
template <class T>
hipError_t launch_prime_keyswitch(T *out, const T *in, const T *ksk, const PrimeKsConst<T> &K, size_t lin, size_t lout, size_t row_stride,
                                  size_t batch, hipStream_t st);

}  // namespace cntt
