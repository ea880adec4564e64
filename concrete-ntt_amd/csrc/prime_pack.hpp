// The two kernels the LWE-to-GLWE packing keyswitch of the prime plans (include/cntt_prime_pack.h) adds to the fused mul_accumulate
// chain it runs on:
//     prime_pack_decompose_kernel   terms[g][(i - i0) levels + l - 1][t] = -d_l(in[g][t][i]) mod p (t < m), 0 (m <= t < n)  for one chunk
//                                   of mask words [i0, i0 + nw): the negated digit polynomials, i.e. the LWE list transposed through LDS
//                                   with the signed gadget decomposition mod p of cntt_prime_pbs.h fused into the transpose
//     prime_pack_body_kernel        out[g][q] = 0 (q < k),  out[g][k][t] = in[g][t][Lin] (t < m), 0 beyond: the accumulator's start
// The loop between them is host code (host_prime_pack.inc) over external_product_device.  The kernels are instantiated in
// prime_pack.hip; host_prime.hip sees the launchers only.  This is native_pack.hpp transposed to words mod p: the tile is the same, the
// digit rule is that of prime_pbs.hpp.
//
// The transpose.  The input is contiguous along i (the words of one ciphertext), the output along t (the coefficients of one digit
// polynomial).  A 256-thread workgroup owns a tile of TT = 64 ciphertexts x TI = 32 mask words of one batch element g.  It loads the
// tile with lanes running along i -- 32 consecutive words of a ciphertext per 32 lanes, two ciphertexts per wave; a ciphertext has
// Lin + 1 words, so its rows are not 16-byte aligned in general and the loads are one word each -- and parks the canonical word x in
// LDS.  After the barrier wave v takes the mask words v, v + 4, ... of the tile with lane = t: one LDS read, the lift (below), then per
// level a shift, a mask, a compare and a subtraction, and ONE coalesced store of 64 consecutive words of digit polynomial (i, l).
//
// LDS rows are padded by one WORD (ROW = TI + 1 = 33 words).  Word index of (t, i) is t ROW + i, so with D = sizeof(T) / 4 dwords per word:
//   store (lanes along i, t fixed per 32 lanes; every ds_write banks modulo 32 dwords and serves 32 / D contiguous lanes per cycle):
//     the 32 / D lanes of a group hold consecutive i of one row (32 / D divides TI = 32) = 32 consecutive dwords: no conflict.
//   load (lanes along t, i fixed): lane t starts at dword D (t ROW + i).
//     4 bytes, ds_read_b32, groups of 32 lanes, 32 banks: t * 33 mod 32 = t, all different.
//     8 bytes, ds_read_b64, groups of 32 lanes, 64 banks, two per lane: 2 (t * 33 mod 32) = 2 t, the 32 pairs tile the 64 banks.
//   An even ROW would put t and t + 32 / gcd(ROW, 32) on one bank; ROW = 33 is odd.
//
// The digits.  T = the word type (TB bits), W = bit length of p, s = W - base_log levels, B = 2^base_log, x' = the balanced lift of x.
// y = x' + off with off = 2^(s-1) + sum_{l >= 2} (B/2) 2^(W - base_log l) (PrimeGadgetConst::off) holds digit l >= 2, offset by B/2, in
// its bits [W - base_log l, W - base_log (l-1)), and floor(y / 2^(W - base_log)) is the top digit, signed and unmasked, in
// [-B/2, B/2].  -2^(W-1) < y < 2^W: one bit more than a word when W = TB.  So LDS holds the canonical x, not y, and the lift follows the
// transposed read -- a compare, a select and an add per word, once for all levels -- which keeps a word a word (and the bank argument
// above as it stands) where parking y would need a 65th bit next to it.  The top digit takes the form of prime_keyswitch.hpp:
// x > (p - 1) / 2 is x >= p - x for odd p; then y < 2^(W-1), and y is negative exactly when the top bit of y mod 2^TB is set, where an
// arithmetic shift is the floor; otherwise the shift is logical.  sh1 = 0 (one level, base_log = W) is a shift by nothing of y = x'.
//
// The stored word is the NEGATED digit, canonical mod p, so that the external product accumulates -sum D (*) K:
//     top digit d_1:                        d_1 > 0 ? p - d_1 : -d_1
//     lower levels, field e = d + B/2:      e <= B/2 ? B/2 - e : p + B/2 - e
// A word x = 0 gives y = off, whose top digit is 0 (off < 2^(W - base_log)) and whose fields are all B/2: every stored word is 0.  The
// tail t >= m of every digit polynomial is therefore written by the same stores from x = 0 (tiles wholly past m skip the load), and no
// memset precedes the kernel.  Every bound is checked per word.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace cntt {

constexpr int PPACK_TT = 64;   // ciphertexts of one tile = the run of coefficients one wave stores
constexpr int PPACK_TI = 32;   // mask words of one tile

// constants of one call (prime_pack_const in host_prime_pack.inc, from gadget_const)
template <class T> struct PrimePackConst {
    T p, off;        // modulus; 2^(s-1) + K' 2^s of prime_pbs.hpp
    T mask, half;    // B - 1 (read by the levels below the top only: base_log <= W / 2 there),  B / 2
    uint32_t sh1;    // W - base_log: position of the top digit
    uint32_t base_log, levels;
};

// in: batch x m ciphertexts of lin + 1 canonical words; terms: batch x nw * levels polynomials of n = 2^logn words; i0 + nw <= lin, m <= n.
// Grid-stride over the tiles, the i tiles of one (g, t tile) next to each other.
template <class T>
__global__ __launch_bounds__(256) void prime_pack_decompose_kernel(T *__restrict__ terms, const T *__restrict__ in, const PrimePackConst<T> G,
                                                                   uint32_t logn, size_t lin, size_t m, size_t i0, uint32_t nw, size_t batch) {
    using S = typename std::make_signed<T>::type;
    constexpr uint32_t TT = PPACK_TT, TI = PPACK_TI, ROW = TI + 1;
    static_assert(ROW % 2 == 1 && (TT * TI) % 256 == 0 && TI % (32 / (sizeof(T) / 4)) == 0, "see the bank rules above");
    __shared__ __attribute__((aligned(16))) T tile[TT][ROW];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t n = (size_t)1 << logn, tt_tiles = (n + TT - 1) / TT, ti_tiles = (nw + TI - 1) / TI, tiles = batch * tt_tiles * ti_tiles;
    for (size_t q = blockIdx.x; q < tiles; q += gridDim.x) {
        const uint32_t ib = (uint32_t)(q % ti_tiles) * TI;   // first mask word of the tile, counted from i0
        const size_t r = q / ti_tiles, t0 = (r % tt_tiles) * TT, g = r / tt_tiles;
        if (t0 < m) {   // (the same for the whole workgroup) a tile wholly past m stores zeros only
#pragma unroll
            for (uint32_t e = threadIdx.x; e < TT * TI; e += 256u) {
                const uint32_t ii = e % TI, tt = e / TI;
                const size_t t = t0 + tt;
                if (t < m && ib + ii < nw) tile[tt][ii] = in[(g * m + t) * (lin + 1) + i0 + ib + ii];
            }
        }
        __syncthreads();
        const size_t t = t0 + lane;
        if (t < n) {
            for (uint32_t ii = wave; ii < TI && ib + ii < nw; ii += 4u) {
                T x = 0;   // past m: the digits of zero, all zero
                if (t < m) x = tile[lane][ii];
                const bool hi = x >= (T)(G.p - x);
                const T y = (T)(x + G.off - (hi ? G.p : (T)0));
                const bool neg = hi && (S)y < 0;
                T *dst = terms + (((g * nw + ib + ii) * G.levels) << logn) + t;
                // -d_1: |d_1| of a negative top digit as it stands, p - d_1 of a positive one
                const T d1 = neg ? (T)(0 - (T)((S)y >> G.sh1)) : (T)(y >> G.sh1);
                *dst = neg || d1 == 0 ? d1 : (T)(G.p - d1);
                uint32_t sh = G.sh1;
                for (uint32_t l = 1; l < G.levels; ++l) {
                    sh -= G.base_log;
                    dst += n;
                    const T e = (T)((y >> sh) & G.mask);   // the digit + B / 2
                    *dst = e <= G.half ? (T)(G.half - e) : (T)(G.p - e + G.half);
                }
            }
        }
        __syncthreads();   // the tile has been read
    }
}

// one thread per output word, grid-stride; the body words of the m ciphertexts are lin + 1 words apart (a gather of batch * m words)
template <class T>
__global__ __launch_bounds__(256) void prime_pack_body_kernel(T *__restrict__ out, const T *__restrict__ in, uint32_t logn, size_t glwe_dim,
                                                              size_t lin, size_t m, size_t batch) {
    const size_t per = (glwe_dim + 1) << logn, total = batch * per, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t g = i / per, r = i - g * per, c = r & (((size_t)1 << logn) - 1);
        if ((r >> logn) == glwe_dim && c < m) out[i] = in[(g * m + c) * (lin + 1) + lin];
        else out[i] = 0;
    }
}

// launchers (prime_pack.hip), T = uint32_t / uint64_t; grid of the body kernel from ew_grid
template <class T>
hipError_t launch_prime_pack_decompose(T *terms, const T *in, const PrimePackConst<T> &G, int logn, size_t lin, size_t m, size_t i0, size_t nw,
                                       size_t batch, hipStream_t st);
template <class T>
hipError_t launch_prime_pack_body(T *out, const T *in, int logn, size_t glwe_dim, size_t lin, size_t m, size_t batch, unsigned grid,
                                  hipStream_t st);

}  // namespace cntt
