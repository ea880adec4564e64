// The two kernels the LWE-to-GLWE packing keyswitch of the native / native_binary plans (include/cntt_pack.h) adds to the external
// product it runs on:
//     native_pack_decompose_kernel   terms[g][(i - i0) levels + l - 1][t] = -d_l(in[g][t][i]) (t < m), 0 (m <= t < n)  for one chunk of
//                                    mask words [i0, i0 + nw): the negated digit polynomials, i.e. the LWE list transposed through LDS
//                                    with the signed gadget decomposition of cntt_gadget.h fused into the transpose
//     native_pack_body_kernel        out[g][p] = 0 (p < k),  out[g][k][t] = in[g][t][Lin] (t < m), 0 beyond: the accumulator's start
// The loop between them is host code (host_native_ext.hip) over the external product.  The kernels are instantiated in native_pack.hip;
// host_native_ext.hip sees the launchers only.
//
// The transpose.  The input is contiguous along i (the words of one ciphertext), the output along t (the coefficients of one digit
// polynomial).  A 256-thread workgroup owns a tile of TT = 64 ciphertexts x TI mask words of one batch element g.  It loads the tile
// with lanes running along i -- TI consecutive words of a ciphertext per TI lanes, 64 / TI ciphertexts per wave; a ciphertext has
// Lin + 1 words, so its rows are not 16-byte aligned in general and the loads are one word each -- adds `off` once (below) and parks
// y in LDS.  After the barrier wave v takes the mask words v, v + 4, ... of the tile with lane = t: one LDS read, then per level a
// shift, a mask, one subtraction, and ONE coalesced store of 64 consecutive words of digit polynomial (i, l).
//
// LDS rows are padded by one WORD (ROW = TI + 1 words).  Word index of (t, i) is t ROW + i, so with D = sizeof(W) / 4 dwords per word:
//   store (lanes along i, t fixed per TI lanes; every ds_write banks modulo 32 dwords and serves 32 / D contiguous lanes per cycle):
//     the 32 / D lanes of a group hold consecutive i of one row (32 / D divides TI = 32, 32, 16) = 32 consecutive dwords: no conflict.
//   load (lanes along t, i fixed): lane t starts at dword D (t ROW + i).
//     4 bytes, ds_read_b32, groups of 32 lanes, 32 banks: t * 33 mod 32 = t, all different.
//     8 bytes, ds_read_b64, groups of 32 lanes, 64 banks, two per lane: 2 (t * 33 mod 32) = 2 t, the 32 pairs tile the 64 banks.
//     16 bytes, ds_read_b128, groups of 16 lanes whose t mod 16 are all different (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
//     the same plus 32), 64 banks, four per lane: 4 (t * 17 mod 16) = 4 (t mod 16), the 16 quadruples tile the 64 banks.
//   An even ROW would put t and t + 32 / gcd on one bank; ROW = TI + 1 is odd for every TI used.  (The 16-byte case needs the 128-bit
//   LDS instructions: Word128 is 16-byte aligned and so are its rows, 17 * 16 bytes.)
//
// The digits are the y = x + 2^(s-1) + K 2^s bit fields of native_gadget.hpp; the stored word is the NEGATED digit, B/2 - field, so
// that the external product accumulates -sum D (*) K.  The tail t >= m of every digit polynomial is written as zeros by the same
// stores (tiles wholly past m skip the load), so no memset precedes the kernel.  Every bound is checked per word.
#pragma once
#include "native_gadget.hpp"

namespace cntt {

constexpr int PACK_TT = 64;   // ciphertexts of one tile = the run of coefficients one wave stores
template <class W> struct PackTile {
    static constexpr int TI = 32;   // mask words of one tile
};
template <> struct PackTile<Word128> {
    static constexpr int TI = 16;
};

// constants of one call (any base_log <= w, as the stand-alone decomposition)
template <class W> struct PackConst {
    W off, mask, half;   // 2^(s-1) + K 2^s,  B - 1,  B / 2
    uint32_t base_log, levels;
};

// in: batch x m ciphertexts of lin + 1 words; terms: batch x nw * levels polynomials of n = 2^logn words; i0 + nw <= lin, m <= n.
// Grid-stride over the tiles, the i tiles of one (g, t tile) next to each other.
template <class W>
__global__ __launch_bounds__(256) void native_pack_decompose_kernel(W *__restrict__ terms, const W *__restrict__ in, const PackConst<W> G,
                                                                    uint32_t logn, size_t lin, size_t m, size_t i0, uint32_t nw,
                                                                    size_t batch) {
    using O = WordOps<W>;
    constexpr uint32_t TT = PACK_TT, TI = PackTile<W>::TI, ROW = TI + 1;
    static_assert(ROW % 2 == 1 && (TT * TI) % 256 == 0 && TI % (32 / (sizeof(W) / 4)) == 0, "see the bank rules above");
    __shared__ __attribute__((aligned(16))) W tile[TT][ROW];
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
                if (t < m && ib + ii < nw) tile[tt][ii] = O::add(in[(g * m + t) * (lin + 1) + i0 + ib + ii], G.off);
            }
        }
        __syncthreads();
        const size_t t = t0 + lane;
        const bool live = t < m;
        if (t < n) {
            for (uint32_t ii = wave; ii < TI && ib + ii < nw; ii += 4u) {
                W y = W{};
                if (live) y = tile[lane][ii];
                W *dst = terms + (((g * nw + ib + ii) * G.levels) << logn) + t;
                uint32_t sh = (uint32_t)O::BITS;
                for (uint32_t l = 0; l < G.levels; ++l, dst += n) {
                    sh -= G.base_log;
                    const W d = O::sub(G.half, O::band(O::shr(y, sh), G.mask));   // -(field - B/2)
                    *dst = live ? d : W{};
                }
            }
        }
        __syncthreads();   // the tile has been read
    }
}

// one thread per output word, grid-stride; the body words of the m ciphertexts are lin + 1 words apart (a gather of batch * m words)
template <class W>
__global__ __launch_bounds__(256) void native_pack_body_kernel(W *__restrict__ out, const W *__restrict__ in, uint32_t logn, size_t glwe_dim,
                                                               size_t lin, size_t m, size_t batch) {
    const size_t per = (glwe_dim + 1) << logn, total = batch * per, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t g = i / per, r = i - g * per, c = r & (((size_t)1 << logn) - 1);
        if ((r >> logn) == glwe_dim && c < m) out[i] = in[(g * m + c) * (lin + 1) + lin];
        else out[i] = W{};
    }
}

// launchers (native_pack.hip); word = 4, 8 or 16 bytes; off_lo / off_hi = the two halves of gadget_offset (off_hi: 128-bit words);
// grid of the body kernel from cntt_ew_grid
hipError_t launch_native_pack_decompose(int word, void *terms, const void *in, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                        unsigned levels, int logn, size_t lin, size_t m, size_t i0, size_t nw, size_t batch, hipStream_t st);
hipError_t launch_native_pack_body(int word, void *out, const void *in, int logn, size_t glwe_dim, size_t lin, size_t m, size_t batch,
                                   unsigned grid, hipStream_t st);

}  // namespace cntt
