// The many-LUT bootstrap of the native plans and the circuit bootstrap with one rotation per input bit (include/cntt_manylut.h).
// Three kernels around the unchanged blind rotation (blind_rotate_device of pbs_host.hpp) and the unchanged functional keyswitch
// (native_cbs_ks_kernel, native_cbs_sum_kernel of native_cbs.hpp), t = log_lut_count, n' = n / 2^t; the words W are u32 / u64 / Word128
// through WordOps<W>, the residue kinds never enter:
//     native_modswitch_manylut_kernel     the tiled transpose of native_lwe_modswitch_kernel with the coarse rule ms_t(x) = ms_{n'}(x) << t;
//                                         the CBS variant adds 2^(w - 2) to the body on the way (bit 30 of the top 32 bits) and writes the
//                                         one shared table of the circuit bootstrap, v[m 2^t + h] = 2^w - H_(h+1) for h < Lc and 0 above
//     native_sample_extract_many_kernel   the extraction at the indices 0 .. count - 1 from ONE read of the accumulator (below)
//     native_cbs_manylut_extract_kernel   the circuit bootstrap's extraction at the indices l - 1, + H_l on the body and the R Lc signed
//                                         int32 digits in the layout native_cbs_ks_kernel reads; u is never stored
// The kernels are instantiated in native_manylut.hip; host_native_ext.hip sees the launchers only.
//
// The window of native_sample_extract_many_kernel, that of prime_sample_extract_many_kernel.  Row h of an element takes, for the mask
// polynomial f and the destination word j, the source f[h - j] (negated past the wrap).  A thread owns the NV = 16 / sizeof(W)
// destination words j .. j + NV - 1 of a chunk of at most NEXM_ROWS = 8 rows h0 .. h0 + 7: its sources f[h - j - i] are the
// NEXM_ROWS + NV - 1 consecutive words from h0 - j - NV + 1 on, reversed.  j and h0 are multiples of NV, so the window is covered by
// 1 + NEXM_ROWS / NV whole vectors of NV words starting at h0 - j - NV, and n is a multiple of NV, so a vector never straddles the wrap:
// one sign per vector.  Every load is 16 bytes, every store 16 bytes along the row.  A row of the output has k n + 1 words, so on 32- and
// 64-bit words its vectors are aligned to the word only, and so is a caller's glwe: both sides use a vector type aligned to sizeof(W)
// (global memory takes such an access whole).  A Word128 is its own 16-byte vector, aligned as such.
#pragma once
#include "native_cbs.hpp"
#include "native_pbs.hpp"

namespace cntt {

constexpr uint32_t NEXM_ROWS = 8;   // rows of one chunk of the extraction: the window stays in registers

// 16 bytes at the alignment of a word of `Bytes` bytes
typedef uint32_t NativeExmVec __attribute__((ext_vector_type(4)));
template <size_t Bytes> struct NativeExmAligned;
template <> struct NativeExmAligned<4> {
    typedef NativeExmVec type __attribute__((aligned(4)));
};
template <> struct NativeExmAligned<8> {
    typedef NativeExmVec type __attribute__((aligned(8)));
};
template <> struct NativeExmAligned<16> {
    typedef NativeExmVec type;
};

// rot_t[i batch + b] = ms_t(lwe'[b][i]) (i < L), rot_t[L batch + b] = 2n - ms_t(lwe'[b][L]) mod 2n, with
// ms_t(x) = ((((x >> (w - (logn - t) - 2)) + 1) >> 1) mod 2n') << t on the top 32 bits of the word.  CBS: lwe' = lwe with 2^(w - 2) added
// to the body (bit 30 of the top 32 bits, as native_cbs_setup_kernel does it), and the blocks past the tiles write the table's (k + 1) n
// words (16-byte vectors, 256 per block and trip).  Tiles as native_lwe_modswitch_kernel: read along i, written along b, every bound
// checked per word.  C.cbs_levels <= 2^t (the launcher checks).
template <class W, bool CBS>
__global__ __launch_bounds__(256) void native_modswitch_manylut_kernel(uint32_t *__restrict__ rot_t, W *__restrict__ table,
                                                                       const W *__restrict__ lwe, const NativeCbsConst C, uint32_t log_lut,
                                                                       size_t lwe_dim, size_t batch) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = NativeExmVec;
    __shared__ uint32_t tile[PBS_TILE][PBS_TILE + 1];
    const size_t row = lwe_dim + 1, ti = (row + PBS_TILE - 1) / PBS_TILE, tb = (batch + PBS_TILE - 1) / PBS_TILE, tiles = ti * tb;
    const size_t nvec = CBS ? ((size_t)(C.k + 1u) << (C.logn - LOGV)) : 0, vblocks = (nvec + 255) / 256;
    const uint32_t tx = threadIdx.x & (PBS_TILE - 1), ty = threadIdx.x / PBS_TILE;   // ty < 8
    const uint32_t mask = (2u << C.logn) - 1u, sh = 32u - (C.logn - log_lut) - 2u, cmask = (2u << (C.logn - log_lut)) - 1u;
    for (size_t t = blockIdx.x; t < tiles + vblocks; t += gridDim.x) {
        if (t >= tiles) {   // CBS only: one block of table vectors (uniform per block: no barrier is skipped by part of a block)
            const size_t v = (t - tiles) * 256 + threadIdx.x;
            if (v < nvec) {
                const uint32_t q = (uint32_t)(v >> (C.logn - LOGV)), pos0 = (uint32_t)(v & (((size_t)1 << (C.logn - LOGV)) - 1)) << LOGV;
                union {
                    W w[NV];
                    V v;
                } d;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const uint32_t h = (pos0 + (uint32_t)j) & ((1u << log_lut) - 1u);
                    d.w[j] = q == C.k && h < C.cbs_levels ? O::sub(native_cbs_zero<W>(), native_cbs_h<W>(C.cbs_base_log, h + 1u))
                                                          : native_cbs_zero<W>();
                }
                reinterpret_cast<V *>(table)[v] = d.v;
            }
            continue;
        }
        const size_t i0 = (t % ti) * PBS_TILE, b0 = (t / ti) * PBS_TILE;
#pragma unroll
        for (uint32_t r = ty; r < PBS_TILE; r += 8) {
            const size_t b = b0 + r, i = i0 + tx;
            if (b < batch && i < row) {
                uint32_t top = native_cbs_top32<W>(lwe[b * row + i]);
                if (CBS && i == lwe_dim) top += 1u << 30;
                uint32_t m = ((((top >> sh) + 1u) >> 1) & cmask) << log_lut;
                if (i == lwe_dim) m = (0u - m) & mask;
                tile[r][tx] = m;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = ty; r < PBS_TILE; r += 8) {
            const size_t i = i0 + r, b = b0 + tx;
            if (i < row && b < batch) rot_t[i * batch + b] = tile[tx][r];
        }
        __syncthreads();
    }
}

// lwe_out[b][h][q n + j] = glwe[b][q][h - j], negated mod 2^w past the wrap (j > h), and lwe_out[b][h][k n] = glwe[b][k][h], for h < count.
// Work item = (element, mask polynomial, chunk of NEXM_ROWS rows, vector of NV destination words), the vectors of one row next to each
// other; the batch * count body words are the tail of the same grid-stride walk.  Rows past count are neither formed nor stored, and
// the vectors of the window that only they would read are not loaded.  STREAM: the output is larger than STREAM_BYTES.
template <class W, bool STREAM>
__global__ __launch_bounds__(256) void native_sample_extract_many_kernel(W *__restrict__ lwe_out, const W *__restrict__ glwe, uint32_t logn,
                                                                         size_t glwe_dim, size_t count, size_t batch) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0, NW = 1 + (int)NEXM_ROWS / NV;   // vectors of the window
    using V4 = NativeExmVec;
    using V = typename NativeExmAligned<sizeof(W)>::type;
    const uint32_t lv = logn - LOGV, n = 1u << logn;
    const size_t kn = glwe_dim << logn, row = kn + 1, chunks = (count + NEXM_ROWS - 1) / NEXM_ROWS;
    const size_t nmask = (batch * glwe_dim * chunks) << lv, total = nmask + batch * count, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (t >= nmask) {   // the body words
            const size_t e = t - nmask, b = e / count, h = e - b * count;
            lwe_out[e * row + kn] = glwe[((b * (glwe_dim + 1)) << logn) + kn + h];
            continue;
        }
        const uint32_t j = (uint32_t)(t & (((size_t)1 << lv) - 1)) << LOGV;
        const size_t t1 = t >> lv, c = t1 % chunks, t2 = t1 / chunks, q = t2 % glwe_dim, b = t2 / glwe_dim;
        const uint32_t h0 = (uint32_t)c * NEXM_ROWS, rows = (uint32_t)(count - h0 < NEXM_ROWS ? count - h0 : NEXM_ROWS);
        const W *f = glwe + ((b * (glwe_dim + 1) + q) << logn);
        // win[r] = the source at h0 - j - NV + r with its sign; row h0 + hh takes win[hh - i + NV] for the destination word j + i
        W win[NW * NV];
#pragma unroll
        for (int m = 0; m < NW; ++m) {
            if ((uint32_t)(m * NV) <= rows - 1u + (uint32_t)NV) {   // else only rows past `rows` would read it
                const uint32_t s = (h0 - j - (uint32_t)NV + (uint32_t)(m * NV)) & (2u * n - 1u);
                union {
                    W w[NV];
                    V4 v;
                } x;
                x.v = *reinterpret_cast<const V *>(f + (s & (n - 1u)));
#pragma unroll
                for (int i = 0; i < NV; ++i) win[m * NV + i] = O::neg_if(x.w[i], (s & n) != 0);
            }
        }
        W *dst = lwe_out + ((b * count + h0) * row + (q << logn) + j);
#pragma unroll
        for (uint32_t hh = 0; hh < NEXM_ROWS; ++hh) {
            if (hh < rows) {
                union {
                    W w[NV];
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
// native_cbs_extract_kernel through the same WordOps and GadgetConst: y = x + off, then per level ((y >> sh) & mask) - half.
template <class W>
__global__ __launch_bounds__(256) void native_cbs_manylut_extract_kernel(int32_t *__restrict__ digits, const W *__restrict__ acc,
                                                                         const GadgetConst<W> G, const NativeCbsConst C, size_t batch) {
    using O = WordOps<W>;
    const uint32_t n = 1u << C.logn;
    const size_t lin = (size_t)C.k << C.logn, row = lin + 1, total = batch * row;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t b = t / row, i = t - b * row;
        const W *g = acc + ((b * (C.k + 1u)) << C.logn);
        const uint32_t pos = (uint32_t)(i & (n - 1u));
        const W *f = g + (i - pos);   // the polynomial of word i; the body polynomial for i == lin (pos = 0)
        for (uint32_t l1 = 0; l1 < C.cbs_levels; ++l1) {
            W x;
            if (i == lin) {
                x = O::add(f[l1], native_cbs_h<W>(C.cbs_base_log, l1 + 1u));
            } else {
                const uint32_t s = (l1 - pos) & (2u * n - 1u);
                x = O::neg_if(f[s & (n - 1u)], (s & n) != 0);
            }
            const W y = O::add(x, G.off);
            int32_t *dst = digits + ((b * C.cbs_levels + l1) * row + i) * G.levels;
            uint32_t sh = (uint32_t)O::BITS;
            for (uint32_t l = 0; l < G.levels; ++l) {
                sh -= G.base_log;
                dst[l] = (int32_t)(native_cbs_low32<W>(O::band(O::shr(y, sh), G.mask)) - native_cbs_low32<W>(G.half));
            }
        }
    }
}

// launchers (native_manylut.hip): word = 4 / 8 / 16 bytes; grid from ew_grid, stream = the STREAM_BYTES policy decided by the caller;
// off = the word gadget_offset gives (host_native_ext.hip), in two halves
hipError_t launch_native_modswitch_manylut(int word, uint32_t *rot_t, const void *lwe, int logn, unsigned log_lut, size_t lwe_dim, size_t batch,
                                           unsigned grid, hipStream_t st);
hipError_t launch_native_cbs_manylut_setup(int word, uint32_t *rot_t, void *table, const void *lwe, const NativeCbsConst &C, unsigned log_lut,
                                           size_t lwe_dim, size_t batch, unsigned grid, hipStream_t st);
hipError_t launch_native_sample_extract_many(int word, void *lwe_out, const void *glwe, int logn, size_t glwe_dim, size_t count, size_t batch,
                                             bool stream, unsigned grid, hipStream_t st);
hipError_t launch_native_cbs_manylut_extract(int word, int32_t *digits, const void *acc, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                             unsigned levels, const NativeCbsConst &C, size_t batch, unsigned grid, hipStream_t st);

}  // namespace cntt
