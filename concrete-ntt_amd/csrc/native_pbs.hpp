// The two ends of the programmable bootstrap of the native / native_binary plans (include/cntt_pbs.h):
//     native_lwe_modswitch_kernel    LWE words -> exponents below 2n, transposed so that every iteration's `rot` is contiguous
//     native_pbs_init_kernel         acc[b][p] = X^(rot[b]) lut[p]        (the gather of native_gadget_kernel's rotate mode, no digits)
//     native_sample_extract_kernel   GLWE -> LWE of dimension k n: a reversed, negated copy per mask polynomial plus the body word
// The loop between them is host code (host_native_ext.hip, native_blind_rotate_device) over the r7 decomposition kernel and the r6 external
// product, which this file does not touch.  The kernels are instantiated in native_pbs.hip; host_native_ext.hip sees the launchers only.
#pragma once
#include "native_gadget.hpp"

namespace cntt {

// the top 32 bits of a word: ms() needs logn + 2 <= 32 of them (for the 128-bit word only the high half is read)
template <class W> __device__ __forceinline__ uint32_t pbs_top32(const W *p);
template <> __device__ __forceinline__ uint32_t pbs_top32<uint32_t>(const uint32_t *p) { return *p; }
template <> __device__ __forceinline__ uint32_t pbs_top32<uint64_t>(const uint64_t *p) { return (uint32_t)(*p >> 32); }
template <> __device__ __forceinline__ uint32_t pbs_top32<Word128>(const Word128 *p) { return (uint32_t)(p->hi >> 32); }

constexpr int PBS_TILE = 32;   // transpose tile: 32 x 32 exponents through LDS, 256 threads as 32 x 8

// rot_t[i * batch + b] = ms(lwe[b][i]) (i < L),  rot_t[L * batch + b] = 2n - ms(lwe[b][L]) mod 2n, with
// ms(x) = (((x >> (w - logn - 2)) + 1) >> 1) mod 2n.  Rows of the tile are read along i (the LWE words of one element are contiguous) and
// written along b (row i of rot_t is contiguous): both sides coalesced.  Grid-stride over the tiles; every bound is checked per word.
template <class W>
__global__ __launch_bounds__(256) void native_lwe_modswitch_kernel(uint32_t *__restrict__ rot_t, const W *__restrict__ lwe, uint32_t logn,
                                                                   size_t lwe_dim, size_t batch) {
    __shared__ uint32_t tile[PBS_TILE][PBS_TILE + 1];
    const size_t row = lwe_dim + 1, ti = (row + PBS_TILE - 1) / PBS_TILE, tb = (batch + PBS_TILE - 1) / PBS_TILE, tiles = ti * tb;
    const uint32_t tx = threadIdx.x & (PBS_TILE - 1), ty = threadIdx.x / PBS_TILE;   // ty < 8
    const uint32_t sh = 32u - logn - 2u, mask = (2u << logn) - 1u;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t i0 = (t % ti) * PBS_TILE, b0 = (t / ti) * PBS_TILE;
#pragma unroll
        for (uint32_t r = ty; r < PBS_TILE; r += 8) {
            const size_t b = b0 + r, i = i0 + tx;
            if (b < batch && i < row) {
                uint32_t m = (((pbs_top32<W>(lwe + b * row + i) >> sh) + 1u) >> 1) & mask;
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

// acc[b][p] = X^(rot[b]) lut[p] (lut_stride == 0: shared by the batch) or X^(rot[b]) lut[b][p] (lut_stride = npolys): one thread per 16
// bytes of destination, grid-stride over batch * npolys polynomials; STREAM as native_gadget_kernel
template <class W, bool STREAM>
__global__ __launch_bounds__(256) void native_pbs_init_kernel(W *__restrict__ acc, const W *__restrict__ lut, const uint32_t *__restrict__ rot,
                                                              uint32_t logn, uint32_t npolys, uint32_t lut_stride, size_t npoly_total) {
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;   // 16 bytes of any word type
    const uint32_t lv = logn - LOGV;
    const size_t total = npoly_total << lv, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t q = i >> lv, b = q / npolys, p = q - b * npolys;
        const uint32_t pos0 = (uint32_t)(i & (((size_t)1 << lv) - 1)) << LOGV;
        const uint32_t a = rot[b] & ((2u << logn) - 1u);
        const W *f = lut + ((b * lut_stride + p) << logn);
        union {
            W w[NV];
            V v;
        } d;
#pragma unroll
        for (int k = 0; k < NV; ++k) d.w[k] = gadget_source<W>(f, pos0 + (uint32_t)k, a, logn, false);
        V *dst = reinterpret_cast<V *>(acc + (q << logn) + pos0);
        if constexpr (STREAM) __builtin_nontemporal_store(d.v, dst);
        else *dst = d.v;
    }
}

// lwe_out[b][p n + j] = glwe[b][p][h - j], negated past the wrap (j > h) -- coefficient h of X^j glwe[b][p], the same gather -- and the
// body lwe_out[b][k n] = glwe[b][k][h].  One thread per output word (an element has k n + 1 of them: no 16-byte alignment to rely on).
template <class W>
__global__ __launch_bounds__(256) void native_sample_extract_kernel(W *__restrict__ lwe_out, const W *__restrict__ glwe, uint32_t logn,
                                                                    size_t glwe_dim, uint32_t h, size_t batch) {
    const size_t kn = glwe_dim << logn, row = kn + 1, total = batch * row, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t b = i / row, r = i - b * row;
        const W *g = glwe + ((b * (glwe_dim + 1)) << logn);
        if (r == kn) lwe_out[i] = g[kn + h];
        else lwe_out[i] = gadget_source<W>(g + ((r >> logn) << logn), h, (uint32_t)(r & (((size_t)1 << logn) - 1)), logn, false);
    }
}

// launchers (native_pbs.hip); word = 4, 8 or 16 bytes, grid from cntt_ew_grid, stream = the STREAM_BYTES policy decided by the caller
hipError_t launch_native_lwe_modswitch(int word, uint32_t *rot_t, const void *lwe, int logn, size_t lwe_dim, size_t batch, unsigned grid,
                                       hipStream_t st);
hipError_t launch_native_pbs_init(int word, void *acc, const void *lut, const uint32_t *rot, int logn, uint32_t npolys, bool per_element,
                                  size_t batch, bool stream, unsigned grid, hipStream_t st);
hipError_t launch_native_sample_extract(int word, void *lwe_out, const void *glwe, int logn, size_t glwe_dim, uint32_t index, size_t batch,
                                        unsigned grid, hipStream_t st);

}  // namespace cntt
