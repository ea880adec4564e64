// LWE keyswitch of the native / native_binary plans (include/cntt_keyswitch.h): a tiled wrapping integer GEMM on the VALU,
//     out[b][c] = (c == Lout ? in[b][Lin] : 0) - sum_{i < Lin} sum_{l = 1..levels} d_l(in[b][i]) ksk[(i levels + l - 1) row_stride + c]   mod 2^w
// with d_1 .. d_levels the signed digits of cntt_gadget.h.  The kernel is instantiated in native_keyswitch.hip; host_native_ext.hip sees
// the launcher only.
//
// Tiling.  A 256-thread workgroup owns BM = 4 TB batch elements x BN = 64 TC columns: wave v the batch elements v TB .. v TB + TB - 1,
// lane x the columns x, x + 64, ...  So a key load of a wave is 64 consecutive words of one key row (coalesced along c) and is used for
// the thread's TB batch elements; a digit is the same LDS word for all 64 lanes (a broadcast read) and is used for its TC columns.
// The Lin mask words are walked in chunks of KS_ROWS / levels words.  A chunk's words are loaded ONCE per workgroup, and their digits
// -- one add and one shift + mask per digit, the y = x + 2^(s-1) + K 2^s form of native_gadget.hpp -- are staged in LDS as 32-bit
// numbers (base_log <= 31); there is no digits buffer in memory.
//
// Unsigned digits.  The staged number is u = d + B/2 in [0, B), i.e. the bit field of y as it stands, so a multiply-accumulate is
// acc += u * k with a zero-extended 32-bit u: no sign fix-up on the 64- and 128-bit words.  The surplus (B/2) sum_r ksk[r][c] does not
// depend on the batch element: every thread sums the key words it loads anyway (TC adds per row beside TB TC multiply-accumulates)
// and the epilogue takes it off, together with the negation and the body:  out = body + (B/2) ksum - acc.
// Everything wraps modulo 2^w, so the order of the sums does not matter and the words are those of the header's formula.
#pragma once
#include "native_gadget.hpp"

namespace cntt {

constexpr int KS_ROWS = 128;   // digit rows (one per (word, level)) of one chunk in LDS; >= the largest `levels` (128: base_log 1, w 128)

// register tile of one thread: TB batch elements x TC columns
template <class W> struct KsTile {
    static constexpr int TB = 16, TC = 2;
};
template <> struct KsTile<Word128> {
    static constexpr int TB = 8, TC = 2;
};

// The accumulator of one (batch element, column) pair and acc += u * k modulo 2^w for a 32-bit unsigned u.
// u32 words: one v_mul_lo_u32, and one v_add3_u32 per two products.
template <class W> struct KsAcc {
    W v = 0;
    __device__ __forceinline__ void mad(uint32_t u, W k) { v += u * k; }
    __device__ __forceinline__ W value() const { return v; }
};
// u64 words: the low half of k into a 64-bit sum (one v_mad_u64_u32), the high half into a 32-bit sum of its own (as the u32 words),
// joined at the end -- 2.5 instructions per multiply-accumulate where acc += (uint64_t)u * k compiles to two v_mad_u64_u32 and two moves
template <> struct KsAcc<uint64_t> {
    uint64_t lo = 0;
    uint32_t hi = 0;
    __device__ __forceinline__ void mad(uint32_t u, uint64_t k) {
        lo += (uint64_t)u * (uint32_t)k;
        hi += u * (uint32_t)(k >> 32);
    }
    __device__ __forceinline__ uint64_t value() const { return lo + ((uint64_t)hi << 32); }
};
template <> struct KsAcc<Word128> {
    using A = unsigned __int128;
    A v = 0;
    __device__ __forceinline__ void mad(uint32_t u, Word128 k) { v += (A)u * (((A)k.hi << 64) | k.lo); }
    __device__ __forceinline__ Word128 value() const { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }
};
template <class W> __device__ __forceinline__ uint32_t ks_low32(W a) { return (uint32_t)a; }
template <> __device__ __forceinline__ uint32_t ks_low32<Word128>(Word128 a) { return (uint32_t)a.lo; }

// off = 2^(s-1) + K 2^s (gadget_offset of the host); row_stride >= lout + 1, in words; levels <= KS_ROWS, base_log <= 31.
// Grid-stride over the tiles, column tiles of one batch tile next to each other; every bound is checked per word.
template <class W>
__global__ __launch_bounds__(256) void native_keyswitch_kernel(W *__restrict__ out, const W *__restrict__ in, const W *__restrict__ ksk, W off,
                                                               uint32_t base_log, uint32_t levels, size_t lin, size_t lout,
                                                               size_t row_stride, size_t batch) {
    using O = WordOps<W>;
    constexpr int TB = KsTile<W>::TB, TC = KsTile<W>::TC, BM = 4 * TB, BN = 64 * TC;
    static_assert(TB % 4 == 0, "a thread reads its digits sixteen bytes at a time");
    __shared__ __attribute__((aligned(16))) uint32_t dig[KS_ROWS][BM];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t ncol = lout + 1, ct = (ncol + BN - 1) / BN, bt = (batch + BM - 1) / BM, tiles = ct * bt;
    const uint32_t kc = (uint32_t)KS_ROWS / levels;   // words per chunk
    const uint32_t mask = (1u << base_log) - 1u;
    for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const size_t c0 = (t % ct) * BN, b0 = (t / ct) * BM;
        KsAcc<W> acc[TB][TC];
        W ksum[TC];
        size_t col[TC];   // a column past the row reads the row's last word instead: loaded, summed, never stored
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            const size_t c = c0 + lane + 64u * (uint32_t)j;
            col[j] = c < ncol ? c : lout;
            ksum[j] = W{};
#pragma unroll
            for (int i = 0; i < TB; ++i) acc[i][j] = KsAcc<W>{};
        }
        for (size_t i0 = 0; i0 < lin; i0 += kc) {
            const uint32_t nw = lin - i0 < kc ? (uint32_t)(lin - i0) : kc;
            __syncthreads();   // the previous chunk's digits have been read
            for (uint32_t e = threadIdx.x; e < nw * BM; e += 256u) {
                const uint32_t ii = e / BM, bb = e % BM;
                const size_t b = b0 + bb;
                W y = W{};   // a batch element past the end: zero digits, never stored
                if (b < batch) y = O::add(in[b * (lin + 1) + i0 + ii], off);
                uint32_t sh = (uint32_t)O::BITS;
                for (uint32_t l = 0; l < levels; ++l) {
                    sh -= base_log;
                    dig[ii * levels + l][bb] = ks_low32<W>(O::shr(y, sh)) & mask;
                }
            }
            __syncthreads();
            const uint32_t nr = nw * levels;
            const W *krow = ksk + i0 * levels * row_stride;
#pragma unroll 2
            for (uint32_t rr = 0; rr < nr; ++rr, krow += row_stride) {
                W k[TC];
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
                    ksum[j] = O::add(ksum[j], k[j]);
#pragma unroll
                    for (int i = 0; i < TB; ++i) acc[i][j].mad(u[i], k[j]);
                }
            }
        }
        // out = body + (B/2) ksum - acc
        const uint32_t half = 1u << (base_log - 1u);
#pragma unroll
        for (int j = 0; j < TC; ++j) {
            const size_t c = c0 + lane + 64u * (uint32_t)j;
            if (c >= ncol) continue;
            KsAcc<W> surplus;
            surplus.mad(half, ksum[j]);
            const W corr = surplus.value();
#pragma unroll
            for (int i = 0; i < TB; ++i) {
                const size_t b = b0 + wave * TB + (uint32_t)i;
                if (b >= batch) continue;
                W v = O::sub(corr, acc[i][j].value());
                if (c == lout) v = O::add(v, in[b * (lin + 1) + lin]);
                out[b * ncol + c] = v;
            }
        }
    }
}

// launcher (native_keyswitch.hip); word = 4, 8 or 16 bytes; off_lo / off_hi = the two halves of gadget_offset (off_hi: 128-bit words)
hipError_t launch_native_keyswitch(int word, void *out, const void *in, const void *ksk, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                   unsigned levels, size_t lin, size_t lout, size_t row_stride, size_t batch, hipStream_t st);

}  // namespace cntt
