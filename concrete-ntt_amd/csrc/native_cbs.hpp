// The circuit bootstrap of the native plans (include/cntt_cbs.h): LWE encryptions of bits in, the words of GGSW selectors out.  Four
// kernels around the unchanged blind rotation (blind_rotate_device of pbs_host.hpp), E = batch * cbs_levels bootstrap elements, element
// e = b * cbs_levels + (l - 1); the words W are u32 / u64 / Word128, the residue kinds never enter:
//     native_cbs_setup_kernel     one launch: the rot_t rows of the E elements (ms() of lwe_in[b] with 2^(w - 2) added to the body, the
//                                 body row negated, replicated over the levels) and the E per-element tables, trivial GLWE ciphertexts
//                                 whose body is the constant 2^w - H_l
//     native_cbs_extract_kernel   reads the E accumulators once: sample extraction at index 0 and + H_l on the body in registers, then the
//                                 R = (k n + 1) ks_levels signed digits of every word as int32.  The LWE ciphertexts u are never stored.
//     native_cbs_ks_kernel        the hot one, the functional keyswitch as a product: per key q an E x R matrix of int32 digits times an
//                                 R x (k + 1) n matrix of PLAIN key words, cut into slabs of rows; every slab sum is one wrapping word
//     native_cbs_sum_kernel       adds the slabs mod 2^w, negates, stores the selector words in the selector layout
// The split into residues and the forward transforms that follow are host code (host_native_cbs.inc) over native_split_device and
// native_ntt_device.  The kernels are instantiated in native_cbs.hip; host_native_ext.hip sees the launchers only.
//
// The digits are those of native_gadget_kernel (native_gadget.hpp) through the same WordOps and GadgetConst: y = x + off, then per level
// ((y >> sh) & mask) - half; ks_base_log <= 31, so a digit lies in [-2^30, 2^30) and its low 32 bits are the int32.
//
// The product, on the layout of prime_cbs_ks_kernel (prime_cbs.hpp).  A 256-thread workgroup owns NCBS_ET = 8 elements x 256 vectors of 16
// bytes of consecutive key columns x one slab of rows of one key.  A thread keeps ONE wrapping word per (element, slot) in registers --
// 8 x 16 bytes = 32 VGPRs for every word width -- and reads every key word of its columns once for the eight elements.  The digit is the
// same for the whole workgroup: the tile's digits are parked in LDS, NCBS_CH rows at a time, as [row][element], every lane reads the same
// 32 bytes (a broadcast, no bank conflict) and __builtin_amdgcn_readfirstlane moves the digit to a scalar register, so the sign test is
// a scalar branch and the multiplier |d| <= 2^30 a scalar operand.  Mod 2^w the sum needs no wide accumulator and no reduction:
//   32-bit words: acc += d w is one v_mad_u32 (the two's complement of d multiplies as it is).
//   64-bit words: |d| w mod 2^64 = mad_u64_u32(|d|, lo(w)) + ((|d| hi(w)) << 32), added or subtracted.
//   128-bit words: four 32-bit limbs, |d| w mod 2^128 as a carry chain of mad_u64_u32, added or subtracted.
// Slabs exist because at k = 1, n = 1024 a key has 4096 columns = 8 workgroups per E-tile on 64-bit words: too few to pull HBM
// bandwidth.  The sums are exact mod 2^w, so the result does not depend on the slab count.  No atomics.
#pragma once
#include "native_gadget.hpp"

namespace cntt {

constexpr unsigned NCBS_CUS = 256;        // CUs of the part the grid rule is written for
constexpr unsigned NCBS_ET = 8;           // elements of one tile of the product
constexpr unsigned NCBS_CH = 128;         // rows of digits parked in LDS at a time
constexpr unsigned NCBS_SLAB_MIN = 64;    // a slab has at least this many rows (the last one may have fewer)

// Workgroups of native_cbs_ks_kernel for `items` work items (key x E-tile x column block x slab): one per item up to 8 per CU, a
// grid-stride walk beyond.  An ASSUMPTION carried over from prime_cbs_grid, not a measured optimum.  cntt_native_cbs_grid exports it.
inline unsigned native_cbs_grid(size_t items, int /*logn*/, size_t /*word_bytes*/) {
    const size_t cap = (size_t)8 * NCBS_CUS;
    return (unsigned)(items < 1 ? 1 : items > cap ? cap : items);
}

// the shape of the product: column blocks per key, E-tiles, rows per slab, slabs (the header states the rule: that of prime_cbs_shape)
struct NativeCbsShape {
    size_t cols, tiles, rows, slabs;
    __host__ __device__ size_t items(size_t k) const { return (k + 1) * cols * tiles * slabs; }
};
inline NativeCbsShape native_cbs_shape(size_t n, size_t word_bytes, size_t k, size_t r, size_t e) {
    const size_t cap = (size_t)8 * NCBS_CUS, per_block = 256 * (16 / word_bytes);
    NativeCbsShape s;
    s.cols = ((k + 1) * n + per_block - 1) / per_block;
    s.tiles = (e + NCBS_ET - 1) / NCBS_ET;
    const size_t base = (k + 1) * s.cols * (s.tiles ? s.tiles : 1);
    size_t s0 = cap / base;                                              // slabs that still fit one trip of the grid
    const size_t most = (r + NCBS_SLAB_MIN - 1) / NCBS_SLAB_MIN;
    s0 = s0 > most ? most : s0;
    s0 = s0 < 1 ? 1 : s0;
    s.rows = (r + s0 - 1) / s0;
    s.slabs = (r + s.rows - 1) / s.rows;
    return s;
}

// constants of the set-up and the extraction kernel
struct NativeCbsConst {
    uint32_t logn, k, cbs_base_log, cbs_levels;
};

// 2^sh as a word, sh below the word width
template <class W> __host__ __device__ __forceinline__ W native_cbs_pow2(uint32_t sh) { return (W)((W)1 << sh); }
template <> __host__ __device__ __forceinline__ Word128 native_cbs_pow2<Word128>(uint32_t sh) {
    return sh >= 64 ? Word128{0, (uint64_t)1 << (sh - 64)} : Word128{(uint64_t)1 << sh, 0};
}
// H_l = 2^(w - cbs_base_log l - 1): cbs_base_log * cbs_levels <= w - 1 keeps the exponent at 0 or above
template <class W> __device__ __forceinline__ W native_cbs_h(uint32_t base_log, uint32_t l) {
    return native_cbs_pow2<W>((uint32_t)WordOps<W>::BITS - base_log * l - 1u);
}
template <class W> __device__ __forceinline__ W native_cbs_zero() { return (W)0; }
template <> __device__ __forceinline__ Word128 native_cbs_zero<Word128>() { return Word128{0, 0}; }
template <class W> __device__ __forceinline__ uint32_t native_cbs_low32(W x) { return (uint32_t)x; }
template <> __device__ __forceinline__ uint32_t native_cbs_low32<Word128>(Word128 x) { return (uint32_t)x.lo; }
// the top 32 bits of a word
template <class W> __device__ __forceinline__ uint32_t native_cbs_top32(W x);
template <> __device__ __forceinline__ uint32_t native_cbs_top32<uint32_t>(uint32_t x) { return x; }
template <> __device__ __forceinline__ uint32_t native_cbs_top32<uint64_t>(uint64_t x) { return (uint32_t)(x >> 32); }
template <> __device__ __forceinline__ uint32_t native_cbs_top32<Word128>(Word128 x) { return (uint32_t)(x.hi >> 32); }

// rot_t: (L + 1) x E uint32, rot_t[i E + e] = ms(lwe'[b][i]) with ms() of native_lwe_modswitch_kernel (native_pbs.hpp), the body row negated
// mod 2n.  lwe' = lwe with 2^(w - 2) added to the body: ms() reads the top 32 bits only, and 2^(w - 2) is bit 30 of them, so the word is
// never formed.  table: E x (k + 1) polynomials, masks zero, the body polynomial the constant 2^w - H_l.  One grid-stride walk over the
// (L + 1) E exponents and then the table's 16-byte vectors.
template <class W>
__global__ __launch_bounds__(256) void native_cbs_setup_kernel(uint32_t *__restrict__ rot_t, W *__restrict__ table, const W *__restrict__ lwe,
                                                               const NativeCbsConst C, size_t lwe_dim, size_t elements) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const size_t nrot = (lwe_dim + 1) * elements, nvec = (elements * (C.k + 1u)) << (C.logn - LOGV);
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint32_t sh = 32u - C.logn - 2u, mask = (2u << C.logn) - 1u;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nrot + nvec; t += stride) {
        if (t < nrot) {
            const size_t i = t / elements, e = t - i * elements, b = e / C.cbs_levels;
            uint32_t top = native_cbs_top32<W>(lwe[b * (lwe_dim + 1) + i]);
            if (i == lwe_dim) top += 1u << 30;
            uint32_t m = (((top >> sh) + 1u) >> 1) & mask;
            if (i == lwe_dim) m = (0u - m) & mask;
            rot_t[t] = m;
        } else {
            const size_t v = t - nrot, poly = v >> (C.logn - LOGV), e = poly / (C.k + 1u);
            const uint32_t q = (uint32_t)(poly - e * (C.k + 1u)), l = (uint32_t)(e % C.cbs_levels) + 1u;
            const W c = q == C.k ? O::sub(native_cbs_zero<W>(), native_cbs_h<W>(C.cbs_base_log, l)) : native_cbs_zero<W>();
            union {
                W w[NV];
                V v;
            } d;
#pragma unroll
            for (int j = 0; j < NV; ++j) d.w[j] = c;
            reinterpret_cast<V *>(table)[v] = d.v;
        }
    }
}

// digits[e R + i Lk + j - 1] = d_j(u[e][i]) for i <= Lin = k n, where u[e] is the sample extraction at index 0 of acc[e]
// (native_sample_extract_kernel: gadget_source with h = 0) with H_l added to the body.  One thread per word of u.  G: off, mask, half,
// base_log and levels are read (base_log <= 31).
template <class W>
__global__ __launch_bounds__(256) void native_cbs_extract_kernel(int32_t *__restrict__ digits, const W *__restrict__ acc, const GadgetConst<W> G,
                                                                 const NativeCbsConst C, size_t elements) {
    using O = WordOps<W>;
    const size_t lin = (size_t)C.k << C.logn, row = lin + 1, total = elements * row;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const size_t e = t / row, i = t - e * row;
        const W *g = acc + ((e * (C.k + 1u)) << C.logn);
        W x;
        if (i == lin) x = O::add(g[lin], native_cbs_h<W>(C.cbs_base_log, (uint32_t)(e % C.cbs_levels) + 1u));
        else x = gadget_source<W>(g + ((i >> C.logn) << C.logn), 0u, (uint32_t)(i & (((size_t)1 << C.logn) - 1)), C.logn, false);
        const W y = O::add(x, G.off);
        int32_t *dst = digits + t * G.levels;
        uint32_t sh = (uint32_t)O::BITS;
        for (uint32_t l = 0; l < G.levels; ++l) {
            sh -= G.base_log;
            dst[l] = (int32_t)(native_cbs_low32<W>(O::band(O::shr(y, sh), G.mask)) - native_cbs_low32<W>(G.half));
        }
    }
}

// the accumulator of one (element, slot): one wrapping word.  add(m, w, neg): acc +- m w mod 2^w for the magnitude m <= 2^30 of a digit
template <class W> struct NativeCbsAcc;
template <> struct NativeCbsAcc<uint32_t> {
    uint32_t a;
    __device__ __forceinline__ void zero() { a = 0; }
    __device__ __forceinline__ void add(uint32_t m, uint32_t w, bool neg) { a = neg ? a - m * w : a + m * w; }
    __device__ __forceinline__ uint32_t value() const { return a; }
};
template <> struct NativeCbsAcc<uint64_t> {
    uint64_t a;
    __device__ __forceinline__ void zero() { a = 0; }
    __device__ __forceinline__ void add(uint32_t m, uint64_t w, bool neg) {
        const uint64_t pr = (uint64_t)m * (uint32_t)w + ((uint64_t)(m * (uint32_t)(w >> 32)) << 32);
        a = neg ? a - pr : a + pr;
    }
    __device__ __forceinline__ uint64_t value() const { return a; }
};
template <> struct NativeCbsAcc<Word128> {
    unsigned __int128 a;
    __device__ __forceinline__ void zero() { a = 0; }
    __device__ __forceinline__ void add(uint32_t m, Word128 w, bool neg) {
        // limbs w0 .. w3 of 32 bits: m w mod 2^128 = m w0 + (m w1 << 32) + (m w2 << 64) + (lo32(m w3) << 96)
        const uint64_t p0 = (uint64_t)m * (uint32_t)w.lo, p1 = (uint64_t)m * (uint32_t)(w.lo >> 32) + (p0 >> 32);
        const uint64_t p2 = (uint64_t)m * (uint32_t)w.hi + (p1 >> 32);
        const uint32_t p3 = m * (uint32_t)(w.hi >> 32) + (uint32_t)(p2 >> 32);
        const uint64_t lo = ((uint64_t)(uint32_t)p1 << 32) | (uint32_t)p0, hi = ((uint64_t)p3 << 32) | (uint32_t)p2;
        const unsigned __int128 pr = ((unsigned __int128)hi << 64) | lo;
        a = neg ? a - pr : a + pr;
    }
    __device__ __forceinline__ Word128 value() const { return Word128{(uint64_t)a, (uint64_t)(a >> 64)}; }
};

// part[((s (k + 1) + q) E + e) C + col] = sum over the rows r of slab s of digits[e R + r] * key[(q R + r) C + col] mod 2^w, C = (k + 1) n
// columns.  Work item = (slab, key, E-tile, column block), the column blocks of one (slab, key, tile) next to each other; grid-stride.
// Every bound is checked: rows past R and elements past E take the digit 0 and are not stored, vectors past C are neither read nor stored.
template <class W>
__global__ __launch_bounds__(256) void native_cbs_ks_kernel(W *__restrict__ part, const int32_t *__restrict__ digits, const W *__restrict__ key,
                                                            uint32_t logn, uint32_t k, size_t rows_total, size_t elements, NativeCbsShape Z) {
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    __shared__ __attribute__((aligned(16))) int32_t dig[NCBS_CH][NCBS_ET];
    const size_t cvec = ((size_t)(k + 1u) << logn) >> LOGV;   // 16-byte vectors of one key row
    const size_t items = Z.items(k);
    for (size_t it = blockIdx.x; it < items; it += gridDim.x) {
        const size_t cb = it % Z.cols, t1 = it / Z.cols, tile = t1 % Z.tiles, t2 = t1 / Z.tiles, q = t2 % (k + 1u), slab = t2 / (k + 1u);
        const size_t e0 = tile * NCBS_ET, r0 = slab * Z.rows, r1 = r0 + Z.rows < rows_total ? r0 + Z.rows : rows_total;
        const size_t v = cb * 256 + threadIdx.x;
        const bool live = v < cvec;
        const V *kq = reinterpret_cast<const V *>(key) + q * rows_total * cvec + v;
        NativeCbsAcc<W> acc[NCBS_ET][NV];
#pragma unroll
        for (unsigned e = 0; e < NCBS_ET; ++e)
#pragma unroll
            for (int j = 0; j < NV; ++j) acc[e][j].zero();
        for (size_t rc = r0; rc < r1; rc += NCBS_CH) {
            const uint32_t nr = (uint32_t)(r1 - rc < NCBS_CH ? r1 - rc : NCBS_CH);
            __syncthreads();   // the chunk before has been read
            for (uint32_t x = threadIdx.x; x < NCBS_CH * NCBS_ET; x += 256u) {
                const uint32_t rr = x % NCBS_CH, ee = x / NCBS_CH;
                dig[rr][ee] = rr < nr && e0 + ee < elements ? digits[(e0 + ee) * rows_total + rc + rr] : 0;
            }
            __syncthreads();
            if (live) {
                for (uint32_t rr = 0; rr < nr; ++rr) {
                    union {
                        W w[NV];
                        V v;
                    } kw;
                    kw.v = kq[(rc + rr) * cvec];
#pragma unroll
                    for (unsigned e = 0; e < NCBS_ET; ++e) {
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
            for (unsigned e = 0; e < NCBS_ET; ++e) {
                if (e0 + e >= elements) break;
                union {
                    W w[NV];
                    V v;
                } o;
#pragma unroll
                for (int j = 0; j < NV; ++j) o.w[j] = acc[e][j].value();
                reinterpret_cast<V *>(part)[((slab * (k + 1u) + q) * elements + e0 + e) * cvec + v] = o.v;
            }
        }
    }
}

// sel[b][(q Lc + l - 1) (k + 1) + o][c] = -sum_s part[s][q][e][o n + c] mod 2^w, e = b Lc + l - 1: one thread per 16 bytes, grid-stride
template <class W>
__global__ __launch_bounds__(256) void native_cbs_sum_kernel(W *__restrict__ sel, const W *__restrict__ part, uint32_t logn, uint32_t k,
                                                             uint32_t cbs_levels, size_t elements, size_t slabs) {
    using O = WordOps<W>;
    constexpr int NV = 16 / sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const size_t cvec = ((size_t)(k + 1u) << logn) >> LOGV, per_slab = (k + 1u) * elements * cvec;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < per_slab; t += stride) {
        const size_t v = t % cvec, qe = t / cvec, e = qe % elements, q = qe / elements, b = e / cbs_levels, l1 = e - b * cbs_levels;
        union {
            W w[NV];
            V v;
        } s, a;
        s.v = reinterpret_cast<const V *>(part)[t];
        for (size_t i = 1; i < slabs; ++i) {
            a.v = reinterpret_cast<const V *>(part)[i * per_slab + t];
#pragma unroll
            for (int j = 0; j < NV; ++j) s.w[j] = O::add(s.w[j], a.w[j]);
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) s.w[j] = O::sub(native_cbs_zero<W>(), s.w[j]);
        reinterpret_cast<V *>(sel)[((b * (k + 1u) + q) * cbs_levels + l1) * cvec + v] = s.v;
    }
}

// launchers (native_cbs.hip): word = 4 / 8 / 16 bytes; off = the word gadget_offset gives (host_native_ext.hip), in two halves
hipError_t launch_native_cbs_setup(int word, uint32_t *rot_t, void *table, const void *lwe, const NativeCbsConst &C, size_t lwe_dim,
                                   size_t elements, unsigned grid, hipStream_t st);
hipError_t launch_native_cbs_extract(int word, int32_t *digits, const void *acc, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                     unsigned levels, const NativeCbsConst &C, size_t elements, unsigned grid, hipStream_t st);
hipError_t launch_native_cbs_ks(int word, void *part, const int32_t *digits, const void *key, int logn, size_t glwe_dim, size_t rows,
                                size_t elements, const NativeCbsShape &Z, hipStream_t st);
hipError_t launch_native_cbs_sum(int word, void *sel, const void *part, int logn, size_t glwe_dim, unsigned cbs_levels, size_t elements,
                                 size_t slabs, unsigned grid, hipStream_t st);

}  // namespace cntt
