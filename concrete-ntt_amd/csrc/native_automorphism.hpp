// The ring automorphism X -> X^t of the native plans (include/cntt_automorphism.h), three kernels on the walk of prime_automorphism.hpp:
//     native_automorphism_kernel          out[j] = +-in[j t^-1 mod 2n] mod 2^w: the coefficient-domain map, gather form, W = u32 / u64 / Word128
//     native_automorphism_ntt_kernel      out[c] = in[c'] with 2 brev(c') + 1 = t (2 brev(c) + 1) mod 2n: the slot permutation of ONE residue
//                                         plane, R = u32 / u64 residues; it does not look at the words, so it serves every kind
//     native_automorphism_gadget_kernel   the hot one: per Galois keyswitch ONE pass over the input ciphertext that writes the k * levels
//                                         negated digit polynomials of the permuted mask polynomials and the prefilled output
// The external product after the third is host code (host_native_automorphism.inc) over native_ext_device.  The kernels are instantiated
// in native_automorphism.hip; host_native_ext.hip sees the launchers only.
//
// The walk.  One 256-thread workgroup per polynomial, grid-stride over the polynomials; a thread owns 16 bytes of consecutive destination
// coefficients (NV = 4 / 2 / 1 words) and takes the vectors tid, tid + 256, ... of its polynomial, so every store is a coalesced 16-byte
// one.  The sources of one vector are NV gathers: j -> u = j tinv mod 2n advances by tinv per coefficient.  No address depends on a data
// word.
//
// LDS (the compile-time switch).  With LDS = true the workgroup first stages the whole source polynomial into LDS with coalesced 16-byte
// loads -- possible while n sizeof(W) <= 64 KiB (NATIVE_AUTOM_LDS_BYTES): Word128 up to n = 4096, u64 up to 8192, u32 up to 16384 -- and
// gathers from there; with LDS = false the same code gathers from global memory, which is what larger polynomials always take.
// Bank pattern of the staged gather, from the banking rule of the part (64 banks of 4 bytes; a 4-byte read is banked mod 32 dwords in two
// 32-lane groups, an 8-byte read mod 64 dwords in two 32-lane groups, a 16-byte read mod 64 dwords in four 16-lane groups whose lane
// numbers cover every residue mod 16): word c of the vectors of consecutive lanes is NV * tinv words apart with tinv odd, i.e. always
// 4 * tinv dwords.  So
//     u32      the 32 lanes of a group fall on 32 / 4 = 8 bank positions:                      4-way conflict
//     u64      the 32 lanes of a group fall on 64 / 4 = 16 positions of two banks each:        2-way conflict
//     Word128  the 16 lanes of a group fall on 16 distinct slots of four banks each:           conflict-free
// (derived, not measured with a counter; the slot permutation's reads are bit-reversed and depend on t: not analysed).  This unit does not
// try to engineer the conflicts away.  Which form is faster where the polynomial is L2-resident either way is a measurement:
// profiles/r27_native_automorphism.txt.
//
// The digits are those of native_gadget_kernel (native_gadget.hpp) through the same WordOps and GadgetConst: y = sigma(x) + off, then per
// level the field (y >> sh) & mask; the kernel stores half - field, the NEGATED digit, as a wrapping w-bit word.  Neither the permuted
// polynomial nor the un-negated digits are ever stored.
#pragma once
#include <algorithm>

#include "native_gadget.hpp"

namespace cntt {

constexpr size_t NATIVE_AUTOM_LDS_BYTES = (size_t)64 << 10;   // the largest polynomial that is staged
constexpr unsigned NATIVE_AUTOM_CUS = 256;                      // CUs of the part the grid rule is written for
// Workgroups of the three kernels for `polys` polynomials of 2^logn words of word_bytes: one per polynomial up to what is resident at
// once -- 8 workgroups per CU (the 32-wave cap), fewer where the staged polynomial limits it (160 KiB of LDS per CU) -- and a grid-stride
// walk beyond.  The rule of prime_automorphism_grid: an ASSUMPTION about what fills the chip, not a measured optimum.
// cntt_native_automorphism_grid exports it (tests derive a second trip from it); it does not depend on the LDS switch.
inline unsigned native_automorphism_grid(size_t polys, int logn, size_t word_bytes) {
    const size_t bytes = word_bytes << logn;
    size_t per_cu = 8;
    if (bytes <= NATIVE_AUTOM_LDS_BYTES && bytes > 0) per_cu = std::min<size_t>(8, std::max<size_t>(1, ((size_t)160 << 10) / bytes));
    const size_t cap = per_cu * NATIVE_AUTOM_CUS;
    return (unsigned)(polys < 1 ? 1 : polys > cap ? cap : polys);
}

template <class W> struct NativeAutomVec {
    static constexpr int NV = 16 / (int)sizeof(W), LOGV = NV == 4 ? 2 : NV == 2 ? 1 : 0;
};

// stages polynomial f (n = 2^logn words, n * sizeof(W) <= NATIVE_AUTOM_LDS_BYTES) into LDS; the barrier before it protects the previous
// trip's reads
template <class W> __device__ __forceinline__ void native_autom_stage(W *lds, const W *__restrict__ f, uint32_t logn) {
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    const uint32_t nvec = 1u << (logn - (uint32_t)NativeAutomVec<W>::LOGV);
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < nvec; v += 256u) reinterpret_cast<V *>(lds)[v] = reinterpret_cast<const V *>(f)[v];
    __syncthreads();
}

// sigma_t(f)[j] for the running index u = j tinv mod 2n
template <class W> __device__ __forceinline__ W native_autom_word(const W *f, uint32_t u, uint32_t n) {
    return WordOps<W>::neg_if(f[u & (n - 1u)], (u & n) != 0);
}

// out[q] = sigma_t(in[q]) (NTT = false, tinv = t^-1 mod 2n) or the slot permutation (NTT = true, tinv is t itself) for q < npoly_total
template <class W, bool STREAM, bool LDS, bool NTT>
__device__ __forceinline__ void native_autom_walk(W *__restrict__ out, const W *__restrict__ in, uint32_t tinv, uint32_t logn, size_t npoly_total) {
    constexpr int NV = NativeAutomVec<W>::NV, LOGV = NativeAutomVec<W>::LOGV;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char native_autom_lds[];
    W *lds = reinterpret_cast<W *>(native_autom_lds);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - (uint32_t)LOGV);
    for (size_t q = blockIdx.x; q < npoly_total; q += gridDim.x) {
        const W *f = in + (q << logn);
        if constexpr (LDS) native_autom_stage<W>(lds, f, logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            union {
                W w[NV];
                V v;
            } d;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const uint32_t j = j0 + (uint32_t)c;
                if constexpr (NTT) {
                    const uint32_t e = (tinv * (2u * (__brev(j) >> (32u - logn)) + 1u)) & m2n;   // odd
                    const uint32_t s = __brev(e >> 1) >> (32u - logn);
                    if constexpr (LDS) d.w[c] = lds[s];
                    else d.w[c] = f[s];
                } else {
                    const uint32_t u = (j * tinv) & m2n;
                    if constexpr (LDS) d.w[c] = native_autom_word<W>(lds, u, n);
                    else d.w[c] = native_autom_word<W>(f, u, n);
                }
            }
            V *dst = reinterpret_cast<V *>(out + (q << logn) + j0);
            if constexpr (STREAM) __builtin_nontemporal_store(d.v, dst);
            else *dst = d.v;
        }
    }
}

template <class W, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void native_automorphism_kernel(W *__restrict__ out, const W *__restrict__ in, uint32_t tinv, uint32_t logn,
                                                                  size_t npoly_total) {
    native_autom_walk<W, STREAM, LDS, false>(out, in, tinv, logn, npoly_total);
}
template <class R, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void native_automorphism_ntt_kernel(R *__restrict__ out, const R *__restrict__ in, uint32_t t, uint32_t logn,
                                                                      size_t npoly_total) {
    native_autom_walk<R, STREAM, LDS, true>(out, in, t, logn, npoly_total);
}

// in, out: batch x (k + 1) polynomials; terms: batch x k * levels polynomials.  Polynomial (b, q):
//   q < k   terms[b][q levels + l - 1] = -d_l(sigma_t(in[b][q])) mod 2^w,   out[b][q] = add ? in[b][q] : 0
//   q = k   out[b][k] = sigma_t(in[b][k]) (+ in[b][k] mod 2^w when add)
// STREAM: the digit polynomials are larger than STREAM_BYTES and pass through once (the output keeps the default policy: the external
// product reads it back next).  G: off, mask, half, base_log and levels are read; the source fields of GadgetConst are not.
template <class W, bool STREAM, bool LDS>
__global__ __launch_bounds__(256) void native_automorphism_gadget_kernel(W *__restrict__ terms, W *__restrict__ out, const W *__restrict__ in,
                                                                         const GadgetConst<W> G, uint32_t tinv, uint32_t logn, uint32_t k,
                                                                         uint32_t add, size_t batch) {
    using O = WordOps<W>;
    constexpr int NV = NativeAutomVec<W>::NV, LOGV = NativeAutomVec<W>::LOGV;
    using V = __attribute__((ext_vector_type(4))) uint32_t;
    extern __shared__ __attribute__((aligned(16))) unsigned char native_autom_lds[];
    W *lds = reinterpret_cast<W *>(native_autom_lds);
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, nvec = 1u << (logn - (uint32_t)LOGV);
    const size_t npoly_total = batch * ((size_t)k + 1);
    for (size_t i = blockIdx.x; i < npoly_total; i += gridDim.x) {
        const size_t b = i / (k + 1u);
        const uint32_t q = (uint32_t)(i - b * (k + 1u));
        const W *f = in + (i << logn);
        if constexpr (LDS) native_autom_stage<W>(lds, f, logn);
        for (uint32_t v = threadIdx.x; v < nvec; v += 256u) {
            const uint32_t j0 = v << LOGV;
            W x[NV];
            union {
                W w[NV];
                V v;
            } d, own;
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const uint32_t u = ((j0 + (uint32_t)c) * tinv) & m2n;
                if constexpr (LDS) x[c] = native_autom_word<W>(lds, u, n);
                else x[c] = native_autom_word<W>(f, u, n);
            }
            if (add) {
                if constexpr (LDS) own.v = reinterpret_cast<const V *>(lds)[v];
                else own.v = reinterpret_cast<const V *>(f)[v];
            } else {
                own.v = V{0u, 0u, 0u, 0u};
            }
            V *o = reinterpret_cast<V *>(out + (i << logn) + j0);
            if (q == k) {   // (the same for the whole workgroup) the body: sigma_t(in) (+ in)
#pragma unroll
                for (int c = 0; c < NV; ++c) d.w[c] = O::add(x[c], own.w[c]);
                *o = d.v;
                continue;
            }
            *o = own.v;
            W *dst = terms + (((b * k + q) * G.levels) << logn) + j0;
#pragma unroll
            for (int c = 0; c < NV; ++c) x[c] = O::add(x[c], G.off);   // y
            uint32_t sh = (uint32_t)O::BITS;
            for (uint32_t l = 0; l < G.levels; ++l, dst += (size_t)1 << logn) {
                sh -= G.base_log;
#pragma unroll
                for (int c = 0; c < NV; ++c) d.w[c] = O::sub(G.half, O::band(O::shr(x[c], sh), G.mask));   // -(field - half)
                if constexpr (STREAM) __builtin_nontemporal_store(d.v, reinterpret_cast<V *>(dst));
                else *reinterpret_cast<V *>(dst) = d.v;
            }
        }
    }
}

// launchers (native_automorphism.hip).  word = 4 / 8 / 16 bytes (the ntt form: the residue, 4 / 8); lds: stage through LDS where the
// polynomial fits (the caller's wish; the launcher falls back to the global gather above NATIVE_AUTOM_LDS_BYTES); stream: the STREAM_BYTES
// policy decided by the caller; off = the word gadget_offset gives (host_native_ext.hip), in two halves
hipError_t launch_native_automorphism(int word, void *out, const void *in, uint32_t t, bool ntt, int logn, size_t npoly_total, bool stream,
                                      bool lds, hipStream_t st);
hipError_t launch_native_automorphism_gadget(int word, void *terms, void *out, const void *in, uint64_t off_lo, uint64_t off_hi,
                                             unsigned base_log, unsigned levels, uint32_t t, int logn, size_t glwe_dim, bool add_input,
                                             size_t batch, bool stream, bool lds, hipStream_t st);

}  // namespace cntt
