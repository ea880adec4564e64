// The multi-bit blind rotation of the native plans (include/cntt_multibit.h): one group of g mask words is absorbed by ONE external product
// against a key bundled from 2^g GGSW ciphertexts, per residue prime of the plan.  As in prime_multibit.hpp the bundle is never formed: in
// the NTT domain of prime P_i the monomial is a pointwise factor, so per prime i, element b, output o and word c
//     out_i[b][o][c] = sum_{t < 2^g} M_i(e_t(b))[c] * ( sum_{j < nterms} terms_i[b][j][c] * key_i[t][j][o][c] )   mod P_i, canonical
// which is native_multibit_accumulate_kernel, the only kernel of this file.  Digits, residue split, transforms and CRT around it are the
// stand-alone ones; the loop is host code (multibit_host.hpp; its step: host_native_multibit.inc).  Instantiated in native_multibit.hip.  Plan32 kinds only: the
// residues are 32-bit words of the ten primes PRIMES32 (host_common.hpp), all below 2^30.
//
// It differs from prime_multibit_accumulate_kernel<uint32_t> in three ways.
//
// 1. All residue planes in one launch.  The plane is the y coordinate of the workgroup, so it is part of the work index and uniform in a
//    wave: the per-prime constants (P_i, -P_i^-1 mod 2^32, the plane pointers, the table pointer) are passed by value in MultibitPlanes and
//    read with scalar loads at a uniform index -- no private copy of the struct.  The subset-sum exponents e_t and the factor
//    2 bitrev(c) + 1 do not depend on the prime: there is one form of them, computed once per work item before the pattern loop, and
//    nothing per-prime enters them.  A native64 group step makes one pointwise launch where five prime launches would.
//
// 2. Lazy inner sum.  Transform outputs and key residues are canonical (include/cntt.h: "Every output is canonical"), so with P < 2^30
//        x y <= (P - 1)^2 < 2^60,      the sum of FOUR products  < 4 P^2 = (4 P) P < 2^32 P          (4 P < 2^32  <=>  P < 2^30)
//    and w < 2^32 P is the input range of one Montgomery reduction with R = 2^32:  m = (w mod R)(-P^-1) mod R,  u = (w + m P) / R <
//    (2^32 P + 2^32 P) / 2^32 = 2 P, one conditional subtraction makes it canonical, u = w R^-1 mod P.  So four products are summed in one
//    64-bit register (a 32 x 32 + 64 multiply-add each, no reduction), reduced ONCE, and added into a 32-bit running sum with one
//    conditional subtraction; the prime kernel pays a full mont_mul and an add_mod per term.  The chunk is four and no wider: five
//    products reach 5 P^2 > 2^32 P for P > 2^32 / 5, which every prime here is.  MULTIBIT_LAZY_TERMS and the static_assert below tie the
//    chunk to the bound, and the host asserts the bound for every prime of PRIMES32 (host_native_multibit.inc).
//    A ragged tail of 1 ... 3 products is the same sum with fewer terms.
//
// 3. Normalisation folded into the table.  tab_i[m] = psi_i^m n^-1 R^2 mod P_i for m < n.  A chunk's reduction leaves R^-1 on the inner sum
//    and the Montgomery product with the table word another one; the table's R^2 takes both off and its n^-1 is the factor that
//    mul_assign_normalize would leave: the stand-alone (unnormalised) inverse transform of the output is then the canonical residue of the
//    step's coefficient, and cntt_native_inv_batch on the output planes gives the coefficient-domain words.  The table's words are never 0,
//    so -x = P - x.
//
// The monomial, as in prime_multibit.hpp: M(e)[c] = +-psi^(m mod n), m = e (2 bitrev_logn(c) + 1) mod 2n, minus when m >= n (psi^n = -1).
// Loop order (pattern t outermost, one running sum per thread), the thread-to-vector mapping (one thread owns one 16-byte vector of one
// (b, o) output polynomial of one plane) and the grid-stride loop with a capped grid are those of the prime kernel; see there for what
// was and was not A/B-tested.
#pragma once
#include "ntt_arith.hpp"

namespace cntt {

constexpr unsigned NATIVE_MULTIBIT_MAX_GROUPING = 4;
constexpr unsigned NATIVE_MULTIBIT_MAX_PLANES = 10;
// every prime the kernel can meet is below this (host_native_multibit.inc asserts it for PRIMES32)
constexpr uint32_t NATIVE_MULTIBIT_PRIME_BOUND = 1u << 30;
// products summed between two reductions: MULTIBIT_LAZY_TERMS P^2 < 2^32 P must hold for every P below the bound
constexpr unsigned MULTIBIT_LAZY_TERMS = 4;
static_assert((uint64_t)MULTIBIT_LAZY_TERMS * NATIVE_MULTIBIT_PRIME_BOUND <= ((uint64_t)1 << 32),
              "the lazy chunk leaves the input range of one Montgomery reduction");

// The grid: x = 256 threads per 256 vectors of ONE plane's output, at most this many workgroups per plane and a grid-stride loop beyond;
// y = the planes.  512 per plane keeps a native64 launch (five planes) near the 2048 workgroups of the prime kernel -- the same
// ASSUMPTION about what fills the chip, not a measured optimum.  cntt_native_multibit_grid exports the rule (tests derive a second trip
// from it).
constexpr unsigned NATIVE_MULTIBIT_MAX_BLOCKS = 512;
inline unsigned native_multibit_grid(size_t vectors) {
    const size_t blocks = (vectors + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > NATIVE_MULTIBIT_MAX_BLOCKS ? NATIVE_MULTIBIT_MAX_BLOCKS : blocks);
}

// per-prime constants and planes, by value (as KeyPlanes / FusedTables are): plane i at index i
struct MultibitPlanes {
    uint32_t *out[NATIVE_MULTIBIT_MAX_PLANES];           // batch x nout residue polynomials, written only
    const uint32_t *terms[NATIVE_MULTIBIT_MAX_PLANES];   // batch x nterms, forward-transformed, canonical
    const uint32_t *key[NATIVE_MULTIBIT_MAX_PLANES];     // 2^g x nterms x nout, pattern-major, canonical
    const uint32_t *tab[NATIVE_MULTIBIT_MAX_PLANES];     // psi^m n^-1 R^2 mod P, m < n (R = 2^32)
    uint32_t p[NATIVE_MULTIBIT_MAX_PLANES], pinv_neg[NATIVE_MULTIBIT_MAX_PLANES];
};

// w R^-1 mod P, canonical, for w < 2^32 P (R = 2^32): the low words of w and m P cancel, their carry is (low(w) != 0)
__device__ __forceinline__ uint32_t multibit_redc(uint64_t w, uint32_t p, uint32_t pinv_neg) {
    const uint32_t m = (uint32_t)w * pinv_neg;
    const uint32_t u = (uint32_t)(w >> 32) + __umulhi(m, p) + ((uint32_t)w != 0u);   // < 2 P < 2^31
    return u >= p ? u - p : u;
}

// rot_rows: g rows of `batch` exponents (taken mod 2n).  n = 2^logn >= 32.  gridDim.y = the planes.  No output plane may overlap an input.
// R: the residue word, uint32_t -- a template so that the one instance lives in native_multibit.hip, the unit that launches it.
template <class R>
__global__ __launch_bounds__(256) void native_multibit_accumulate_kernel(MultibitPlanes A, const uint32_t *__restrict__ rot_rows,
                                                                         uint32_t logn, uint32_t nterms, uint32_t nout, uint32_t g,
                                                                         size_t batch) {
    static_assert(sizeof(R) == 4, "residues of the Plan32 kinds are 32-bit words");
    constexpr int NV = 4, LOGV = 2;
    using V = __attribute__((ext_vector_type(NV))) uint32_t;
    const uint32_t plane = blockIdx.y;   // uniform: the loads below are scalar
    const uint32_t p = A.p[plane], pinv_neg = A.pinv_neg[plane];
    const uint32_t *__restrict__ tab = A.tab[plane];
    const V *__restrict__ terms = reinterpret_cast<const V *>(A.terms[plane]);
    const V *__restrict__ key = reinterpret_cast<const V *>(A.key[plane]);
    V *__restrict__ out = reinterpret_cast<V *>(A.out[plane]);
    const uint32_t lv = logn - LOGV;   // log2 vectors per polynomial
    const uint32_t n = 1u << logn, m2n = 2u * n - 1u, npat = 1u << g;
    const size_t total = (batch * nout) << lv, stride = (size_t)gridDim.x * blockDim.x;
    const size_t kstep = (size_t)nout << lv;   // vectors from key[t][j][o] to key[t][j + 1][o]
    const uint32_t nfull = nterms & ~(MULTIBIT_LAZY_TERMS - 1u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i & (((size_t)1 << lv) - 1), bo = i >> lv;
        const size_t b = bo / nout, o = bo - b * nout;
        // prime-independent: the group's exponents and 2 bitrev(c) + 1 of the four words, once per work item
        uint32_t a[NATIVE_MULTIBIT_MAX_GROUPING], idx[NV];
#pragma unroll
        for (uint32_t q = 0; q < NATIVE_MULTIBIT_MAX_GROUPING; ++q) a[q] = q < g ? rot_rows[(size_t)q * batch + b] & m2n : 0u;
#pragma unroll
        for (int k = 0; k < NV; ++k) idx[k] = 2u * (__brev(((uint32_t)v << LOGV) + (uint32_t)k) >> (32u - logn)) + 1u;
        const V *tv = terms + ((b * nterms) << lv) + v;
        const V *kv = key + (o << lv) + v;
        V acc;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[k] = 0;
        for (uint32_t t = 0; t < npat; ++t) {
            uint32_t e = 0;
#pragma unroll
            for (uint32_t q = 0; q < NATIVE_MULTIBIT_MAX_GROUPING; ++q) e += (t >> q) & 1u ? a[q] : 0u;
            V s;
#pragma unroll
            for (int k = 0; k < NV; ++k) s[k] = 0;
            uint32_t j = 0;
            for (; j < nfull; j += MULTIBIT_LAZY_TERMS) {   // four products, one reduction
                uint64_t w[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) w[k] = 0;
#pragma unroll
                for (uint32_t u = 0; u < MULTIBIT_LAZY_TERMS; ++u) {
                    const V x = tv[(size_t)(j + u) << lv];
                    const V y = kv[(size_t)(j + u) * kstep];
#pragma unroll
                    for (int k = 0; k < NV; ++k) w[k] += (uint64_t)x[k] * y[k];
                }
#pragma unroll
                for (int k = 0; k < NV; ++k) s[k] = add_mod<uint32_t>(s[k], multibit_redc(w[k], p, pinv_neg), p);
            }
            if (j < nterms) {   // the ragged tail: 1 ... 3 products
                uint64_t w[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) w[k] = 0;
                for (; j < nterms; ++j) {
                    const V x = tv[(size_t)j << lv];
                    const V y = kv[(size_t)j * kstep];
#pragma unroll
                    for (int k = 0; k < NV; ++k) w[k] += (uint64_t)x[k] * y[k];
                }
#pragma unroll
                for (int k = 0; k < NV; ++k) s[k] = add_mod<uint32_t>(s[k], multibit_redc(w[k], p, pinv_neg), p);
            }
            kv += (size_t)nterms * kstep;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const uint32_t m = (e * idx[k]) & m2n;   // e (2 bitrev(c) + 1) mod 2n: the wrap of 32 bits is a multiple of 2n
                const uint32_t w = tab[m & (n - 1u)];
                acc[k] = add_mod<uint32_t>(acc[k], mont_mul(s[k], m & n ? p - w : w, p, pinv_neg), p);
            }
        }
        out[i] = acc;
    }
}

// launcher (native_multibit.hip): nplanes planes of A in one launch
hipError_t launch_native_multibit_accumulate(const MultibitPlanes &A, unsigned nplanes, const uint32_t *rot_rows, int logn, size_t nterms,
                                             size_t nout, unsigned grouping, size_t batch, hipStream_t st);

}  // namespace cntt
