// cntt.hpp -- header-only C++17 mirror of the concrete-ntt API over the C ABI of libcntt_hip.so (cntt.h).
//
// Same module / type / method names and the same error behaviour as the crate (src/lib.rs:88-110):
//   cntt::prime32::Plan, cntt::prime64::Plan            try_new -> std::optional, fwd / inv / mul_assign_normalize /
//                                                       normalize / mul_accumulate on caller-owned slices
//   cntt::native32 / native64 / native128::Plan32, native_binary32 / 64 / 128::Plan32, and the Plan52 variants
//   cntt::product::Plan, product::FwdMode, product::InvMode
// Where the reference returns None this returns std::nullopt; where it panics (length asserts, modulus <= 1) this
// throws cntt::Panic; HIP failures -- including "no GPU": there is no CPU path -- throw cntt::DeviceError.
// The *_batch methods are the device-resident batched extension (see cntt.h for layouts).
// INPUT CONTRACT (cntt.h): coefficients handed to fwd / inv / the pointwise calls are canonical, 0 <= x < modulus.  Words >= modulus are
// neither rejected nor reduced: the call completes, the affected outputs are unspecified residues (as in the reference, whose back ends
// disagree with each other outside that range).
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "cntt.h"
#include "cntt_ext.h"
#include "cntt_multibit.h"
#include "cntt_prime_keyswitch.h"
#include "cntt_prime_multibit.h"
#include "cntt_prime_pack.h"
#include "cntt_prime_pbs.h"

namespace cntt {

struct Panic : std::logic_error {
    using std::logic_error::logic_error;
};
struct DeviceError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

namespace detail {
inline void check(int rc) {
    if (rc == CNTT_OK) return;
    const std::string msg = cntt_last_error();
    if (rc == CNTT_EINVAL || rc == CNTT_ELEN) throw Panic(msg);
    if (rc == CNTT_ENOMEM) throw std::bad_alloc();
    throw DeviceError(msg);
}
// `try_new`: CNTT_NONE -> nullopt, other failures throw
template <class H, class F> std::optional<H *> try_handle(F &&make) {
    H *h = nullptr;
    const int rc = make(&h);
    if (rc == CNTT_NONE) return std::nullopt;
    check(rc);
    return h;
}

template <class T> struct PrimeApi;
#define CNTT_PRIME_TRAITS(BITS, T)                                                                                   \
    template <> struct PrimeApi<T> {                                                                                 \
        using handle = cntt_plan##BITS##_t;                                                                          \
        static int plan_new(size_t n, T p, handle **o) { return cntt_prime##BITS##_plan_new(n, p, o); }               \
        static handle *clone(const handle *h) { return cntt_prime##BITS##_plan_clone(h); }                            \
        static void free(handle *h) { cntt_prime##BITS##_plan_free(h); }                                              \
        static size_t ntt_size(const handle *h) { return cntt_prime##BITS##_ntt_size(h); }                            \
        static T modulus(const handle *h) { return cntt_prime##BITS##_modulus(h); }                                   \
        static int fwd(const handle *h, T *b, size_t n) { return cntt_prime##BITS##_fwd(h, b, n); }                   \
        static int inv(const handle *h, T *b, size_t n) { return cntt_prime##BITS##_inv(h, b, n); }                   \
        static int mul_assign_normalize(const handle *h, T *l, size_t ln, const T *r, size_t rn) {                    \
            return cntt_prime##BITS##_mul_assign_normalize(h, l, ln, r, rn);                                          \
        }                                                                                                            \
        static int normalize(const handle *h, T *v, size_t n) { return cntt_prime##BITS##_normalize(h, v, n); }       \
        static int mul_accumulate(const handle *h, T *a, size_t an, const T *l, size_t ln, const T *r, size_t rn) {   \
            return cntt_prime##BITS##_mul_accumulate(h, a, an, l, ln, r, rn);                                         \
        }                                                                                                            \
        static int fwd_batch(const handle *h, T *b, size_t k, cntt_mem_t w, void *s) {                                \
            return cntt_prime##BITS##_fwd_batch(h, b, k, w, s);                                                       \
        }                                                                                                            \
        static int inv_batch(const handle *h, T *b, size_t k, cntt_mem_t w, void *s) {                                \
            return cntt_prime##BITS##_inv_batch(h, b, k, w, s);                                                       \
        }                                                                                                            \
        static int mul_assign_normalize_batch(const handle *h, T *l, const T *r, size_t k, cntt_mem_t w, void *s) {   \
            return cntt_prime##BITS##_mul_assign_normalize_batch(h, l, r, k, w, s);                                   \
        }                                                                                                            \
        static int mul_ntt_batch(const handle *h, T *l, const T *r, size_t k, cntt_mem_t w, void *s) {                \
            return cntt_prime##BITS##_mul_ntt_batch(h, l, r, k, w, s);                                                \
        }                                                                                                            \
        static int external_product_batch(const handle *h, T *o, const T *t, const T *key, size_t j, size_t no,      \
                                          size_t k, int acc, cntt_mem_t w, void *s) {                                 \
            return cntt_prime##BITS##_external_product_batch(h, o, t, key, j, no, k, acc, w, s);                      \
        }                                                                                                            \
        /* cntt_prime_pbs.h */                                                                                       \
        static int gadget_decompose_batch(const handle *h, T *t, const T *f, const uint32_t *rot, size_t np, unsigned bl,       \
                                          unsigned lv, cntt_src_mode_t m, size_t k, cntt_mem_t w, void *s) {         \
            return cntt_prime##BITS##_gadget_decompose_batch(h, t, f, rot, np, bl, lv, m, k, w, s);                   \
        }                                                                                                            \
        static int lwe_modswitch_batch(const handle *h, uint32_t *r, const T *lwe, size_t ld, size_t k, cntt_mem_t w, void *s) { \
            return cntt_prime##BITS##_lwe_modswitch_batch(h, r, lwe, ld, k, w, s);                                    \
        }                                                                                                            \
        static int blind_rotate_batch(const handle *h, T *acc, const T *lut, int per, const uint32_t *r, const T *bsk, size_t ld,  \
                                      size_t gd, unsigned bl, unsigned lv, size_t k, void *ws, size_t wsb, cntt_mem_t w, void *s) { \
            return cntt_prime##BITS##_blind_rotate_batch(h, acc, lut, per, r, bsk, ld, gd, bl, lv, k, ws, wsb, w, s); \
        }                                                                                                            \
        static int sample_extract_batch(const handle *h, T *o, const T *g, size_t gd, size_t idx, size_t k, cntt_mem_t w, void *s) { \
            return cntt_prime##BITS##_sample_extract_batch(h, o, g, gd, idx, k, w, s);                                \
        }                                                                                                            \
        static int bootstrap_batch(const handle *h, T *o, const T *in, const T *lut, int per, const T *bsk, size_t ld, size_t gd,  \
                                   unsigned bl, unsigned lv, size_t k, void *ws, size_t wsb, cntt_mem_t w, void *s) {  \
            return cntt_prime##BITS##_bootstrap_batch(h, o, in, lut, per, bsk, ld, gd, bl, lv, k, ws, wsb, w, s);     \
        }                                                                                                            \
        static size_t pbs_workspace_bytes(const handle *h, size_t ld, size_t gd, unsigned lv, size_t k) {             \
            return cntt_prime##BITS##_pbs_workspace_bytes(h, ld, gd, lv, k);                                          \
        }                                                                                                            \
        /* cntt_prime_keyswitch.h */                                                                                 \
        static int keyswitch_batch(const handle *h, T *o, const T *in, const T *ksk, size_t li, size_t lo, size_t rs, unsigned bl, \
                                   unsigned lv, size_t k, cntt_mem_t w, void *s) {                                    \
            return cntt_prime##BITS##_keyswitch_batch(h, o, in, ksk, li, lo, rs, bl, lv, k, w, s);                    \
        }                                                                                                            \
        static int keyswitch_bootstrap_batch(const handle *h, T *o, const T *in, const T *ksk, size_t rs, unsigned kbl, unsigned klv, \
                                             const T *lut, int per, const T *bsk, size_t ld, size_t gd, unsigned bl, unsigned lv,  \
                                             size_t k, void *ws, size_t wsb, cntt_mem_t w, void *s) {                 \
            return cntt_prime##BITS##_keyswitch_bootstrap_batch(h, o, in, ksk, rs, kbl, klv, lut, per, bsk, ld, gd, bl, lv, k, ws, wsb, \
                                                                w, s);                                               \
        }                                                                                                            \
        static size_t ks_pbs_workspace_bytes(const handle *h, size_t ld, size_t gd, unsigned lv, size_t k) {          \
            return cntt_prime##BITS##_ks_pbs_workspace_bytes(h, ld, gd, lv, k);                                       \
        }                                                                                                            \
        /* cntt_prime_pack.h */                                                                                      \
        static int pack_keyswitch_batch(const handle *h, T *o, const T *in, const T *key, size_t li, size_t m, size_t gd, unsigned bl, \
                                        unsigned lv, size_t k, void *ws, size_t wsb, cntt_mem_t w, void *s) {         \
            return cntt_prime##BITS##_pack_keyswitch_batch(h, o, in, key, li, m, gd, bl, lv, k, ws, wsb, w, s);       \
        }                                                                                                            \
        static size_t pack_workspace_bytes(const handle *h, size_t li, unsigned lv, size_t k) {                       \
            return cntt_prime##BITS##_pack_workspace_bytes(h, li, lv, k);                                             \
        }                                                                                                            \
        /* cntt_prime_multibit.h */                                                                                  \
        static int multibit_accumulate_batch(const handle *h, T *o, const T *t, const uint32_t *r, const T *key, size_t nt, size_t no, \
                                             unsigned g, size_t k, cntt_mem_t w, void *s) {                           \
            return cntt_prime##BITS##_multibit_accumulate_batch(h, o, t, r, key, nt, no, g, k, w, s);                 \
        }                                                                                                            \
        static int multibit_blind_rotate_batch(const handle *h, T *a, const T *lut, int per, const uint32_t *r, const T *key, size_t ld, \
                                               size_t gd, unsigned bl, unsigned lv, unsigned g, size_t k, void *ws, size_t wsb,     \
                                               cntt_mem_t w, void *s) {                                               \
            return cntt_prime##BITS##_multibit_blind_rotate_batch(h, a, lut, per, r, key, ld, gd, bl, lv, g, k, ws, wsb, w, s); \
        }                                                                                                            \
        static int multibit_bootstrap_batch(const handle *h, T *o, const T *in, const T *lut, int per, const T *key, size_t ld, size_t gd, \
                                            unsigned bl, unsigned lv, unsigned g, size_t k, void *ws, size_t wsb, cntt_mem_t w,       \
                                            void *s) {                                                                \
            return cntt_prime##BITS##_multibit_bootstrap_batch(h, o, in, lut, per, key, ld, gd, bl, lv, g, k, ws, wsb, w, s); \
        }                                                                                                            \
        static size_t multibit_pbs_workspace_bytes(const handle *h, size_t ld, size_t gd, unsigned lv, unsigned g, size_t k) { \
            return cntt_prime##BITS##_multibit_pbs_workspace_bytes(h, ld, gd, lv, g, k);                              \
        }                                                                                                            \
    };
CNTT_PRIME_TRAITS(32, uint32_t)
CNTT_PRIME_TRAITS(64, uint64_t)
#undef CNTT_PRIME_TRAITS

// prime32::Plan / prime64::Plan (src/prime32.rs:601-927, src/prime64.rs:221-1129)
template <class T> class PrimePlan {
    using A = PrimeApi<T>;
    typename A::handle *h_ = nullptr;
    bool owned_ = true;

  public:
    explicit PrimePlan(typename A::handle *h, bool owned = true) : h_(h), owned_(owned) {}
    PrimePlan(const PrimePlan &o) : h_(A::clone(o.h_)) {}  // #[derive(Clone)]
    PrimePlan(PrimePlan &&o) noexcept : h_(std::exchange(o.h_, nullptr)), owned_(o.owned_) {}
    PrimePlan &operator=(PrimePlan o) noexcept {
        std::swap(h_, o.h_);
        std::swap(owned_, o.owned_);
        return *this;
    }
    ~PrimePlan() {
        if (h_ && owned_) A::free(h_);
    }
    static std::optional<PrimePlan> try_new(size_t polynomial_size, T modulus) {
        auto h = try_handle<typename A::handle>([&](auto **o) { return A::plan_new(polynomial_size, modulus, o); });
        if (!h) return std::nullopt;
        return PrimePlan(*h);
    }
    size_t ntt_size() const { return A::ntt_size(h_); }
    T modulus() const { return A::modulus(h_); }
    void fwd(T *buf, size_t len) const { check(A::fwd(h_, buf, len)); }
    void inv(T *buf, size_t len) const { check(A::inv(h_, buf, len)); }
    void fwd(std::vector<T> &buf) const { fwd(buf.data(), buf.size()); }
    void inv(std::vector<T> &buf) const { inv(buf.data(), buf.size()); }
    void mul_assign_normalize(T *lhs, size_t ln, const T *rhs, size_t rn) const { check(A::mul_assign_normalize(h_, lhs, ln, rhs, rn)); }
    void mul_assign_normalize(std::vector<T> &lhs, const std::vector<T> &rhs) const {
        mul_assign_normalize(lhs.data(), lhs.size(), rhs.data(), rhs.size());
    }
    void normalize(T *v, size_t n) const { check(A::normalize(h_, v, n)); }
    void mul_accumulate(T *acc, size_t an, const T *lhs, size_t ln, const T *rhs, size_t rn) const {
        check(A::mul_accumulate(h_, acc, an, lhs, ln, rhs, rn));
    }
    // batched extension: `batch` polynomials back to back in device (or host) memory, enqueued on `stream`
    void fwd_batch(T *bufs, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::fwd_batch(h_, bufs, batch, where, stream));
    }
    void inv_batch(T *bufs, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::inv_batch(h_, bufs, batch, where, stream));
    }
    void mul_assign_normalize_batch(T *lhs, const T *rhs, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::mul_assign_normalize_batch(h_, lhs, rhs, batch, where, stream));
    }
    void mul_ntt_batch(T *lhs, const T *rhs_ntt, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::mul_ntt_batch(h_, lhs, rhs_ntt, batch, where, stream));
    }
    void external_product_batch(T *out, const T *terms, const T *key_ntt, size_t nterms, size_t nout, size_t batch,
                                bool accumulate = false, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::external_product_batch(h_, out, terms, key_ntt, nterms, nout, batch, accumulate ? 1 : 0, where, stream));
    }
    // programmable bootstrap mod p (cntt_prime_pbs.h): signed digits of the balanced lift of polys, X^rot polys or X^rot polys - polys;
    // modulus switch to exponents below 2n; blind rotation in place over bsk_ntt = n^-1 fwd(key); sample extraction; all in one call
    void gadget_decompose_batch(T *terms, const T *polys, const uint32_t *rot, size_t npolys, unsigned base_log, unsigned levels,
                                cntt_src_mode_t src_mode, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::gadget_decompose_batch(h_, terms, polys, rot, npolys, base_log, levels, src_mode, batch, where, stream));
    }
    void lwe_modswitch_batch(uint32_t *rot_t, const T *lwe, size_t lwe_dim, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                             void *stream = nullptr) const {
        check(A::lwe_modswitch_batch(h_, rot_t, lwe, lwe_dim, batch, where, stream));
    }
    void blind_rotate_batch(T *acc, const T *lut, bool lut_per_element, const uint32_t *rot_t, const T *bsk_ntt, size_t lwe_dim,
                            size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                            size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::blind_rotate_batch(h_, acc, lut, lut_per_element ? 1 : 0, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch,
                                    workspace, workspace_bytes, where, stream));
    }
    void sample_extract_batch(T *lwe_out, const T *glwe, size_t glwe_dim, size_t index, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                              void *stream = nullptr) const {
        check(A::sample_extract_batch(h_, lwe_out, glwe, glwe_dim, index, batch, where, stream));
    }
    void bootstrap_batch(T *lwe_out, const T *lwe_in, const T *lut, bool lut_per_element, const T *bsk_ntt, size_t lwe_dim,
                         size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                         size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::bootstrap_batch(h_, lwe_out, lwe_in, lut, lut_per_element ? 1 : 0, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch,
                                 workspace, workspace_bytes, where, stream));
    }
    size_t pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) const {
        return A::pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels, batch);
    }
    // LWE keyswitch mod p (cntt_prime_keyswitch.h) from lwe_dim_in to lwe_dim_out, and keyswitch (glwe_dim * n -> lwe_dim) + bootstrap in
    // one call
    void keyswitch_batch(T *lwe_out, const T *lwe_in, const T *ksk, size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride,
                         unsigned base_log, unsigned levels, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::keyswitch_batch(h_, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where, stream));
    }
    size_t ks_pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk, size_t batch) const {
        return A::ks_pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels_bsk, batch);
    }
    void keyswitch_bootstrap_batch(T *lwe_out, const T *lwe_in, const T *ksk, size_t row_stride, unsigned ks_base_log, unsigned ks_levels,
                                   const T *lut, bool lut_per_element, const T *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                   unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr, size_t workspace_bytes = 0,
                                   cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::keyswitch_bootstrap_batch(h_, lwe_out, lwe_in, ksk, row_stride, ks_base_log, ks_levels, lut, lut_per_element ? 1 : 0,
                                           bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace, workspace_bytes, where, stream));
    }
    // LWE-to-GLWE packing keyswitch through the NTT mod p (cntt_prime_pack.h): lwe_count LWE ciphertexts of dimension lwe_dim_in into one
    // GLWE; pksk_ntt = n^-1 fwd(key), one buffer
    size_t pack_workspace_bytes(size_t lwe_dim_in, unsigned levels, size_t batch) const {
        return A::pack_workspace_bytes(h_, lwe_dim_in, levels, batch);
    }
    void pack_keyswitch_batch(T *glwe_out, const T *lwe_in, const T *pksk_ntt, size_t lwe_dim_in, size_t lwe_count, size_t glwe_dim,
                              unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr, size_t workspace_bytes = 0,
                              cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::pack_keyswitch_batch(h_, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch, workspace,
                                      workspace_bytes, where, stream));
    }
    // multi-bit blind rotation and bootstrap mod p (cntt_prime_multibit.h): groups of `grouping` mask words, one bundled external product
    // each; bsk_mb = n^-1 fwd(key), one buffer of (lwe_dim / grouping) * 2^grouping GGSW ciphertexts
    size_t multibit_pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels, unsigned grouping, size_t batch) const {
        return A::multibit_pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels, grouping, batch);
    }
    void multibit_accumulate_batch(T *out_ntt, const T *terms_ntt, const uint32_t *rot_rows, const T *key_group, size_t nterms, size_t nout,
                                   unsigned grouping, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(A::multibit_accumulate_batch(h_, out_ntt, terms_ntt, rot_rows, key_group, nterms, nout, grouping, batch, where, stream));
    }
    void multibit_blind_rotate_batch(T *acc, const T *lut, bool lut_per_element, const uint32_t *rot_t, const T *bsk_mb, size_t lwe_dim,
                                     size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                     void *workspace = nullptr, size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE,
                                     void *stream = nullptr) const {
        check(A::multibit_blind_rotate_batch(h_, acc, lut, lut_per_element ? 1 : 0, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log, levels,
                                             grouping, batch, workspace, workspace_bytes, where, stream));
    }
    void multibit_bootstrap_batch(T *lwe_out, const T *lwe_in, const T *lut, bool lut_per_element, const T *bsk_mb, size_t lwe_dim,
                                  size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                  void *workspace = nullptr, size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE,
                                  void *stream = nullptr) const {
        check(A::multibit_bootstrap_batch(h_, lwe_out, lwe_in, lut, lut_per_element ? 1 : 0, bsk_mb, lwe_dim, glwe_dim, base_log, levels,
                                          grouping, batch, workspace, workspace_bytes, where, stream));
    }
    const typename A::handle *handle() const { return h_; }
};

// native / native_binary plans: W = coefficient word (uint32_t, uint64_t, or u128 as two uint64_t), R = residue word
template <cntt_native_kind_t KIND, class R, int NPRIMES, int WORD_BYTES> class NativePlan {
    cntt_native_t *h_ = nullptr;

  public:
    explicit NativePlan(cntt_native_t *h) : h_(h) {}
    NativePlan(const NativePlan &o) : h_(cntt_native_plan_clone(o.h_)) {}
    NativePlan(NativePlan &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    NativePlan &operator=(NativePlan o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~NativePlan() {
        if (h_) cntt_native_plan_free(h_);
    }
    static std::optional<NativePlan> try_new(size_t polynomial_size) {
        auto h = try_handle<cntt_native_t>([&](auto **o) { return cntt_native_plan_new(KIND, polynomial_size, o); });
        if (!h) return std::nullopt;
        return NativePlan(*h);
    }
    size_t ntt_size() const { return cntt_native_ntt_size(h_); }
    static constexpr int nprimes() { return NPRIMES; }
    // ntt_0() .. ntt_k(): borrowed prime plan
    PrimePlan<R> ntt(int i) const {
        if constexpr (sizeof(R) == 4)
            return PrimePlan<R>(const_cast<cntt_plan32_t *>(cntt_native_ntt32(h_, i)), false);
        else
            return PrimePlan<R>(const_cast<cntt_plan64_t *>(cntt_native_ntt64(h_, i)), false);
    }
    // value: ntt_size words of WORD_BYTES bytes; residues: NPRIMES buffers of ntt_size R words
    void fwd(const void *value, size_t len, R *const (&residues)[NPRIMES]) const {
        check(cntt_native_fwd(h_, value, len, reinterpret_cast<void *const *>(residues)));
    }
    void fwd_binary(const void *value, size_t len, R *const (&residues)[NPRIMES]) const {
        check(cntt_native_fwd_binary(h_, value, len, reinterpret_cast<void *const *>(residues)));
    }
    void inv(void *value, size_t len, R *const (&residues)[NPRIMES]) const {
        check(cntt_native_inv(h_, value, len, reinterpret_cast<void *const *>(residues)));
    }
    void negacyclic_polymul(void *prod, size_t pn, const void *lhs, size_t ln, const void *rhs, size_t rn) const {
        check(cntt_native_negacyclic_polymul(h_, prod, pn, lhs, ln, rhs, rn));
    }
    void negacyclic_polymul_batch(void *prod, const void *lhs, const void *rhs, size_t batch,
                                  cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_negacyclic_polymul_batch(h_, prod, lhs, rhs, batch, where, stream));
    }
    void reserve(size_t batch) const { check(cntt_native_reserve(h_, batch)); }
    // external product (cntt_ext.h): out[b][o] (+)= sum_j terms[b][j] (*) key[j][o] mod 2^w, key_ntt = NPRIMES residue planes of
    // nterms * nout forward-transformed key polynomials
    size_t max_terms() const { return cntt_native_max_terms(h_); }
    void external_product_batch(void *out, const void *terms, const void *const *key_ntt, size_t nterms, size_t nout, size_t batch,
                                bool accumulate = false, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_external_product_batch(h_, out, terms, key_ntt, nterms, nout, batch, accumulate ? 1 : 0, where, stream));
    }
    // signed gadget digits of polys, X^rot polys or X^rot polys - polys (cntt_gadget.h), and the external product that derives them
    // while loading: out = addend + sum_{p,l} digit_l(source(polys[p])) (*) key[p * levels + l - 1][o]
    void gadget_decompose_batch(void *terms, const void *polys, const uint32_t *rot, size_t npolys, unsigned base_log, unsigned levels,
                                cntt_src_mode_t mode, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_gadget_decompose_batch(h_, terms, polys, rot, npolys, base_log, levels, mode, batch, where, stream));
    }
    void external_product_decomposed_batch(void *out, const void *polys, const uint32_t *rot, const void *addend,
                                           const void *const *key_ntt, size_t npolys, unsigned base_log, unsigned levels,
                                           cntt_src_mode_t mode, size_t nout, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                                           void *stream = nullptr) const {
        check(cntt_native_external_product_decomposed_batch(h_, out, polys, rot, addend, key_ntt, npolys, base_log, levels, mode, nout,
                                                            batch, where, stream));
    }
    // programmable bootstrap (cntt_pbs.h): modulus switch, blind rotation in place, sample extraction, and all three in one call
    size_t pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels, size_t batch) const {
        return cntt_native_pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels, batch);
    }
    void lwe_modswitch_batch(uint32_t *rot_t, const void *lwe, size_t lwe_dim, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                             void *stream = nullptr) const {
        check(cntt_native_lwe_modswitch_batch(h_, rot_t, lwe, lwe_dim, batch, where, stream));
    }
    void blind_rotate_batch(void *acc, const void *lut, bool lut_per_element, const uint32_t *rot_t, const void *const *bsk_ntt,
                            size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                            size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_blind_rotate_batch(h_, acc, lut, lut_per_element ? 1 : 0, rot_t, bsk_ntt, lwe_dim, glwe_dim, base_log, levels,
                                             batch, workspace, workspace_bytes, where, stream));
    }
    void sample_extract_batch(void *lwe_out, const void *glwe, size_t glwe_dim, size_t index, size_t batch,
                              cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_sample_extract_batch(h_, lwe_out, glwe, glwe_dim, index, batch, where, stream));
    }
    void bootstrap_batch(void *lwe_out, const void *lwe_in, const void *lut, bool lut_per_element, const void *const *bsk_ntt,
                         size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                         size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_bootstrap_batch(h_, lwe_out, lwe_in, lut, lut_per_element ? 1 : 0, bsk_ntt, lwe_dim, glwe_dim, base_log, levels,
                                          batch, workspace, workspace_bytes, where, stream));
    }
    // LWE keyswitch (cntt_keyswitch.h) from lwe_dim_in to lwe_dim_out, and keyswitch (glwe_dim * n -> lwe_dim) + bootstrap in one call
    void keyswitch_batch(void *lwe_out, const void *lwe_in, const void *ksk, size_t lwe_dim_in, size_t lwe_dim_out, size_t row_stride,
                         unsigned base_log, unsigned levels, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                         void *stream = nullptr) const {
        check(cntt_native_keyswitch_batch(h_, lwe_out, lwe_in, ksk, lwe_dim_in, lwe_dim_out, row_stride, base_log, levels, batch, where,
                                          stream));
    }
    size_t ks_pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels_bsk, size_t batch) const {
        return cntt_native_ks_pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels_bsk, batch);
    }
    void keyswitch_bootstrap_batch(void *lwe_out, const void *lwe_in, const void *ksk, size_t row_stride, unsigned ks_base_log,
                                   unsigned ks_levels, const void *lut, bool lut_per_element, const void *const *bsk_ntt, size_t lwe_dim,
                                   size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                                   size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_keyswitch_bootstrap_batch(h_, lwe_out, lwe_in, ksk, row_stride, ks_base_log, ks_levels, lut,
                                                    lut_per_element ? 1 : 0, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, batch, workspace,
                                                    workspace_bytes, where, stream));
    }
    // LWE-to-GLWE packing keyswitch through the NTT (cntt_pack.h): lwe_count LWE ciphertexts of dimension lwe_dim_in into one GLWE
    size_t pack_workspace_bytes(size_t lwe_dim_in, unsigned levels, size_t batch) const {
        return cntt_native_pack_workspace_bytes(h_, lwe_dim_in, levels, batch);
    }
    void pack_keyswitch_batch(void *glwe_out, const void *lwe_in, const void *const *pksk_ntt, size_t lwe_dim_in, size_t lwe_count,
                              size_t glwe_dim, unsigned base_log, unsigned levels, size_t batch, void *workspace = nullptr,
                              size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE, void *stream = nullptr) const {
        check(cntt_native_pack_keyswitch_batch(h_, glwe_out, lwe_in, pksk_ntt, lwe_dim_in, lwe_count, glwe_dim, base_log, levels, batch,
                                               workspace, workspace_bytes, where, stream));
    }
    // multi-bit blind rotation and bootstrap (cntt_multibit.h; Plan32 kinds): groups of `grouping` mask words, one bundled external
    // product each; bsk_mb = the residue planes cntt_native_fwd_batch writes for (lwe_dim / grouping) * 2^grouping GGSW ciphertexts
    size_t multibit_pbs_workspace_bytes(size_t lwe_dim, size_t glwe_dim, unsigned levels, unsigned grouping, size_t batch) const {
        return cntt_native_multibit_pbs_workspace_bytes(h_, lwe_dim, glwe_dim, levels, grouping, batch);
    }
    void multibit_accumulate_batch(void *const *out_ntt, const void *const *terms_ntt, const uint32_t *rot_rows, const void *const *key_group,
                                   size_t nterms, size_t nout, unsigned grouping, size_t batch, cntt_mem_t where = CNTT_MEM_DEVICE,
                                   void *stream = nullptr) const {
        check(cntt_native_multibit_accumulate_batch(h_, out_ntt, terms_ntt, rot_rows, key_group, nterms, nout, grouping, batch, where, stream));
    }
    void multibit_blind_rotate_batch(void *acc, const void *lut, bool lut_per_element, const uint32_t *rot_t, const void *const *bsk_mb,
                                     size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                     void *workspace = nullptr, size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE,
                                     void *stream = nullptr) const {
        check(cntt_native_multibit_blind_rotate_batch(h_, acc, lut, lut_per_element ? 1 : 0, rot_t, bsk_mb, lwe_dim, glwe_dim, base_log,
                                                      levels, grouping, batch, workspace, workspace_bytes, where, stream));
    }
    void multibit_bootstrap_batch(void *lwe_out, const void *lwe_in, const void *lut, bool lut_per_element, const void *const *bsk_mb,
                                  size_t lwe_dim, size_t glwe_dim, unsigned base_log, unsigned levels, unsigned grouping, size_t batch,
                                  void *workspace = nullptr, size_t workspace_bytes = 0, cntt_mem_t where = CNTT_MEM_DEVICE,
                                  void *stream = nullptr) const {
        check(cntt_native_multibit_bootstrap_batch(h_, lwe_out, lwe_in, lut, lut_per_element ? 1 : 0, bsk_mb, lwe_dim, glwe_dim, base_log,
                                                   levels, grouping, batch, workspace, workspace_bytes, where, stream));
    }
};
}  // namespace detail

// Contiguous shard [begin, end) of `rank` when a batch of independent polynomials is split over `world` devices (cntt_shard_bounds;
// SURVEY 8e): the caller drives the devices -- one thread + stream per device around a shared plan, examples/multi_device.cpp.
inline std::pair<size_t, size_t> shard_bounds(size_t batch, int world, int rank) {
    size_t b = 0, e = 0;
    detail::check(cntt_shard_bounds(batch, world, rank, &b, &e));
    return {b, e};
}
// TESTING ONLY (include/cntt.h): kernel-selection switches for A/B timing and device-vs-device parity tests; results never change.
inline void debug_set(const char *key, int value) { detail::check(cntt_debug_set(key, value)); }
inline int debug_get(const char *key) {
    int v = 0;
    detail::check(cntt_debug_get(key, &v));
    return v;
}


namespace prime32 {
using Plan = detail::PrimePlan<uint32_t>;
}
namespace prime64 {
using Plan = detail::PrimePlan<uint64_t>;
struct Solinas {
    static constexpr uint64_t P = 0xFFFFFFFF00000001ull;  // src/prime64/generic_solinas.rs:35-40
};
}  // namespace prime64
namespace native32 {
using Plan32 = detail::NativePlan<CNTT_NATIVE32_PLAN32, uint32_t, 3, 4>;
using Plan52 = detail::NativePlan<CNTT_NATIVE32_PLAN52, uint64_t, 2, 4>;
}  // namespace native32
namespace native64 {
using Plan32 = detail::NativePlan<CNTT_NATIVE64_PLAN32, uint32_t, 5, 8>;
using Plan52 = detail::NativePlan<CNTT_NATIVE64_PLAN52, uint64_t, 3, 8>;
}  // namespace native64
namespace native128 {
using Plan32 = detail::NativePlan<CNTT_NATIVE128_PLAN32, uint32_t, 10, 16>;
}
namespace native_binary32 {
using Plan32 = detail::NativePlan<CNTT_NATIVE_BINARY32_PLAN32, uint32_t, 2, 4>;
using Plan52 = detail::NativePlan<CNTT_NATIVE_BINARY32_PLAN52, uint64_t, 1, 4>;
}  // namespace native_binary32
namespace native_binary64 {
using Plan32 = detail::NativePlan<CNTT_NATIVE_BINARY64_PLAN32, uint32_t, 3, 8>;
using Plan52 = detail::NativePlan<CNTT_NATIVE_BINARY64_PLAN52, uint64_t, 2, 8>;
}  // namespace native_binary64
namespace native_binary128 {
using Plan32 = detail::NativePlan<CNTT_NATIVE_BINARY128_PLAN32, uint32_t, 5, 16>;
}

// product::Plan (src/product.rs:139-967)
namespace product {
struct FwdMode {  // enum FwdMode { Generic, Bounded(u64) }  src/product.rs:124-129
    bool bounded = false;
    uint64_t bound = 0;
    static FwdMode Generic() { return {}; }
    static FwdMode Bounded(uint64_t b) { return {true, b}; }
};
enum class InvMode { Replace = CNTT_INV_REPLACE, Accumulate = CNTT_INV_ACCUMULATE };  // src/product.rs:131-136

class Plan {
    cntt_product_t *h_ = nullptr;

  public:
    explicit Plan(cntt_product_t *h) : h_(h) {}
    Plan(const Plan &o) : h_(cntt_product_plan_clone(o.h_)) {}
    Plan(Plan &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Plan &operator=(Plan o) noexcept {
        std::swap(h_, o.h_);
        return *this;
    }
    ~Plan() {
        if (h_) cntt_product_plan_free(h_);
    }
    static std::optional<Plan> try_new(size_t polynomial_size, uint64_t modulus, const std::vector<uint64_t> &factors) {
        auto h = detail::try_handle<cntt_product_t>(
            [&](auto **o) { return cntt_product_plan_new(polynomial_size, modulus, factors.data(), factors.size(), o); });
        if (!h) return std::nullopt;
        return Plan(*h);
    }
    size_t ntt_size() const { return cntt_product_ntt_size(h_); }
    uint64_t modulus() const { return cntt_product_modulus(h_); }
    size_t ntt_domain_len() const { return cntt_product_ntt_domain_len(h_); }
    void fwd(std::vector<uint64_t> &ntt, const std::vector<uint64_t> &standard, FwdMode mode) const {
        detail::check(cntt_product_fwd(h_, ntt.data(), ntt.size(), standard.data(), standard.size(),
                                       mode.bounded ? CNTT_FWD_BOUNDED : CNTT_FWD_GENERIC, mode.bound));
    }
    void inv(std::vector<uint64_t> &standard, std::vector<uint64_t> &ntt, InvMode mode) const {
        detail::check(cntt_product_inv(h_, standard.data(), standard.size(), ntt.data(), ntt.size(), (cntt_inv_mode_t)mode));
    }
    void mul_assign_normalize(std::vector<uint64_t> &lhs, const std::vector<uint64_t> &rhs) const {
        detail::check(cntt_product_mul_assign_normalize(h_, lhs.data(), lhs.size(), rhs.data(), rhs.size()));
    }
    void normalize(std::vector<uint64_t> &values) const { detail::check(cntt_product_normalize(h_, values.data(), values.size())); }
    void mul_accumulate(std::vector<uint64_t> &acc, const std::vector<uint64_t> &lhs, const std::vector<uint64_t> &rhs) const {
        detail::check(cntt_product_mul_accumulate(h_, acc.data(), acc.size(), lhs.data(), lhs.size(), rhs.data(), rhs.size()));
    }
    // batched extension (plane-major NTT domain, see cntt.h)
    void fwd_batch(uint64_t *ntt, const uint64_t *standard, size_t batch, FwdMode mode, cntt_mem_t where = CNTT_MEM_DEVICE,
                   void *stream = nullptr) const {
        detail::check(cntt_product_fwd_batch(h_, ntt, standard, batch, mode.bounded ? CNTT_FWD_BOUNDED : CNTT_FWD_GENERIC,
                                             mode.bound, where, stream));
    }
    void inv_batch(uint64_t *standard, uint64_t *ntt, size_t batch, InvMode mode, cntt_mem_t where = CNTT_MEM_DEVICE,
                   void *stream = nullptr) const {
        detail::check(cntt_product_inv_batch(h_, standard, ntt, batch, (cntt_inv_mode_t)mode, where, stream));
    }
    void external_product_batch(uint64_t *out, const uint64_t *terms, const uint64_t *key_ntt, size_t nterms, size_t nout,
                                size_t batch, FwdMode fmode, InvMode imode, cntt_mem_t where = CNTT_MEM_DEVICE,
                                void *stream = nullptr) const {
        detail::check(cntt_product_external_product_batch(h_, out, terms, key_ntt, nterms, nout, batch,
                                                          fmode.bounded ? CNTT_FWD_BOUNDED : CNTT_FWD_GENERIC, fmode.bound,
                                                          (cntt_inv_mode_t)imode, where, stream));
    }
};
}  // namespace product

}  // namespace cntt
