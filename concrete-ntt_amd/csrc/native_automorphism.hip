// kernel instantiations and the launchers of the native plans' ring automorphism (native_automorphism.hpp): u32 / u64 / Word128 words,
// u32 / u64 residues
#include "native_automorphism.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W autom_word_from(U128 v) { return (W)v; }
template <> Word128 autom_word_from<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

// t^-1 mod 2n for odd t: Newton's iteration doubles the correct low bits (t t = 1 mod 8 to start with)
static uint32_t native_inverse_mod_2n(uint32_t t, int logn) {
    uint32_t x = t;
    for (int i = 0; i < 5; ++i) x *= 2u - t * x;
    return x & ((2u << logn) - 1u);
}

// a thread owns 16 bytes, so a polynomial is at least one vector of the widest count (4 words)
static bool autom_shape_ok(int logn, uint32_t t) { return logn >= 2 && logn <= 30 && (t & 1u) != 0 && t < (2u << logn); }

template <class W>
static void automorphism_w(void *out, const void *in, uint32_t t, bool ntt, int logn, size_t npoly_total, bool stream, bool lds, hipStream_t st) {
    const size_t bytes = sizeof(W) << logn;
    const bool use_lds = lds && bytes <= NATIVE_AUTOM_LDS_BYTES;
    const dim3 grid(native_automorphism_grid(npoly_total, logn, sizeof(W))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = native_inverse_mod_2n(t, logn), ln = (uint32_t)logn;
#define CNTT_NATIVE_AUTOM_LAUNCH(STREAM, LDS)                                                                                                \
    do {                                                                                                                                     \
        if constexpr (sizeof(W) <= 8) {                                                                                                      \
            if (ntt) {                                                                                                                       \
                hipLaunchKernelGGL((native_automorphism_ntt_kernel<W, STREAM, LDS>), grid, block, shm, st, (W *)out, (const W *)in, t, ln,   \
                                   npoly_total);                                                                                             \
                break;                                                                                                                       \
            }                                                                                                                                \
        }                                                                                                                                    \
        hipLaunchKernelGGL((native_automorphism_kernel<W, STREAM, LDS>), grid, block, shm, st, (W *)out, (const W *)in, tinv, ln,            \
                           npoly_total);                                                                                                     \
    } while (0)
    if (stream && use_lds) CNTT_NATIVE_AUTOM_LAUNCH(true, true);
    else if (stream) CNTT_NATIVE_AUTOM_LAUNCH(true, false);
    else if (use_lds) CNTT_NATIVE_AUTOM_LAUNCH(false, true);
    else CNTT_NATIVE_AUTOM_LAUNCH(false, false);
#undef CNTT_NATIVE_AUTOM_LAUNCH
}

hipError_t launch_native_automorphism(int word, void *out, const void *in, uint32_t t, bool ntt, int logn, size_t npoly_total, bool stream,
                                      bool lds, hipStream_t st) {
    if ((word != 4 && word != 8 && (word != 16 || ntt)) || !autom_shape_ok(logn, t) || npoly_total == 0) return hipErrorInvalidValue;
    if (word == 4) automorphism_w<uint32_t>(out, in, t, ntt, logn, npoly_total, stream, lds, st);
    else if (word == 8) automorphism_w<uint64_t>(out, in, t, ntt, logn, npoly_total, stream, lds, st);
    else automorphism_w<Word128>(out, in, t, ntt, logn, npoly_total, stream, lds, st);
    return hipGetLastError();
}

template <class W>
static void automorphism_gadget_w(void *terms, void *out, const void *in, U128 off, unsigned base_log, unsigned levels, uint32_t t, int logn,
                                  size_t glwe_dim, bool add_input, size_t batch, bool stream, bool lds, hipStream_t st) {
    GadgetConst<W> G{};   // (npolys, rotated, cmux: the source fields of native_gadget_kernel, not read here)
    G.off = autom_word_from<W>(off);
    G.mask = autom_word_from<W>(base_log == 128 ? ~(U128)0 : ((U128)1 << base_log) - 1);
    G.half = autom_word_from<W>((U128)1 << (base_log - 1));
    G.base_log = base_log;
    G.levels = levels;
    const size_t bytes = sizeof(W) << logn;
    const bool use_lds = lds && bytes <= NATIVE_AUTOM_LDS_BYTES;
    const dim3 grid(native_automorphism_grid(batch * (glwe_dim + 1), logn, sizeof(W))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = native_inverse_mod_2n(t, logn), ln = (uint32_t)logn, k = (uint32_t)glwe_dim, add = add_input ? 1u : 0u;
#define CNTT_NATIVE_AUTOM_LAUNCH(STREAM, LDS)                                                                                                \
    hipLaunchKernelGGL((native_automorphism_gadget_kernel<W, STREAM, LDS>), grid, block, shm, st, (W *)terms, (W *)out, (const W *)in, G,    \
                       tinv, ln, k, add, batch)
    if (stream && use_lds) CNTT_NATIVE_AUTOM_LAUNCH(true, true);
    else if (stream) CNTT_NATIVE_AUTOM_LAUNCH(true, false);
    else if (use_lds) CNTT_NATIVE_AUTOM_LAUNCH(false, true);
    else CNTT_NATIVE_AUTOM_LAUNCH(false, false);
#undef CNTT_NATIVE_AUTOM_LAUNCH
}

hipError_t launch_native_automorphism_gadget(int word, void *terms, void *out, const void *in, uint64_t off_lo, uint64_t off_hi,
                                             unsigned base_log, unsigned levels, uint32_t t, int logn, size_t glwe_dim, bool add_input,
                                             size_t batch, bool stream, bool lds, hipStream_t st) {
    const unsigned wbits = 8u * (unsigned)word;
    if ((word != 4 && word != 8 && word != 16) || !autom_shape_ok(logn, t) || batch == 0 || glwe_dim + 1 >= ((size_t)1 << 32) || levels == 0 ||
        base_log == 0 || (uint64_t)base_log * levels > wbits || (!terms && glwe_dim))
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    if (word == 4) automorphism_gadget_w<uint32_t>(terms, out, in, off, base_log, levels, t, logn, glwe_dim, add_input, batch, stream, lds, st);
    else if (word == 8) automorphism_gadget_w<uint64_t>(terms, out, in, off, base_log, levels, t, logn, glwe_dim, add_input, batch, stream, lds, st);
    else automorphism_gadget_w<Word128>(terms, out, in, off, base_log, levels, t, logn, glwe_dim, add_input, batch, stream, lds, st);
    return hipGetLastError();
}

}  // namespace cntt
