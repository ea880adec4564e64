// kernel instantiations and the launchers of the native plans' ring packing (native_ring_pack.hpp): u32 / u64 / Word128 words
#include "native_ring_pack.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W ring_word_from(U128 v) { return (W)v; }
template <> Word128 ring_word_from<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

// t^-1 mod 2n for odd t: Newton's iteration doubles the correct low bits (t t = 1 mod 8 to start with)
static uint32_t ring_inverse_mod_2n(uint32_t t, int logn) {
    uint32_t x = t;
    for (int i = 0; i < 5; ++i) x *= 2u - t * x;
    return x & ((2u << logn) - 1u);
}

// a thread owns 16 bytes, so a polynomial is at least one vector of the widest count (4 words)
static bool ring_shape_ok(int word, int logn, size_t glwe_dim) {
    return (word == 4 || word == 8 || word == 16) && logn >= 2 && logn <= 30 && glwe_dim + 1 < ((size_t)1 << 32);
}

template <class W> static void glwe_embed_w(void *glwe, const void *lwe, int logn, size_t glwe_dim, size_t batch, hipStream_t st) {
    const dim3 grid(native_ring_pack_grid(batch * (glwe_dim + 1), logn, sizeof(W))), block(256);
    hipLaunchKernelGGL((native_glwe_embed_kernel<W>), grid, block, 0, st, (W *)glwe, (const W *)lwe, (uint32_t)logn, (uint32_t)glwe_dim, batch);
}

hipError_t launch_native_glwe_embed(int word, void *glwe, const void *lwe, int logn, size_t glwe_dim, size_t batch, hipStream_t st) {
    if (!ring_shape_ok(word, logn, glwe_dim) || batch == 0) return hipErrorInvalidValue;
    if (word == 4) glwe_embed_w<uint32_t>(glwe, lwe, logn, glwe_dim, batch, st);
    else if (word == 8) glwe_embed_w<uint64_t>(glwe, lwe, logn, glwe_dim, batch, st);
    else glwe_embed_w<Word128>(glwe, lwe, logn, glwe_dim, batch, st);
    return hipGetLastError();
}

template <class W>
static void ring_merge_w(void *terms, void *out, const void *even, const void *odd, bool leaf, U128 off, unsigned base_log, unsigned levels,
                         uint32_t t, uint32_t shift, int logn, size_t glwe_dim, size_t h, size_t gs, size_t nct, bool stream, bool lds,
                         hipStream_t st) {
    GadgetConst<W> G{};   // (npolys, rotated, cmux: the source fields of native_gadget_kernel, not read here)
    G.off = ring_word_from<W>(off);
    G.mask = ring_word_from<W>(base_log == 128 ? ~(U128)0 : ((U128)1 << base_log) - 1);
    G.half = ring_word_from<W>((U128)1 << (base_log - 1));
    G.base_log = base_log;
    G.levels = levels;
    const size_t bytes = (2 * sizeof(W)) << logn;
    const bool use_lds = lds && bytes <= NATIVE_AUTOM_LDS_BYTES;
    const dim3 grid(native_ring_pack_grid(nct * (glwe_dim + 1), logn, sizeof(W))), block(256);
    const size_t shm = use_lds ? bytes : 0;
    const uint32_t tinv = ring_inverse_mod_2n(t, logn), ln = (uint32_t)logn, k = (uint32_t)glwe_dim;
#define CNTT_NATIVE_RING_LAUNCH(STREAM, LDS)                                                                                                 \
    do {                                                                                                                                     \
        if (leaf)                                                                                                                            \
            hipLaunchKernelGGL((native_ring_merge_kernel<W, STREAM, LDS, true>), grid, block, shm, st, (W *)terms, (W *)out, (const W *)even, \
                               (const W *)odd, G, tinv, shift, ln, k, h, gs, nct);                                                           \
        else                                                                                                                                 \
            hipLaunchKernelGGL((native_ring_merge_kernel<W, STREAM, LDS, false>), grid, block, shm, st, (W *)terms, (W *)out,                \
                               (const W *)even, (const W *)odd, G, tinv, shift, ln, k, h, gs, nct);                                          \
    } while (0)
    if (stream && use_lds) CNTT_NATIVE_RING_LAUNCH(true, true);
    else if (stream) CNTT_NATIVE_RING_LAUNCH(true, false);
    else if (use_lds) CNTT_NATIVE_RING_LAUNCH(false, true);
    else CNTT_NATIVE_RING_LAUNCH(false, false);
#undef CNTT_NATIVE_RING_LAUNCH
}

hipError_t launch_native_ring_merge(int word, void *terms, void *out, const void *even, const void *odd, bool leaf, uint64_t off_lo,
                                    uint64_t off_hi, unsigned base_log, unsigned levels, uint32_t t, uint32_t shift, int logn, size_t glwe_dim,
                                    size_t h, size_t gs, size_t nct, bool stream, bool lds, hipStream_t st) {
    if (!ring_shape_ok(word, logn, glwe_dim) || (t & 1u) == 0 || t >= (2u << logn) || shift >= (2u << logn) || nct == 0 || h == 0 || nct % h ||
        gs < h || levels == 0 || base_log == 0 || (uint64_t)base_log * levels > 8u * (unsigned)word || (!terms && glwe_dim))
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    if (word == 4) ring_merge_w<uint32_t>(terms, out, even, odd, leaf, off, base_log, levels, t, shift, logn, glwe_dim, h, gs, nct, stream, lds, st);
    else if (word == 8) ring_merge_w<uint64_t>(terms, out, even, odd, leaf, off, base_log, levels, t, shift, logn, glwe_dim, h, gs, nct, stream, lds, st);
    else ring_merge_w<Word128>(terms, out, even, odd, leaf, off, base_log, levels, t, shift, logn, glwe_dim, h, gs, nct, stream, lds, st);
    return hipGetLastError();
}

}  // namespace cntt
