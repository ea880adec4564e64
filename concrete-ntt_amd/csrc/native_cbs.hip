// kernel instantiations and launchers of the native plans' circuit bootstrap (native_cbs.hpp): u32 / u64 / Word128 words
#include "native_cbs.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W cbs_word(U128 v) { return (W)v; }
template <> Word128 cbs_word<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

// f(W{}) for the word type of `word` bytes
template <class F> static void with_cbs_word(int word, F &&f) {
    if (word == 4) f(uint32_t{});
    else if (word == 8) f(uint64_t{});
    else f(Word128{});
}
static bool cbs_word_ok(int word) { return word == 4 || word == 8 || word == 16; }

hipError_t launch_native_cbs_setup(int word, uint32_t *rot_t, void *table, const void *lwe, const NativeCbsConst &C, size_t lwe_dim,
                                   size_t elements, unsigned grid, hipStream_t st) {
    // logn: a thread owns 16 bytes of the table, and ms() reads logn + 2 of the top 32 bits; H_l must be a word
    if (!cbs_word_ok(word) || C.logn < 2 || C.logn > 30 || elements == 0 || C.cbs_levels == 0 || elements % C.cbs_levels || C.cbs_base_log == 0 ||
        (uint64_t)C.cbs_base_log * C.cbs_levels > 8u * (unsigned)word - 1u)
        return hipErrorInvalidValue;
    with_cbs_word(word, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_cbs_setup_kernel<W>), dim3(grid), dim3(256), 0, st, rot_t, (W *)table, (const W *)lwe, C, lwe_dim, elements);
    });
    return hipGetLastError();
}

hipError_t launch_native_cbs_extract(int word, int32_t *digits, const void *acc, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                     unsigned levels, const NativeCbsConst &C, size_t elements, unsigned grid, hipStream_t st) {
    const unsigned wbits = 8u * (unsigned)word;
    if (!cbs_word_ok(word) || elements == 0 || levels == 0 || base_log == 0 || base_log > 31 || (uint64_t)base_log * levels > wbits ||
        C.cbs_levels == 0 || elements % C.cbs_levels || (uint64_t)C.cbs_base_log * C.cbs_levels > wbits - 1u)
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    with_cbs_word(word, [&](auto w) {
        using W = decltype(w);
        GadgetConst<W> G{};   // (npolys, rotated, cmux: the source fields of native_gadget_kernel, not read here)
        G.off = cbs_word<W>(off);
        G.mask = cbs_word<W>(((U128)1 << base_log) - 1);
        G.half = cbs_word<W>((U128)1 << (base_log - 1));
        G.base_log = base_log;
        G.levels = levels;
        hipLaunchKernelGGL((native_cbs_extract_kernel<W>), dim3(grid), dim3(256), 0, st, digits, (const W *)acc, G, C, elements);
    });
    return hipGetLastError();
}

hipError_t launch_native_cbs_ks(int word, void *part, const int32_t *digits, const void *key, int logn, size_t glwe_dim, size_t rows,
                                size_t elements, const NativeCbsShape &Z, hipStream_t st) {
    // the shape must cover the rows, the elements and the columns it is launched for; the key is read in 16-byte vectors
    if (!cbs_word_ok(word) || logn < 2 || logn > 30 || rows == 0 || elements == 0 || glwe_dim + 1 >= ((size_t)1 << 32) || Z.rows == 0 ||
        Z.rows * Z.slabs < rows || Z.tiles * NCBS_ET < elements || Z.cols * 256 * (16 / (size_t)word) < ((glwe_dim + 1) << logn) ||
        (uintptr_t)key % 16 || (uintptr_t)part % 16)
        return hipErrorInvalidValue;
    const dim3 grid(native_cbs_grid(Z.items(glwe_dim), logn, (size_t)word));
    with_cbs_word(word, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_cbs_ks_kernel<W>), grid, dim3(256), 0, st, (W *)part, digits, (const W *)key, (uint32_t)logn, (uint32_t)glwe_dim,
                           rows, elements, Z);
    });
    return hipGetLastError();
}

hipError_t launch_native_cbs_sum(int word, void *sel, const void *part, int logn, size_t glwe_dim, unsigned cbs_levels, size_t elements,
                                 size_t slabs, unsigned grid, hipStream_t st) {
    if (!cbs_word_ok(word) || elements == 0 || slabs == 0 || cbs_levels == 0 || elements % cbs_levels) return hipErrorInvalidValue;
    with_cbs_word(word, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_cbs_sum_kernel<W>), dim3(grid), dim3(256), 0, st, (W *)sel, (const W *)part, (uint32_t)logn, (uint32_t)glwe_dim,
                           (uint32_t)cbs_levels, elements, slabs);
    });
    return hipGetLastError();
}

}  // namespace cntt
