// kernel instantiations and launchers of the native plans' many-LUT bootstrap and one-rotation circuit bootstrap (native_manylut.hpp):
// u32 / u64 / Word128 words
#include "native_manylut.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W manylut_word(U128 v) { return (W)v; }
template <> Word128 manylut_word<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

// f(W{}) for the word type of `word` bytes
template <class F> static void with_manylut_word(int word, F &&f) {
    if (word == 4) f(uint32_t{});
    else if (word == 8) f(uint64_t{});
    else f(Word128{});
}
static bool manylut_word_ok(int word) { return word == 4 || word == 8 || word == 16; }

hipError_t launch_native_modswitch_manylut(int word, uint32_t *rot_t, const void *lwe, int logn, unsigned log_lut, size_t lwe_dim, size_t batch,
                                           unsigned grid, hipStream_t st) {
    // ms_t() reads logn - t + 2 of the top 32 bits
    if (!manylut_word_ok(word) || logn < 1 || logn > 30 || log_lut > (unsigned)logn || batch == 0) return hipErrorInvalidValue;
    const NativeCbsConst C{(uint32_t)logn, 0u, 0u, 0u};
    with_manylut_word(word, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_modswitch_manylut_kernel<W, false>), dim3(grid), dim3(256), 0, st, rot_t, (W *)nullptr, (const W *)lwe, C,
                           (uint32_t)log_lut, lwe_dim, batch);
    });
    return hipGetLastError();
}

hipError_t launch_native_cbs_manylut_setup(int word, uint32_t *rot_t, void *table, const void *lwe, const NativeCbsConst &C, unsigned log_lut,
                                           size_t lwe_dim, size_t batch, unsigned grid, hipStream_t st) {
    // a thread owns 16 bytes of the table; the levels fit the interleaved table, and the two bit values n / 2 and 3 n / 2 lie on the coarse
    // grid; H_l must be a word
    if (!manylut_word_ok(word) || C.logn < 2 || C.logn > 30 || log_lut + 1u > C.logn || batch == 0 || C.cbs_levels == 0 ||
        C.cbs_levels > (1u << log_lut) || C.cbs_base_log == 0 || (uint64_t)C.cbs_base_log * C.cbs_levels > 8u * (unsigned)word - 1u ||
        (uintptr_t)table % 16)
        return hipErrorInvalidValue;
    with_manylut_word(word, [&](auto w) {
        using W = decltype(w);
        hipLaunchKernelGGL((native_modswitch_manylut_kernel<W, true>), dim3(grid), dim3(256), 0, st, rot_t, (W *)table, (const W *)lwe, C,
                           (uint32_t)log_lut, lwe_dim, batch);
    });
    return hipGetLastError();
}

hipError_t launch_native_sample_extract_many(int word, void *lwe_out, const void *glwe, int logn, size_t glwe_dim, size_t count, size_t batch,
                                             bool stream, unsigned grid, hipStream_t st) {
    // n is a multiple of the 16 / word words of a vector
    if (!manylut_word_ok(word) || logn < 0 || logn > 30 || ((size_t)word << logn) < 16 || count == 0 || count > ((size_t)1 << logn) || batch == 0) return hipErrorInvalidValue;
    with_manylut_word(word, [&](auto w) {
        using W = decltype(w);
        if (stream)
            hipLaunchKernelGGL((native_sample_extract_many_kernel<W, true>), dim3(grid), dim3(256), 0, st, (W *)lwe_out, (const W *)glwe,
                               (uint32_t)logn, glwe_dim, count, batch);
        else
            hipLaunchKernelGGL((native_sample_extract_many_kernel<W, false>), dim3(grid), dim3(256), 0, st, (W *)lwe_out, (const W *)glwe,
                               (uint32_t)logn, glwe_dim, count, batch);
    });
    return hipGetLastError();
}

hipError_t launch_native_cbs_manylut_extract(int word, int32_t *digits, const void *acc, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                             unsigned levels, const NativeCbsConst &C, size_t batch, unsigned grid, hipStream_t st) {
    const unsigned wbits = 8u * (unsigned)word;
    if (!manylut_word_ok(word) || batch == 0 || C.logn < 1 || C.logn > 30 || levels == 0 || base_log == 0 || base_log > 31 ||
        (uint64_t)base_log * levels > wbits || C.cbs_levels == 0 || C.cbs_levels > (1u << (C.logn - 1u)) ||
        (uint64_t)C.cbs_base_log * C.cbs_levels > wbits - 1u)
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    with_manylut_word(word, [&](auto w) {
        using W = decltype(w);
        GadgetConst<W> G{};   // (npolys, rotated, cmux: the source fields of native_gadget_kernel, not read here)
        G.off = manylut_word<W>(off);
        G.mask = manylut_word<W>(((U128)1 << base_log) - 1);
        G.half = manylut_word<W>((U128)1 << (base_log - 1));
        G.base_log = base_log;
        G.levels = levels;
        hipLaunchKernelGGL((native_cbs_manylut_extract_kernel<W>), dim3(grid), dim3(256), 0, st, digits, (const W *)acc, G, C, batch);
    });
    return hipGetLastError();
}

}  // namespace cntt
