// kernel instantiations and the launcher of the native plans' CMux (native_cmux.hpp): u32 / u64 / Word128 words
#include "native_cmux.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W cmux_word(U128 v) { return (W)v; }
template <> Word128 cmux_word<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

template <class W>
static void cmux_diff_w(void *terms, void *out, const void *c0, const void *c1, bool leaf, U128 off, unsigned base_log, unsigned levels,
                        int logn, size_t glwe_dim, size_t h, size_t gs, size_t nct, bool stream, hipStream_t st) {
    GadgetConst<W> G{};   // (npolys, rotated, cmux: the source fields of native_gadget_kernel, not read here)
    G.off = cmux_word<W>(off);
    G.mask = cmux_word<W>(base_log == 128 ? ~(U128)0 : ((U128)1 << base_log) - 1);
    G.half = cmux_word<W>((U128)1 << (base_log - 1));
    G.base_log = base_log;
    G.levels = levels;
    const dim3 grid(native_cmux_grid(nct * (glwe_dim + 1), logn, sizeof(W))), block(256);
    const uint32_t ln = (uint32_t)logn, k = (uint32_t)glwe_dim;
#define CNTT_CMUX_LAUNCH(STREAM, LEAF)                                                                                                  \
    hipLaunchKernelGGL((native_cmux_diff_kernel<W, STREAM, LEAF>), grid, block, 0, st, (W *)terms, (W *)out, (const W *)c0, (const W *)c1, G, \
                       ln, k, h, gs, nct)
    if (stream && leaf) CNTT_CMUX_LAUNCH(true, true);
    else if (stream) CNTT_CMUX_LAUNCH(true, false);
    else if (leaf) CNTT_CMUX_LAUNCH(false, true);
    else CNTT_CMUX_LAUNCH(false, false);
#undef CNTT_CMUX_LAUNCH
}

hipError_t launch_native_cmux_diff(int word, void *terms, void *out, const void *c0, const void *c1, bool leaf, uint64_t off_lo,
                                   uint64_t off_hi, unsigned base_log, unsigned levels, int logn, size_t glwe_dim, size_t h, size_t gs,
                                   size_t nct, bool stream, hipStream_t st) {
    const unsigned wbits = 8u * (unsigned)word;
    // logn: a thread owns 16 bytes, so a polynomial is at least one vector of the widest count (4 words)
    if ((word != 4 && word != 8 && word != 16) || logn < 2 || logn > 30 || nct == 0 || h == 0 || nct % h || gs < h ||
        glwe_dim + 1 >= ((size_t)1 << 32) || levels == 0 || base_log == 0 || (uint64_t)base_log * levels > wbits || (!terms && !leaf))
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    if (word == 4) cmux_diff_w<uint32_t>(terms, out, c0, c1, leaf, off, base_log, levels, logn, glwe_dim, h, gs, nct, stream, st);
    else if (word == 8) cmux_diff_w<uint64_t>(terms, out, c0, c1, leaf, off, base_log, levels, logn, glwe_dim, h, gs, nct, stream, st);
    else cmux_diff_w<Word128>(terms, out, c0, c1, leaf, off, base_log, levels, logn, glwe_dim, h, gs, nct, stream, st);
    return hipGetLastError();
}

}  // namespace cntt
