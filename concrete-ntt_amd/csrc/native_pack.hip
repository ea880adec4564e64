// kernel instantiations and the launchers of the packing keyswitch (native_pack.hpp): u32 / u64 / Word128 words
#include "native_pack.hpp"

namespace cntt {

using U128 = unsigned __int128;
template <class W> static W pack_word(U128 v) { return (W)v; }
template <> Word128 pack_word<Word128>(U128 v) { return Word128{(uint64_t)v, (uint64_t)(v >> 64)}; }

template <class W>
static void pack_decompose_w(void *terms, const void *in, U128 off, unsigned base_log, unsigned levels, int logn, size_t lin, size_t m,
                             size_t i0, size_t nw, size_t batch, hipStream_t st) {
    constexpr size_t TT = PACK_TT, TI = PackTile<W>::TI;
    PackConst<W> G{};
    G.off = pack_word<W>(off);
    G.mask = pack_word<W>(base_log == 128 ? ~(U128)0 : ((U128)1 << base_log) - 1);
    G.half = pack_word<W>((U128)1 << (base_log - 1));
    G.base_log = base_log;
    G.levels = levels;
    const size_t n = (size_t)1 << logn, tiles = batch * ((n + TT - 1) / TT) * ((nw + TI - 1) / TI);
    const unsigned grid = (unsigned)(tiles < ((size_t)1 << 24) ? tiles : ((size_t)1 << 24) - 1);
    hipLaunchKernelGGL((native_pack_decompose_kernel<W>), dim3(grid), dim3(256), 0, st, (W *)terms, (const W *)in, G, (uint32_t)logn, lin, m,
                       i0, (uint32_t)nw, batch);
}

hipError_t launch_native_pack_decompose(int word, void *terms, const void *in, uint64_t off_lo, uint64_t off_hi, unsigned base_log,
                                        unsigned levels, int logn, size_t lin, size_t m, size_t i0, size_t nw, size_t batch, hipStream_t st) {
    const unsigned wbits = 8u * (unsigned)word;
    if (levels == 0 || base_log == 0 || (uint64_t)base_log * levels > wbits || batch == 0 || nw == 0 || nw >= ((size_t)1 << 32) ||
        i0 + nw > lin || m == 0 || m > ((size_t)1 << logn))
        return hipErrorInvalidValue;
    const U128 off = ((U128)off_hi << 64) | off_lo;
    if (word == 4) pack_decompose_w<uint32_t>(terms, in, off, base_log, levels, logn, lin, m, i0, nw, batch, st);
    else if (word == 8) pack_decompose_w<uint64_t>(terms, in, off, base_log, levels, logn, lin, m, i0, nw, batch, st);
    else pack_decompose_w<Word128>(terms, in, off, base_log, levels, logn, lin, m, i0, nw, batch, st);
    return hipGetLastError();
}

hipError_t launch_native_pack_body(int word, void *out, const void *in, int logn, size_t glwe_dim, size_t lin, size_t m, size_t batch,
                                   unsigned grid, hipStream_t st) {
    if (batch == 0 || m == 0 || m > ((size_t)1 << logn)) return hipErrorInvalidValue;
    if (word == 4)
        hipLaunchKernelGGL((native_pack_body_kernel<uint32_t>), dim3(grid), dim3(256), 0, st, (uint32_t *)out, (const uint32_t *)in,
                           (uint32_t)logn, glwe_dim, lin, m, batch);
    else if (word == 8)
        hipLaunchKernelGGL((native_pack_body_kernel<uint64_t>), dim3(grid), dim3(256), 0, st, (uint64_t *)out, (const uint64_t *)in,
                           (uint32_t)logn, glwe_dim, lin, m, batch);
    else
        hipLaunchKernelGGL((native_pack_body_kernel<Word128>), dim3(grid), dim3(256), 0, st, (Word128 *)out, (const Word128 *)in,
                           (uint32_t)logn, glwe_dim, lin, m, batch);
    return hipGetLastError();
}

}  // namespace cntt
