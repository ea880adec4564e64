// kernel instantiations and launchers of the bootstrap's end kernels (native_pbs.hpp): u32 / u64 / Word128 words
#include "native_pbs.hpp"

namespace cntt {

hipError_t launch_native_lwe_modswitch(int word, uint32_t *rot_t, const void *lwe, int logn, size_t lwe_dim, size_t batch, unsigned grid,
                                       hipStream_t st) {
    if (word == 4)
        hipLaunchKernelGGL((native_lwe_modswitch_kernel<uint32_t>), dim3(grid), dim3(256), 0, st, rot_t, (const uint32_t *)lwe, (uint32_t)logn,
                           lwe_dim, batch);
    else if (word == 8)
        hipLaunchKernelGGL((native_lwe_modswitch_kernel<uint64_t>), dim3(grid), dim3(256), 0, st, rot_t, (const uint64_t *)lwe, (uint32_t)logn,
                           lwe_dim, batch);
    else
        hipLaunchKernelGGL((native_lwe_modswitch_kernel<Word128>), dim3(grid), dim3(256), 0, st, rot_t, (const Word128 *)lwe, (uint32_t)logn,
                           lwe_dim, batch);
    return hipGetLastError();
}

template <class W>
static void pbs_init_w(void *acc, const void *lut, const uint32_t *rot, int logn, uint32_t npolys, bool per_element, size_t batch, bool stream,
                       unsigned grid, hipStream_t st) {
    const uint32_t ls = per_element ? npolys : 0u;
    if (stream)
        hipLaunchKernelGGL((native_pbs_init_kernel<W, true>), dim3(grid), dim3(256), 0, st, (W *)acc, (const W *)lut, rot, (uint32_t)logn, npolys,
                           ls, batch * npolys);
    else
        hipLaunchKernelGGL((native_pbs_init_kernel<W, false>), dim3(grid), dim3(256), 0, st, (W *)acc, (const W *)lut, rot, (uint32_t)logn,
                           npolys, ls, batch * npolys);
}
hipError_t launch_native_pbs_init(int word, void *acc, const void *lut, const uint32_t *rot, int logn, uint32_t npolys, bool per_element,
                                  size_t batch, bool stream, unsigned grid, hipStream_t st) {
    if (word == 4) pbs_init_w<uint32_t>(acc, lut, rot, logn, npolys, per_element, batch, stream, grid, st);
    else if (word == 8) pbs_init_w<uint64_t>(acc, lut, rot, logn, npolys, per_element, batch, stream, grid, st);
    else pbs_init_w<Word128>(acc, lut, rot, logn, npolys, per_element, batch, stream, grid, st);
    return hipGetLastError();
}

hipError_t launch_native_sample_extract(int word, void *lwe_out, const void *glwe, int logn, size_t glwe_dim, uint32_t index, size_t batch,
                                        unsigned grid, hipStream_t st) {
    if (word == 4)
        hipLaunchKernelGGL((native_sample_extract_kernel<uint32_t>), dim3(grid), dim3(256), 0, st, (uint32_t *)lwe_out, (const uint32_t *)glwe,
                           (uint32_t)logn, glwe_dim, index, batch);
    else if (word == 8)
        hipLaunchKernelGGL((native_sample_extract_kernel<uint64_t>), dim3(grid), dim3(256), 0, st, (uint64_t *)lwe_out, (const uint64_t *)glwe,
                           (uint32_t)logn, glwe_dim, index, batch);
    else
        hipLaunchKernelGGL((native_sample_extract_kernel<Word128>), dim3(grid), dim3(256), 0, st, (Word128 *)lwe_out, (const Word128 *)glwe,
                           (uint32_t)logn, glwe_dim, index, batch);
    return hipGetLastError();
}

}  // namespace cntt
