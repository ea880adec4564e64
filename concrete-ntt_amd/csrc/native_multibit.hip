// the kernel instance and the launcher of the native plans' multi-bit accumulate (native_multibit.hpp): 32-bit residues, all planes of a
// plan in one launch
#include "native_multibit.hpp"

namespace cntt {

hipError_t launch_native_multibit_accumulate(const MultibitPlanes &A, unsigned nplanes, const uint32_t *rot_rows, int logn, size_t nterms,
                                             size_t nout, unsigned grouping, size_t batch, hipStream_t st) {
    if (grouping == 0 || grouping > NATIVE_MULTIBIT_MAX_GROUPING || nplanes == 0 || nplanes > NATIVE_MULTIBIT_MAX_PLANES || logn < 5 ||
        logn > 30 || batch == 0 || nout == 0 || nterms == 0 || nterms >= ((size_t)1 << 32) || nout >= ((size_t)1 << 32))
        return hipErrorInvalidValue;
    for (unsigned i = 0; i < nplanes; ++i)
        if (A.p[i] >= NATIVE_MULTIBIT_PRIME_BOUND || !(A.p[i] & 1u)) return hipErrorInvalidValue;   // the lazy sum's range
    const size_t vectors = (batch * nout) << (logn - 2);
    hipLaunchKernelGGL((native_multibit_accumulate_kernel<uint32_t>), dim3(native_multibit_grid(vectors), nplanes), dim3(256), 0, st, A, rot_rows,
                       (uint32_t)logn, (uint32_t)nterms, (uint32_t)nout, (uint32_t)grouping, batch);
    return hipGetLastError();
}

}  // namespace cntt
