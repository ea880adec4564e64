// Part of host_native_ext.hip (included at its end, after host_native_cmux.inc): the native plans' side of the circuit bootstrap from LWE
// bits to GGSW selectors (include/cntt_cbs.h), of the many-LUT bootstrap and of the circuit bootstrap with one rotation per input bit
// (include/cntt_manylut.h) -- the members of NativePbs that cbs_host.hpp asks for, over the kernels of native_cbs.hpp and
// native_manylut.hpp (launched by native_cbs.hip and native_manylut.hip), native_split_device and native_ntt_device, and the C ABI.  The
// checks, the workspace and the launch sequences are cbs_host.hpp's, shared with the prime plans.
#include "../../include/cntt_cbs.h"
#include "../../include/cntt_manylut.h"
#include "native_cbs.hpp"
#include "native_manylut.hpp"

#pragma GCC visibility push(hidden)

int NativePbs::cbs_plan_check(const cntt_native *pl) {
    if (pl->info.binary)
        return fail(CNTT_EINVAL, "plan is of a native_binary kind: a produced selector has full-width words, and the exactness of these kinds rests on "
                                 "0/1 key words");
    return CNTT_OK;
}
int NativePbs::cbs_budget_check(const cntt_native *pl, unsigned cbs_base_log, unsigned cbs_levels) {
    const unsigned wbits = digit_bits(pl);
    if ((uint64_t)cbs_base_log * cbs_levels > wbits - 1)
        return fail(CNTT_EINVAL, "cbs_base_log * cbs_levels = %u * %u exceeds w - 1 = %u: H = 2^(w - cbs_base_log * cbs_levels) / 2 must be a word, "
                                 "and 2 has no inverse mod 2^w", cbs_base_log, cbs_levels, wbits - 1);
    return CNTT_OK;
}
// the extraction owns 16 bytes of a row per thread
int NativePbs::extract_many_check(const cntt_native *pl) {
    if (pl->n * (size_t)pl->info.word < 16)
        return fail(CNTT_EINVAL, "ntt_size = %zu words of %d bytes are below the 16 bytes one thread of the extraction owns", pl->n, pl->info.word);
    return CNTT_OK;
}

#define CBS_PLANES(s) {s "[0]", s "[1]", s "[2]", s "[3]", s "[4]", s "[5]", s "[6]", s "[7]", s "[8]", s "[9]"}
static const char *const CBS_OUT[10] = CBS_PLANES("ggsw_ntt_out");
static const char *const CBS_BSK[10] = CBS_PLANES("bsk_ntt");
#undef CBS_PLANES
// how the key and the output appear among the operands: one plane per prime
int NativePbs::bsk_operands(const cntt_native *pl, Operand *ops, int cnt, Key bsk, size_t kb) {
    for (int i = 0; i < pl->info.nprimes && kb; ++i) ops[cnt++] = {CBS_BSK[i], bsk[i], kb, pl->rbytes(), false};
    return cnt;
}
int NativePbs::cbs_out_planes(const cntt_native *pl, CbsOut out, void **planes, const char **names) {
    std::copy(out, out + pl->info.nprimes, planes);
    std::copy(CBS_OUT, CBS_OUT + pl->info.nprimes, names);
    return pl->info.nprimes;
}

hipError_t NativePbs::launch_modswitch_manylut(const cntt_native *pl, uint32_t *rot_t, const void *lwe, unsigned log_lut, size_t lwe_dim,
                                               size_t batch, unsigned grid, hipStream_t st) {
    return launch_native_modswitch_manylut(pl->info.word, rot_t, lwe, native_logn(pl), log_lut, lwe_dim, batch, grid, st);
}
hipError_t NativePbs::launch_extract_many(const cntt_native *pl, void *lwe_out, const void *glwe, size_t k, size_t count, size_t batch,
                                          bool stream, unsigned grid, hipStream_t st) {
    return launch_native_sample_extract_many(pl->info.word, lwe_out, glwe, native_logn(pl), k, count, batch, stream, grid, st);
}
hipError_t NativePbs::launch_cbs_setup(const cntt_native *pl, uint32_t *rot_t, void *table, const void *lwe, const CbsConst &C,
                                       const unsigned *log_lut, size_t lwe_dim, size_t rotations, unsigned grid, hipStream_t st) {
    if (log_lut) return launch_native_cbs_manylut_setup(pl->info.word, rot_t, table, lwe, C, *log_lut, lwe_dim, rotations, grid, st);
    return launch_native_cbs_setup(pl->info.word, rot_t, table, lwe, C, lwe_dim, rotations, grid, st);
}
hipError_t NativePbs::launch_cbs_extract(const cntt_native *pl, int32_t *digits, const void *acc, unsigned ks_base_log, unsigned ks_levels,
                                         const CbsConst &C, bool one_rotation, size_t rotations, unsigned grid, hipStream_t st) {
    const u128 off = gadget_offset(digit_bits(pl), ks_base_log, ks_levels);
    return (one_rotation ? launch_native_cbs_manylut_extract : launch_native_cbs_extract)(pl->info.word, digits, acc, (uint64_t)off,
                                                                                          (uint64_t)(off >> 64), ks_base_log, ks_levels, C,
                                                                                          rotations, grid, st);
}
hipError_t NativePbs::launch_cbs_ks(const cntt_native *pl, void *part, const int32_t *digits, const void *fpksk, size_t k, size_t rows,
                                    size_t elements, const CbsShape &shape, unsigned, hipStream_t st) {
    return launch_native_cbs_ks(pl->info.word, part, digits, fpksk, native_logn(pl), k, rows, elements, shape, st);
}
hipError_t NativePbs::launch_cbs_sum(const cntt_native *pl, void *sel, const void *part, size_t k, unsigned cbs_levels, size_t elements,
                                     size_t slabs, unsigned grid, hipStream_t st) {
    return launch_native_cbs_sum(pl->info.word, sel, part, native_logn(pl), k, cbs_levels, elements, slabs, grid, st);
}
// the selector words into the caller's planes: the two steps of cntt_native_fwd_batch
int NativePbs::cbs_finish(const cntt_native *pl, void *const *out, const void *sel, size_t polys, hipStream_t st) {
    if (int rc = native_split_device(pl, sel, out, polys * pl->n, false, st)) return rc;
    return native_ntt_device(pl, out, polys, false, st);
}
#pragma GCC visibility pop

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------
extern "C" int cntt_native_circuit_bootstrap_batch(const cntt_native_t *pl, void *const *ggsw_ntt_out, const void *lwe_in,
                                                   const void *const *bsk_ntt, const void *fpksk, size_t lwe_dim, size_t glwe_dim,
                                                   unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                   unsigned cbs_base_log, unsigned cbs_levels, size_t batch, void *workspace,
                                                   size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return circuit_bootstrap<NativePbs>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                        ks_levels, cbs_base_log, cbs_levels, nullptr, batch, workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" size_t cntt_native_circuit_bootstrap_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim, unsigned pbs_levels,
                                                                unsigned ks_levels, unsigned cbs_levels, size_t batch) {
    return cbs_workspace_bytes<NativePbs>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch, false);
}
extern "C" unsigned cntt_native_cbs_grid(size_t items, int logn, size_t word_bytes) { return native_cbs_grid(items, logn, word_bytes); }

extern "C" int cntt_native_lwe_modswitch_manylut_batch(const cntt_native_t *pl, uint32_t *rot_t, const void *lwe, size_t lwe_dim,
                                                       unsigned log_lut_count, size_t batch, cntt_mem_t where, void *stream) {
    return lwe_modswitch_manylut<NativePbs>(pl, rot_t, lwe, lwe_dim, log_lut_count, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_sample_extract_many_batch(const cntt_native_t *pl, void *lwe_out, const void *glwe, size_t glwe_dim, size_t count,
                                                     size_t batch, cntt_mem_t where, void *stream) {
    return sample_extract_many<NativePbs>(pl, lwe_out, glwe, glwe_dim, count, batch, where, (hipStream_t)stream);
}
extern "C" int cntt_native_bootstrap_manylut_batch(const cntt_native_t *pl, void *lwe_out, const void *lwe_in, const void *lut,
                                                   int lut_per_element, const void *const *bsk_ntt, size_t lwe_dim, size_t glwe_dim,
                                                   unsigned base_log, unsigned levels, unsigned log_lut_count, size_t lut_count, size_t batch,
                                                   void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return bootstrap_manylut<NativePbs>(pl, lwe_out, lwe_in, lut, lut_per_element, bsk_ntt, lwe_dim, glwe_dim, base_log, levels, log_lut_count,
                                        lut_count, batch, workspace, workspace_bytes, where, (hipStream_t)stream);
}
extern "C" int cntt_native_circuit_bootstrap_manylut_batch(const cntt_native_t *pl, void *const *ggsw_ntt_out, const void *lwe_in,
                                                           const void *const *bsk_ntt, const void *fpksk, size_t lwe_dim, size_t glwe_dim,
                                                           unsigned pbs_base_log, unsigned pbs_levels, unsigned ks_base_log, unsigned ks_levels,
                                                           unsigned cbs_base_log, unsigned cbs_levels, unsigned log_lut_count, size_t batch,
                                                           void *workspace, size_t workspace_bytes, cntt_mem_t where, void *stream) {
    return circuit_bootstrap<NativePbs>(pl, ggsw_ntt_out, lwe_in, bsk_ntt, fpksk, lwe_dim, glwe_dim, pbs_base_log, pbs_levels, ks_base_log,
                                        ks_levels, cbs_base_log, cbs_levels, &log_lut_count, batch, workspace, workspace_bytes, where,
                                        (hipStream_t)stream);
}
extern "C" size_t cntt_native_circuit_bootstrap_manylut_workspace_bytes(const cntt_native_t *pl, size_t lwe_dim, size_t glwe_dim,
                                                                        unsigned pbs_levels, unsigned ks_levels, unsigned cbs_levels,
                                                                        size_t batch) {
    return cbs_workspace_bytes<NativePbs>(pl, lwe_dim, glwe_dim, pbs_levels, ks_levels, cbs_levels, batch, true);
}
