// capi_order.h — the launch lines of the launch-order stage (aux_kernels.hip and the compact kernel's dry run), one function per
// kernel: the batch calls (capi.hip), the bitmap-fed driver (capi_drivers.hip) and the analysis library's dump (lzf_debug_order,
// capi_drivers.hip) all launch through these, so what the dump observes is the grid and the arguments the product uses.
// Enqueue only; LZF_OK or the launch's error.
#pragma once
#include "capi_internal.h"
#include "kernels.h"

namespace lzf_capi __attribute__((visibility("hidden"))) {

// est[j] of every decompress job: sequences sampled in three windows + input_len >> len_shift (one wavefront per job)
inline int launch_decompress_cost(const lzf_decompress_job* d_jobs, uint32_t n, uint32_t* est, uint32_t len_shift, hipStream_t st) {
    LAUNCH(lzf::lzf_decompress_cost_kernel, dim3(n), dim3(64), 0, st, d_jobs, n, est, len_shift);
    return LZF_OK;
}
// perm[] = the jobs by est[], largest first (one workgroup of 1024 threads, as the two below)
inline int launch_order_by_estimate(const uint32_t* est, uint32_t* perm, uint32_t n, hipStream_t st) {
    LAUNCH(lzf::lzf_order_by_estimate_kernel, dim3(1), dim3(1024), 0, st, est, perm, n);
    return LZF_OK;
}
inline int launch_order_by_input_len(const lzf_decompress_job* d_jobs, uint32_t* perm, uint32_t n, hipStream_t st) {
    LAUNCH(lzf::lzf_order_by_input_len_kernel, dim3(1), dim3(1024), 0, st, d_jobs, perm, n);
    return LZF_OK;
}
// the compress probes: `parts` probe jobs per job cut from its payload, then their dry run (results[].reserved = work of a probe)
inline int launch_cost_probes(const lzf_compress_job* d_jobs, lzf_compress_job* probes, lzf_job_result* probe_results, uint32_t n, uint32_t piece, uint32_t parts, hipStream_t st) {
    const size_t n_probes = (size_t)n * parts;
    LAUNCH(lzf::lzf_cost_probe_jobs_kernel, dim3((uint32_t)((n_probes + 255u) / 256u)), dim3(256), 0, st, d_jobs, probes, n, piece, parts);
    LAUNCH(lzf::lzf_compress_compact_kernel<true>, dim3((uint32_t)n_probes), dim3(64), 0, st, (const lzf_compress_job*)probes, probe_results, (uint32_t)n_probes, (const uint32_t*)nullptr, 0u);
    return LZF_OK;
}
inline int launch_order_by_cost(const lzf_compress_job* d_jobs, const lzf_job_result* probe_results, uint32_t* perm, uint32_t n, uint32_t piece, uint32_t parts, hipStream_t st) {
    LAUNCH(lzf::lzf_order_by_cost_kernel, dim3(1), dim3(1024), 0, st, d_jobs, probe_results, perm, n, piece, parts);
    return LZF_OK;
}

}  // namespace lzf_capi
