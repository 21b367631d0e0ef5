// capi_head.hip — lzf_decompress_head_batch (include/lzfear_hip.h): the first bytes of every job's block, the jobs' out_cap being
// the target.  One launch of lzf_decode_head_kernel (lz4_decode_head.hip), one wavefront per job: as many workgroups as the
// device holds at once draw jobs from a 4-byte counter, the call's only scratch (stream-ordered pool, freed in stream order).
// No launch order: a job costs what its target asks for, not what its input holds.  Enqueue only: no host wait.
#include "capi_internal.h"
#include "lzf_device.h"

namespace lzf {
template <int S, int TOKCAP>
__global__ __launch_bounds__(64) void lzf_decode_head_kernel(const lzf_decompress_job* __restrict__ jobs, lzf_job_result* __restrict__ results,
                                                             uint32_t n_jobs, uint32_t* __restrict__ ticket);
extern template __global__ void lzf_decode_head_kernel<48, 768>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*);
}  // namespace lzf

using namespace lzf_capi;

namespace {
constexpr auto k_head = lzf::lzf_decode_head_kernel<48, 768>;
}

extern "C" int lzf_decompress_head_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_decompress_head_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    uint32_t resident = 0;             // workgroups of the kernel per CU
    {
        std::lock_guard<std::mutex> lk(device_mutex());
        if (!dv.head_resident || dv.spare) {
            int per = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_head, 64, 0));
            dv.head_resident = per > 0 ? (uint32_t)per : 1u;
        }
        resident = dv.head_resident;
    }
    const uint64_t room = (uint64_t)resident * dv.geo.cu;
    AsyncScratch ticket(st);
    HIP_TRY(hipMallocAsync(&ticket.p, 256, st));
    HIP_TRY(hipMemsetAsync(ticket.p, 0, 4, st));
    const uint32_t grid = n_jobs < room ? n_jobs : (uint32_t)room;
    LAUNCH(k_head, dim3(grid), dim3(64), 0, st, d_jobs, d_results, n_jobs, static_cast<uint32_t*>(ticket.p));
    HIP_TRY(ticket.release());
    return LZF_OK;
}
