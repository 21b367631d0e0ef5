// capi_internal.h — what the translation units behind include/lzfear_hip.h share: capi.hip (the extern "C" device entry
// points), capi_head.hip (the head call), capi_drivers.hip (the segmented and bitmap-fed decompress drivers) and capi_host.cpp
// (the host-buffer wrappers).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include "lzfear_hip.h"
#include "lzf_dispatch.h"

namespace lzf { struct seg_job; }

// (hidden: the library exports the C entry points of lzfear_hip.h and nothing of this)
namespace lzf_capi __attribute__((visibility("hidden"))) {

extern thread_local std::string g_last_error;

inline int fail_hip(hipError_t e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_last_error = buf;
    return LZF_E_HIP;
}
#define HIP_TRY(expr)                                                    \
    do {                                                                 \
        hipError_t e__ = (expr);                                         \
        if (e__ != hipSuccess) return lzf_capi::fail_hip(e__, #expr);    \
    } while (0)
// a kernel launch and its launch status (a failed launch must not pass for an empty result array)
#define LAUNCH(...)                                            \
    do {                                                       \
        hipLaunchKernelGGL(__VA_ARGS__);                       \
        HIP_TRY(hipGetLastError());                            \
    } while (0)
// the same where a failed launch must still clean up: rc = the status, and the code goes on
#define LAUNCH_RC(rc, ...)                                     \
    do {                                                       \
        hipLaunchKernelGGL(__VA_ARGS__);                       \
        const hipError_t e__ = hipGetLastError();              \
        if (e__ != hipSuccess) (rc) = lzf_capi::fail_hip(e__, "kernel launch"); \
    } while (0)

int ensure_device();         // the number of devices, or LZF_E_NO_DEVICE
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// stream-ordered scratch of a batch call: handed back to the pool on every way out of the call (a failed launch included)
struct AsyncScratch {
    void* p = nullptr; hipStream_t st = nullptr;
    explicit AsyncScratch(hipStream_t s) : st(s) {}
    AsyncScratch(const AsyncScratch&) = delete;
    AsyncScratch& operator=(const AsyncScratch&) = delete;
    ~AsyncScratch() { if (p) { (void)hipFreeAsync(p, st); } }
    // false (and nothing held) when the pool has no room: every user has a way to do without
    bool alloc(size_t bytes) { if (hipMallocAsync(&p, bytes, st) != hipSuccess) { (void)hipGetLastError(); p = nullptr; } return p != nullptr; }
    uint8_t* at(uint64_t off) const { return static_cast<uint8_t*>(p) + off; }
    hipError_t release() { void* q = p; p = nullptr; return q ? hipFreeAsync(q, st) : hipSuccess; }
};

// the tuning values: the defaults in the product; in the analysis library filled once per process from the environment (analysis/capi_analysis.inc)
const lzf_dispatch::Knobs& knobs();

// the streams and events of grouped calls of the segmented pipeline: made once per device, kept; calls enqueue under the mutex (the work itself overlaps freely)
struct SegLanes {
    std::mutex mu;
    hipStream_t s[lzf_dispatch::kSegMaxGroups - 1u] = {};
    hipEvent_t front[lzf_dispatch::kSegMaxGroups - 1u] = {}, done[lzf_dispatch::kSegMaxGroups - 1u] = {};
    bool made = false, ok = false;
};
// What the library knows about a device, by device number, under one mutex.  A process that moves between devices gets every
// device's own record.  (A stream belongs to the device that was current when it was made.)  A call takes its record once and
// hands it down; what is worked out late (pool, census, residency, lanes) is read and written under device_mutex(), which is
// never held across a wait for the device.
struct Device {
    lzf_dispatch::Geometry geo;      // as the runtime reports it (knobs().fake_cu applied); never changes
    bool pool_kept = false;          // the default memory pool keeps its memory over synchronisation points
    uint32_t fed_slots = 0, fed_xcc_mask = 0;        // workgroups of the fed kernel resident at once, counted; 0: not counted yet
    uint32_t size_resident = 0;      // workgroups of the size kernel per CU (0: not asked yet)
    uint32_t verify_resident = 0;    // ... and of the verify kernel
    uint32_t head_resident = 0;      // ... and of the head kernel (capi_head.hip)
    SegLanes lanes;
    bool spare = false;              // the one record of device numbers beyond the table: nothing is kept in it
};
std::mutex& device_mutex();
Device& device();                    // the current device's record (made at the first call; device 0's when the runtime names none)
void keep_pool_memory(Device& dv);
SegLanes* seg_lanes(Device& dv);     // null when the streams could not be made

// capi_drivers.hip.  *used = false: the path declined the call and launched nothing.
int seg_decompress(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const lzf_dispatch::DecompressPlan& plan, hipStream_t st, bool* used, uint64_t max_in_hint);
int fed_decompress(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, uint32_t* perm, uint32_t* est, hipStream_t st, bool* used, uint64_t max_in_hint);
// the front of the size call's latency class: scratch into `mem` (the caller frees it behind the one-wave kernel), plan .. finish.
// *done = the state array the one-wave kernel skips by, or null: the pool refused the scratch and nothing was launched.
int size_seg_front(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const lzf_dispatch::SizePlan& plan, AsyncScratch& mem, hipStream_t st,
                   const lzf::seg_job** done, uint64_t max_in_hint);

// the same for the verify call's latency class (plan .. the verdicts of the jobs of clean tiles)
int verify_seg_front(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const lzf_dispatch::VerifyPlan& plan, AsyncScratch& mem, hipStream_t st,
                     const lzf::seg_job** done, uint64_t max_in_hint);

}  // namespace lzf_capi
