// capi.hip — the extern "C" device entry points declared in include/lzfear_hip.h: argument checks, the per-device record, the two
// batch calls (which execute a plan of lzf_dispatch.h) and the small launches.  The drivers of the segmented and bitmap-fed paths
// are in capi_drivers.hip, the host-buffer wrappers in capi_host.cpp.  Plain HIP runtime calls + kernel launches; no CPU codec
// anywhere: without a usable HIP device every entry point fails with LZF_E_NO_DEVICE.  The product library reads no environment
// variables; the A/B knobs of the analysis build are one table in analysis/capi_analysis.inc.
#include "capi_internal.h"
#include <cstdlib>
#include "kernels.h"
#include "capi_order.h"

namespace lzf_capi __attribute__((visibility("hidden"))) {
namespace d = lzf_dispatch;

thread_local std::string g_last_error;
namespace {
thread_local const char* g_last_decompress = "";      // what the last lzf_decompress_batch of this thread launched (lzf_last_decompress_launch)
thread_local const char* g_last_compress = "";        // ... and the last lzf_compress_batch
thread_local const char* g_last_size = "";            // ... and the last lzf_decompressed_size_batch
thread_local const char* g_last_verify = "";          // ... and the last lzf_decompress_verify_batch
}

int ensure_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_last_error = "no HIP device available (the lz-fear HIP codec has no CPU fallback)";
        (void)hipGetLastError();
        return LZF_E_NO_DEVICE;
    }
    return n;
}

#ifdef LZF_ANALYSIS
namespace {
#include "analysis/capi_analysis.inc"
}
const d::Knobs& knobs() { static const d::Knobs k = analysis_knobs(); return k; }
#else
const d::Knobs& knobs() { static const d::Knobs k; return k; }
#endif

// ---- the per-device record ---------------------------------------------------------------------------------------------------
std::mutex& device_mutex() { static std::mutex mu; return mu; }
namespace {
// The geometry every dispatch threshold is derived from: compute units and LDS bytes per CU of a device, as the runtime reports
// them (MI355X: 256 and 160 KiB), and the rate of wall_clock64() (s_memrealtime: 100 MHz on MI355X).
d::Geometry read_geometry(int dev) {
    d::Geometry r;
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) == hipSuccess) {
        r.cu = (uint32_t)p.multiProcessorCount;
        if (p.maxSharedMemoryPerMultiProcessor >= 64u * 1024u) r.lds = (uint32_t)p.maxSharedMemoryPerMultiProcessor;
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz >= 1000) r.wall_khz = (uint32_t)khz; else (void)hipGetLastError();
    } else (void)hipGetLastError();      // (only an error of these calls is cleared, never one the caller left pending)
    if (knobs().fake_cu) r.cu = knobs().fake_cu;
    return r;
}
}  // namespace
Device& device() {
    constexpr int kMaxDev = 64;
    static Device* by_dev[kMaxDev + 1] = {};      // (+ one record without kept state for a device number beyond the table)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    const int at = dev >= 0 && dev < kMaxDev ? dev : kMaxDev;
    std::lock_guard<std::mutex> lk(device_mutex());
    if (!by_dev[at]) { by_dev[at] = new Device(); by_dev[at]->geo = read_geometry(dev); by_dev[at]->spare = at == kMaxDev; }
    return *by_dev[at];
}
// The batch calls take their scratch (launch orders, cost probes) from the stream-ordered pool.  By default the pool hands its
// memory back at every synchronisation point, so the next call allocates from the device again — which waits for whatever is
// running.  Keep what the pool has: a later hipMallocAsync on the same stream re-uses it without touching the device.
void keep_pool_memory(Device& dv) {
    std::lock_guard<std::mutex> lk(device_mutex());
    if (dv.pool_kept) return;
    int dev = 0; hipMemPool_t pool = nullptr;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetDefaultMemPool(&pool, dev) == hipSuccess) {
        uint64_t keep = ~0ull;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
    (void)hipGetLastError();
    dv.pool_kept = !dv.spare;
}
SegLanes* seg_lanes(Device& dv) {
    if (dv.spare) return nullptr;
    SegLanes& L = dv.lanes;
    std::lock_guard<std::mutex> lk(device_mutex());
    if (!L.made) {
        // High-priority streams: the runtime keeps a pool of hardware queues PER PRIORITY (four each by default), so these three do not
        // end up sharing a queue with the application's own streams — a resolve stage queued behind the caller's next records stage
        // would serialise the call (measured: 49 blocks 13.4 ms instead of 8.0 with one application side stream alive) — and the
        // resolve stage, the chain of the call, is dispatched ahead of the throughput kernels.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = greatest = 0; }
        bool ok = true;
        for (uint32_t i = 0; i < d::kSegMaxGroups - 1u && ok; ++i)
            ok = hipStreamCreateWithPriority(&L.s[i], hipStreamNonBlocking, greatest) == hipSuccess &&
                 hipEventCreateWithFlags(&L.front[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&L.done[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        L.ok = ok; L.made = true;
    }
    return L.ok ? &L : nullptr;
}

namespace {
static_assert(d::kCompactLds == lzf::kCompactLdsBytes, "lzf_dispatch.h derives the compact kernel's residency from its LDS");
// the kernels of the product dispatch
using lzf::k_paired48; using lzf::k_paired24;
constexpr auto k_staged16 = lzf::lzf_decompress_batched_kernel<4096, 16, 256, true>;
constexpr auto k_compact = lzf::lzf_compress_compact_kernel<false>;
constexpr auto k_compact_dry = lzf::lzf_compress_compact_kernel<true>;
constexpr auto k_general_u32 = lzf::lzf_compress_wave_kernel<LZF_TABLE_U32>;
constexpr auto k_general_u16 = lzf::lzf_compress_wave_kernel<LZF_TABLE_U16>;
constexpr auto k_general_u32_dry = lzf::lzf_compress_wave_kernel<LZF_TABLE_U32, true>;      // the size call's (lzf_compressed_size_batch)
constexpr auto k_general_u16_dry = lzf::lzf_compress_wave_kernel<LZF_TABLE_U16, true>;
constexpr auto k_size = lzf::lzf_decoded_size_kernel<48, 768, false>;
constexpr auto k_verify = lzf::lzf_verify_kernel<48, 768, false>;
constexpr auto k_verify_skip = lzf::lzf_verify_kernel<48, 768, true>;    // behind the latency class: skips what that finished
constexpr auto k_size_skip = lzf::lzf_decoded_size_kernel<48, 768, true>;      // behind the latency class: skips what that finished

// the launch order of a compress or compressed-size call: the cost probe and the order when the plan wants them and the pool has room.
// *perm_out = the order in `scratch`, or null: the caller's order.
int compress_order(const d::CompressPlan& p, const lzf_compress_job* d_jobs, uint32_t n_jobs, AsyncScratch& scratch, hipStream_t st, uint32_t** perm_out) {
    const d::Knobs& kn = knobs();
    // the cost of a compress job is not known from its size: probe (aux_kernels.hip), then longest first
    // (one call over N four-MiB blocks, caller's order against longest first, probe included: 1 020 blocks 287 / 286 ms, 2 040 338 / 293,
    //  3 060 420 / 305, 3 825 440 / 339, 4 590 488 / 357; for thousands of 64 KiB blocks of linked streams the three extra launches were 15 % of the call: bench config5)
    const uint32_t piece = kn.probe_piece, parts = kn.probe_parts;
    const size_t n_probes = (size_t)n_jobs * parts;
    const size_t probes_off = 256;                  // [probe jobs][probe results][perm]
    const size_t res_off = probes_off + align_up(sizeof(lzf_compress_job) * n_probes, 256);
    const size_t perm_off = res_off + align_up(sizeof(lzf_job_result) * n_probes, 256);
    uint32_t* perm = nullptr;
    // (the order is an optimisation: without scratch memory the batch simply runs in the caller's order)
    if (p.want_order && scratch.alloc(perm_off + sizeof(uint32_t) * (size_t)n_jobs)) {
        lzf_compress_job* probes = reinterpret_cast<lzf_compress_job*>(scratch.at(probes_off));
        lzf_job_result* pres = reinterpret_cast<lzf_job_result*>(scratch.at(res_off));
        perm = reinterpret_cast<uint32_t*>(scratch.at(perm_off));
        int rc = launch_cost_probes(d_jobs, probes, pres, n_jobs, piece, parts, st);
        if (rc == LZF_OK) rc = launch_order_by_cost(d_jobs, pres, perm, n_jobs, piece, parts, st);
        if (rc != LZF_OK) return rc;
    }
    *perm_out = perm;
    return LZF_OK;
}

// the launches of lzf_compress_batch: the order, then the kernels
int compress_launches(const d::CompressPlan& p, const lzf_compress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, AsyncScratch& scratch, hipStream_t st) {
    const d::Knobs& kn = knobs();
    uint32_t* perm = nullptr;
    const int orc = compress_order(p, d_jobs, n_jobs, scratch, st, &perm);
    if (orc != LZF_OK) return orc;
    const uint32_t alone = p.fresh_only ? 1u : 0u;
    if (p.kinds & LZF_KINDS_U32) {
#ifdef LZF_DBG_DRY_MAIN      // analysis: results[].reserved = probe batches + sequences of the whole job (no output)
        if (p.use_compact) LAUNCH(k_compact_dry, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, (const uint32_t*)perm, 0u);
#else
        if (p.use_team) {
            LAUNCH(lzf::lzf_compress_team_kernel, dim3(n_jobs), dim3(192), 0, st, d_jobs, d_results, n_jobs, (const uint32_t*)perm, alone);
            // caller-owned tables (linked streams): the same team, compiled with the table carry; it leaves the compact jobs to the kernel above
            if (!p.fresh_only) LAUNCH(lzf::lzf_compress_team_carry_kernel, dim3(n_jobs), dim3(192), 0, st, d_jobs, d_results, n_jobs, (const uint32_t*)perm);
        }
        else if (p.use_compact) LAUNCH(k_compact, dim3(n_jobs), dim3(64), kn.compact_pad_lds, st, d_jobs, d_results, n_jobs, (const uint32_t*)perm, alone);
#endif
        // (behind the team kernel the general kernel skips what that one takes — compact jobs and caller-owned U32 tables — unless a job was handed back)
        if (!p.fresh_only) LAUNCH(k_general_u32, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, p.general_skip, (const uint32_t*)perm);
    }
    if (p.kinds & LZF_KINDS_U16)
        LAUNCH(k_general_u16, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, 0u, (const uint32_t*)perm);
    g_last_compress = p.launch;
    return LZF_OK;
}

// the launches of lzf_compressed_size_batch: the same order, then the dry forms — the compact kernel over the jobs it takes in a
// compress call, the general kernels over the rest.  No latency class: whatever the job count, the team kernel is not launched.
int compressed_size_launches(const d::CompressPlan& p, const lzf_compress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, AsyncScratch& scratch, hipStream_t st) {
    uint32_t* perm = nullptr;
    const int orc = compress_order(p, d_jobs, n_jobs, scratch, st, &perm);
    if (orc != LZF_OK) return orc;
    if (p.kinds & LZF_KINDS_U32) {
        if (p.use_compact) LAUNCH(k_compact_dry, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, (const uint32_t*)perm, p.fresh_only ? 1u : 0u);
        if (!p.fresh_only) LAUNCH(k_general_u32_dry, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, p.use_compact ? 1u : 0u, (const uint32_t*)perm);
    }
    if (p.kinds & LZF_KINDS_U16)
        LAUNCH(k_general_u16_dry, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, 0u, (const uint32_t*)perm);
    return LZF_OK;
}

// the launches of lzf_decompress_batch_sized; perm_mem is handed back by the caller on every way out
int decompress_launches(Device& dv, const d::DecompressPlan& p, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, uint64_t max_input_len, AsyncScratch& perm_mem, hipStream_t st) {
    const d::Knobs& kn = knobs();
    // perm[n] + est[n]: the jobs by their estimated cost, largest first (no room in the pool: the caller's order)
    uint32_t* const perm = p.want_order && perm_mem.alloc(2u * sizeof(uint32_t) * (size_t)n_jobs) ? static_cast<uint32_t*>(perm_mem.p) : nullptr;
    uint32_t* const est = perm ? perm + n_jobs : nullptr;
    // The estimates are sampled by a kernel of their own (three windows per job) — unless the call takes the bitmap-fed path, whose parse
    // counts every job's tokens anyway.  So the sampling waits until the path is known: it runs in front of whatever else is launched.
    // A job's cost: its sequences + a quarter of its compressed bytes (measured: 403 GiB/s with the sequences alone, 414-418 with len >> 4 .. len >> 1)
    bool ordered = false;
    auto order_by_sampling = [&]() -> int {
        if (!perm || ordered) return LZF_OK;
        ordered = true;
        const int rc = launch_decompress_cost(d_jobs, n_jobs, est, kn.order_len_shift, st);
        return rc == LZF_OK ? launch_order_by_estimate(est, perm, n_jobs, st) : rc;
    };
    const uint32_t* const cperm = perm;
    int rc = LZF_OK;
    bool used = false;
#ifdef LZF_ANALYSIS
    if (kn.variant != kVariantAuto) {
        if ((rc = order_by_sampling()) != LZF_OK) return rc;
        g_last_decompress = d::kLaunchVariant;
        return analysis_launch_decompress(kn.variant, d_jobs, d_results, n_jobs, cperm, st);
    }
#endif
    if (p.seg_class && (rc = order_by_sampling()) != LZF_OK) return rc;
    if (p.try_seg) {             // then the pair kernel over the jobs it left (prefix / existing output, errors, sizes outside its window)
        rc = seg_decompress(dv, d_jobs, d_results, n_jobs, p, st, &used, max_input_len);
        if (used) g_last_decompress = p.seg_launch;              // (the ring the call really used)
        if (rc != LZF_OK || used) return rc;
    }
    if (p.try_fed) {
        rc = fed_decompress(dv, d_jobs, d_results, n_jobs, perm, est, st, &used, max_input_len);      // (declines: nothing launched, the order is still to make)
        if (used) g_last_decompress = p.fed_launch;
        if (rc != LZF_OK || used) return rc;
    }
    if ((rc = order_by_sampling()) != LZF_OK) return rc;
    g_last_decompress = p.last_launch;
    if (p.last == d::kPaired48) LAUNCH(k_paired48, dim3(n_jobs), dim3(128), 0, st, d_jobs, d_results, n_jobs, cperm, (const lzf::seg_job*)nullptr);
    else if (p.last == d::kPaired24) LAUNCH(k_paired24, dim3(n_jobs), dim3(128), 0, st, d_jobs, d_results, n_jobs, cperm, (const lzf::seg_job*)nullptr);
    else LAUNCH(k_staged16, dim3(n_jobs), dim3(64), 0, st, d_jobs, d_results, n_jobs, cperm);
    return LZF_OK;
}

}  // namespace
}  // namespace lzf_capi

using namespace lzf_capi;

extern "C" {

int lzf_abi_version(void) { return LZFEAR_ABI_VERSION; }
const char* lzf_last_error(void) { return g_last_error.c_str(); }
const char* lzf_last_decompress_launch(void) { return g_last_decompress; }
const char* lzf_last_compress_launch(void) { return g_last_compress; }
const char* lzf_last_size_launch(void) { return g_last_size; }
const char* lzf_last_verify_launch(void) { return g_last_verify; }
int lzf_device_count(void) { return ensure_device(); }

// Launch order (both batch calls): a batch of more jobs than the chip holds at once runs longest job first, or the launch
// ends with a few long jobs running alone.  The order is internal — results[i] always belongs to jobs[i].
int lzf_compress_batch(const lzf_compress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs,
                       uint32_t table_kinds, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_compress_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    AsyncScratch scratch(st);
    rc = compress_launches(d::compress_plan(dv.geo, knobs(), n_jobs, table_kinds), d_jobs, d_results, n_jobs, scratch, st);
    HIP_TRY(scratch.release());
    return rc;
}

// compress2's status and the bytes it would write for every job, nothing written: the plan of lzf_compress_batch without its latency
// class, executed with the dry kernels.  `out` is never dereferenced; out_cap, the tables and table_kinds mean what they mean there.
// Enqueue only: no host wait.  (lzf_last_compress_launch is left alone: it speaks of the last lzf_compress_batch.)
int lzf_compressed_size_batch(const lzf_compress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs,
                              uint32_t table_kinds, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_compressed_size_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    AsyncScratch scratch(st);
    rc = compressed_size_launches(d::compress_plan(dv.geo, knobs(), n_jobs, table_kinds), d_jobs, d_results, n_jobs, scratch, st);
    HIP_TRY(scratch.release());
    return rc;
}

int lzf_decompress_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, void* hip_stream) {
    return lzf_decompress_batch_sized(d_jobs, d_results, n_jobs, ~0ull, hip_stream);
}

int lzf_decompress_batch_sized(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, uint64_t max_input_len, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_decompress_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    AsyncScratch perm_mem(st);
    rc = decompress_launches(dv, d::decompress_plan(dv.geo, knobs(), n_jobs, max_input_len), d_jobs, d_results, n_jobs, max_input_len, perm_mem, st);
    HIP_TRY(perm_mem.release());
    return rc;
}

// decompress_raw's status and output.len() of every job, nothing decoded.  The call executes lzf_dispatch.h's size_plan:
//   * few large blocks (the latency class): plan, parse and seam of the segmented pipeline, the tiles summed up, every job's tiles
//     added up and checked (lz4_decoded_size_seg.hip) — scratch from the stream-ordered pool, about 1.2 bits per byte of
//     max_input_len x n_jobs, freed in stream order; a pool that refuses it only sends the call down the other way;
//   * always last: lzf_decoded_size_kernel (lz4_decoded_size.hip), one wavefront per job, over the whole call; behind the class it skips
//     the jobs that finished there.  As many workgroups as the device holds at once draw jobs from a 4-byte counter; with more jobs
//     than that, in the order of their input lengths, longest first (4 bytes per job).
// Enqueue only: no host wait.
int lzf_decompressed_size_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, uint64_t max_input_len, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_decompressed_size_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    const d::SizePlan plan = d::size_plan(dv.geo, knobs(), n_jobs, max_input_len);
    AsyncScratch seg_mem(st);
    const lzf::seg_job* done = nullptr;
    if (plan.try_seg && (rc = size_seg_front(dv, d_jobs, d_results, n_jobs, plan, seg_mem, st, &done, max_input_len)) != LZF_OK) return rc;
    g_last_size = done ? plan.seg_launch : plan.last_launch;
    if (done && !plan.last) { HIP_TRY(seg_mem.release()); return LZF_OK; }
    uint32_t resident = 0;             // workgroups of the kernel per CU
    {
        std::lock_guard<std::mutex> lk(device_mutex());
        if (!dv.size_resident || dv.spare) {
            int per = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_size, 64, 0));
            dv.size_resident = per > 0 ? (uint32_t)per : 1u;
        }
        resident = dv.size_resident;
    }
    const uint64_t room = (uint64_t)resident * dv.geo.cu;
    const bool ordered = n_jobs > room;              // more jobs than resident waves: longest input first (4 bytes per job of scratch)
    AsyncScratch ticket(st);
    HIP_TRY(hipMallocAsync(&ticket.p, 256 + (ordered ? sizeof(uint32_t) * (size_t)n_jobs : 0u), st));
    HIP_TRY(hipMemsetAsync(ticket.p, 0, 4, st));
    uint32_t* const perm = ordered ? static_cast<uint32_t*>(ticket.p) + 64 : nullptr;
    if (ordered && (rc = launch_order_by_input_len(d_jobs, perm, n_jobs, st)) != LZF_OK) return rc;
    const uint32_t grid = n_jobs < room ? n_jobs : (uint32_t)room;
    if (done) LAUNCH(k_size_skip, dim3(grid), dim3(64), 0, st, d_jobs, d_results, n_jobs, static_cast<uint32_t*>(ticket.p), (const uint32_t*)perm, done);
    else LAUNCH(k_size, dim3(grid), dim3(64), 0, st, d_jobs, d_results, n_jobs, static_cast<uint32_t*>(ticket.p), (const uint32_t*)perm, (const lzf::seg_job*)nullptr);
    HIP_TRY(ticket.release());
    HIP_TRY(seg_mem.release());
    return LZF_OK;
}

// Does every job decode to the bytes its `out` holds?  The call executes lzf_dispatch.h's verify_plan, the size call's arrangement:
//   * few large blocks (the latency class): the size call's front and tile sums, then every tile's base, the compares tile by tile
//     and the verdicts of the jobs of clean tiles (lz4_verify.hip); a pool that refuses the scratch sends the call down the other way;
//   * always last: lzf_verify_kernel, one wavefront per job over the whole call, skipping what the class finished; launched as the
//     size call launches its one-wave kernel (a 4-byte job counter; longest input first beyond one residency, 4 bytes per job).
// Enqueue only: no host wait.
int lzf_decompress_verify_batch(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n_jobs, uint64_t max_input_len, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_results) { g_last_error = "lzf_decompress_verify_batch: NULL job/result array"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Device& dv = device();
    keep_pool_memory(dv);
    const d::VerifyPlan plan = d::verify_plan(dv.geo, knobs(), n_jobs, max_input_len);
    AsyncScratch seg_mem(st);
    const lzf::seg_job* done = nullptr;
    if (plan.try_seg && (rc = verify_seg_front(dv, d_jobs, d_results, n_jobs, plan, seg_mem, st, &done, max_input_len)) != LZF_OK) return rc;
    g_last_verify = done ? plan.seg_launch : plan.last_launch;
    uint32_t resident = 0;             // workgroups of the kernel per CU
    {
        std::lock_guard<std::mutex> lk(device_mutex());
        if (!dv.verify_resident || dv.spare) {
            int per = 0;
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, k_verify, 64, 0));
            dv.verify_resident = per > 0 ? (uint32_t)per : 1u;
        }
        resident = dv.verify_resident;
    }
    const uint64_t room = (uint64_t)resident * dv.geo.cu;
    const bool ordered = n_jobs > room;
    AsyncScratch ticket(st);
    HIP_TRY(hipMallocAsync(&ticket.p, 256 + (ordered ? sizeof(uint32_t) * (size_t)n_jobs : 0u), st));
    HIP_TRY(hipMemsetAsync(ticket.p, 0, 4, st));
    uint32_t* const perm = ordered ? static_cast<uint32_t*>(ticket.p) + 64 : nullptr;
    if (ordered && (rc = launch_order_by_input_len(d_jobs, perm, n_jobs, st)) != LZF_OK) return rc;
    const uint32_t grid = n_jobs < room ? n_jobs : (uint32_t)room;
    if (done) LAUNCH(k_verify_skip, dim3(grid), dim3(64), 0, st, d_jobs, d_results, n_jobs, static_cast<uint32_t*>(ticket.p), (const uint32_t*)perm, done);
    else LAUNCH(k_verify, dim3(grid), dim3(64), 0, st, d_jobs, d_results, n_jobs, static_cast<uint32_t*>(ticket.p), (const uint32_t*)perm, (const lzf::seg_job*)nullptr);
    HIP_TRY(ticket.release());
    HIP_TRY(seg_mem.release());
    return LZF_OK;
}

int lzf_table_seed_from_dictionary(lzf_u32_table* d_table, const uint8_t* d_dict, uint64_t dict_len, void* hip_stream) {
    if (!d_table || (!d_dict && dict_len)) { g_last_error = "lzf_table_seed_from_dictionary: NULL argument"; return LZF_E_INVALID; }
    if (dict_len > 0xFFFFFFFFull) { g_last_error = "dictionary beyond u32 positions (reference panics, mod.rs:67)"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(d_table, 0, sizeof(lzf_u32_table), st));   // U32Table::default()
    if (dict_len >= 8) {
        const uint64_t count = (dict_len - 8) / 3 + 1;
        uint32_t blocks = (uint32_t)((count + 255) / 256);
        if (blocks > 1024) blocks = 1024;
        LAUNCH(lzf::lzf_seed_table_kernel, dim3(blocks), dim3(256), 0, st, d_table, d_dict, dict_len);
    }
    return LZF_OK;
}

int lzf_table_offset(void* d_table, uint32_t table_kind, uint64_t add, void* hip_stream) {
    if (!d_table || table_kind > LZF_TABLE_U16) { g_last_error = "lzf_table_offset: bad argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_table_offset_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(hip_stream), d_table, table_kind, add);
    return LZF_OK;
}

int lzf_table_offset_batch(void* const* d_tables, const uint64_t* d_adds, uint32_t n, uint32_t table_kind, void* hip_stream) {
    if (n == 0) return LZF_OK;
    if (!d_tables || !d_adds || table_kind > LZF_TABLE_U16) { g_last_error = "lzf_table_offset_batch: bad argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_table_offset_batch_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_tables, d_adds, n, table_kind);
    return LZF_OK;
}

int lzf_chain_decompress_step(const lzf_chain_step* d_steps, lzf_chain_state* d_state, uint32_t n_streams,
                              lzf_decompress_job* d_jobs, const lzf_job_result* d_results, void* hip_stream) {
    if (n_streams == 0) return LZF_OK;
    if (!d_steps || !d_state || !d_jobs || !d_results) { g_last_error = "lzf_chain_decompress_step: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_chain_decompress_step_kernel, dim3(n_streams), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_steps, d_state, n_streams, d_jobs, d_results);
    return LZF_OK;
}

int lzf_chain_decompress_step_trimmed(const lzf_chain_step* d_steps, lzf_chain_state* d_state, uint32_t n_streams,
                                      lzf_decompress_job* d_jobs, const lzf_job_result* d_results, void* hip_stream) {
    if (n_streams == 0) return LZF_OK;
    if (!d_steps || !d_state || !d_jobs || !d_results) { g_last_error = "lzf_chain_decompress_step_trimmed: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_chain_decompress_step_trimmed_kernel, dim3(n_streams), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_steps, d_state, n_streams, d_jobs, d_results);
    return LZF_OK;
}

// Jobs with long existing output, restated over its last 64 KiB for the decode and size calls, and their results put back
// (lzf_history_trim.h).  One launch each, one thread per job.
int lzf_history_trim_batch(const lzf_decompress_job* d_jobs, lzf_decompress_job* d_trimmed, uint64_t* d_shift, uint32_t n_jobs, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_jobs || !d_trimmed || !d_shift) { g_last_error = "lzf_history_trim_batch: NULL argument"; return LZF_E_INVALID; }
    if (d_trimmed == d_jobs) { g_last_error = "lzf_history_trim_batch: d_trimmed must not be d_jobs"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    const uint32_t blocks = (n_jobs - 1u) / 256u < 65535u ? (n_jobs - 1u) / 256u + 1u : 65536u;      // (the kernel strides over the rest)
    LAUNCH(lzf::lzf_history_trim_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_jobs, d_trimmed, d_shift, n_jobs);
    return LZF_OK;
}

int lzf_history_restore_batch(lzf_job_result* d_results, const uint64_t* d_shift, uint32_t n_jobs, void* hip_stream) {
    if (n_jobs == 0) return LZF_OK;
    if (!d_results || !d_shift) { g_last_error = "lzf_history_restore_batch: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    const uint32_t blocks = (n_jobs - 1u) / 256u < 65535u ? (n_jobs - 1u) / 256u + 1u : 65536u;      // (the kernel strides over the rest)
    LAUNCH(lzf::lzf_history_restore_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_results, d_shift, n_jobs);
    return LZF_OK;
}

int lzf_copy_ranges(const uint8_t* const* d_src, uint8_t* const* d_dst, const uint64_t* d_len, uint32_t n, uint64_t max_len, void* hip_stream) {
    if (n == 0 || max_len == 0) return LZF_OK;
    if (!d_src || !d_dst || !d_len) { g_last_error = "lzf_copy_ranges: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    const uint64_t pieces = (max_len + 65535ull) / 65536ull;
    if (pieces > 0x7FFFFFFFull) { g_last_error = "lzf_copy_ranges: max_len too large"; return LZF_E_INVALID; }
    for (uint32_t base = 0; base < n; base += 65535u) {              // grid.y is limited to 65535
        const uint32_t cnt = n - base < 65535u ? n - base : 65535u;
        LAUNCH(lzf::lzf_copy_ranges_kernel, dim3((uint32_t)pieces, cnt), dim3(256), 0, static_cast<hipStream_t>(hip_stream),
               d_src + base, d_dst + base, d_len + base, cnt);
    }
    return LZF_OK;
}

int lzf_xxh32_batch(const uint8_t* const* d_ptrs, const uint64_t* d_lens, uint32_t* d_out, uint32_t n, void* hip_stream) {
    if (n == 0) return LZF_OK;
    if (!d_ptrs || !d_lens || !d_out) { g_last_error = "lzf_xxh32_batch: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    // up to a few thousand buffers (block / content checksums of large blocks): one wave per buffer, streaming loads; beyond
    // that (many small blocks) 16 hashes per wave keep more chains per CU
    // (8192 is XXH32_WAVE_KERNEL_MAX_N of tests/aux_kernel_cases.py: tests/test_gpu_aux_kernels.py,
    //  test_xxh32_lane_kernel_on_both_sides_of_the_switch, calls with that many buffers and with one more.  Move both together.)
    if (n <= 8192u) LAUNCH(lzf::lzf_xxh32_wave_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(hip_stream), d_ptrs, d_lens, d_out, n);
    else LAUNCH(lzf::lzf_xxh32_kernel, dim3((n + 15) / 16), dim3(64), 0, static_cast<hipStream_t>(hip_stream), d_ptrs, d_lens, d_out, n);
    return LZF_OK;
}

// Resumable XXH32 on saved states: one wavefront per state for the update, one thread per state for the digest.
int lzf_xxh32_update_batch(lzf_xxh32_state* d_states, const uint8_t* const* d_ptrs, const uint64_t* d_lens, uint32_t n, void* hip_stream) {
    if (n == 0) return LZF_OK;
    if (!d_states || !d_ptrs || !d_lens) { g_last_error = "lzf_xxh32_update_batch: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_xxh32_update_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(hip_stream), d_states, d_ptrs, d_lens, n);
    return LZF_OK;
}

int lzf_xxh32_digest_batch(const lzf_xxh32_state* d_states, uint32_t* d_out, uint32_t n, void* hip_stream) {
    if (n == 0) return LZF_OK;
    if (!d_states || !d_out) { g_last_error = "lzf_xxh32_digest_batch: NULL argument"; return LZF_E_INVALID; }
    int rc = ensure_device();
    if (rc < 0) return rc;
    LAUNCH(lzf::lzf_xxh32_digest_kernel, dim3((n + 255u) / 256u), dim3(256), 0, static_cast<hipStream_t>(hip_stream), d_states, d_out, n);
    return LZF_OK;
}

}  // extern "C"
