// capi_drivers.hip — the host drivers of the two multi-launch decompress paths: the segmented pipeline (lz4_seg_*.hip) and
// the bitmap-fed kernel behind its plan + parse stages (lz4_decompress_fed.hip), and the front of the size call's latency class.  They execute a plan of lzf_dispatch.h; whether a
// call comes here at all, with which ring and in which groups, is decided there.
#include "capi_internal.h"
#include "kernels.h"
#include "capi_order.h"

namespace lzf_capi __attribute__((visibility("hidden"))) {
namespace {
namespace d = lzf_dispatch;

static_assert(sizeof(lzf::seg_job) == d::kSegJobBytes && sizeof(lzf::u32x4) == d::kSegRecBytes && sizeof(lzf::fed_state) == d::kFedStateBytes, "lzf_dispatch.h lays the scratch out with these sizes");
static_assert(d::kFedTicketBytes == sizeof(uint32_t) * 32u * lzf::kFedTicketStride, "32 ticket counters");
static_assert(d::kSegChunk == lzf::kSegChunk && d::kSegStride == lzf::kSegStride && d::kSegChunkWords == lzf::kSegChunkWords && d::kSegTile == lzf::kSegTile, "lzf_dispatch.h restates the chunk geometry");

using lzf::k_paired48; using lzf::k_paired24;
constexpr auto k_fed32 = lzf::lzf_decompress_fed_kernel<4096, 32, 352>;

template <class T> T* area(const AsyncScratch& s, uint64_t off) { return reinterpret_cast<T*>(s.at(off)); }

// what both paths' contexts share: the jobs, the sizes of the parse, the state array, the arena's top and the bit maps
lzf::seg_ctx seg_ctx_of(const d::Geometry& geo, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::SegDims& dim, uint32_t min_in,
                        const AsyncScratch& s, uint64_t o_st, uint64_t o_top, uint64_t o_bits) {
    lzf::seg_ctx c{};
    c.jobs = d_jobs; c.results = d_results; c.n_jobs = n;
    c.max_in = dim.max_in; c.min_in = min_in; c.maxch = dim.maxch; c.maxtile = dim.maxtile;
    c.st = area<lzf::seg_job>(s, o_st);
    c.rec_top = area<unsigned long long>(s, o_top);
    c.bits = area<uint32_t>(s, o_bits);
    c.n_cu = geo.cu;
    c.g_off = 0u; c.g_n = n;
    return c;
}

// ---- the segmented pipeline -------------------------------------------------------------------------------------------------
struct SegCall {
    AsyncScratch mem;
    lzf::seg_ctx ctx{};
    uint32_t* est = nullptr;       // [n] grouped calls: the jobs by sequences, most first (lzf_seg_rank_kernel)
    explicit SegCall(hipStream_t st) : mem(st) {}
};
// lays the scratch areas of a call out in one stream-ordered allocation; false (and nothing allocated) when the pool has no room
bool seg_alloc(SegCall& s, const d::Geometry& geo, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, uint32_t min_in, uint32_t ring, uint64_t max_in_hint) {
    const d::SegLayout l = d::seg_layout(n, max_in_hint);
    if (!s.mem.alloc(l.total)) return false;
    lzf::seg_ctx& c = s.ctx;
    c = seg_ctx_of(geo, d_jobs, d_results, n, l.d, min_in, s.mem, l.o_st, l.o_top, l.o_bits);
    c.rec_cap = l.rec_cap; c.ring_bytes = ring; c.dbg_force = knobs().seg_force;
    c.xexit = area<uint32_t>(s.mem, l.o_xexit);
    c.vfrom = area<uint32_t>(s.mem, l.o_vfrom);
    c.tile_tok = area<uint32_t>(s.mem, l.o_tile_tok);
    c.tile_out = area<uint32_t>(s.mem, l.o_tile_out);
    c.recs = area<lzf::u32x4>(s.mem, l.o_recs);
    const d::SegRanks r = d::seg_ranks(geo, n);
    c.order = r.order ? area<uint32_t>(s.mem, l.o_order) : nullptr;
    c.by_len = r.by_len ? area<uint32_t>(s.mem, l.o_by_len) : nullptr;
    c.rec_by_len = r.rec_by_len ? 1u : 0u;
    s.est = area<uint32_t>(s.mem, l.o_est);
    return true;
}
inline uint32_t seg_grid(uint32_t target, uint32_t n, uint32_t cap) {
    uint32_t g = target / n; if (g < 1u) g = 1u; if (g > cap) g = cap; return g;
}
// workgroups per launch of the chunk / tile kernels: about one chunk and a handful of tiles each — with 8 192 / 32 768 (each
// workgroup looping over a dozen chunks) the launches ended on their slowest loops: parse 4.3 -> 3.3 ms at 980 blocks, 1.02 -> 0.83 at 196
inline uint32_t seg_parse_target(const lzf::seg_ctx& c) { return knobs().seg_grid_parse ? knobs().seg_grid_parse : d::kSegParsePerCu * c.n_cu; }     // (MI355X: 262 144
inline uint32_t seg_tile_target(const lzf::seg_ctx& c) { return knobs().seg_grid_tile ? knobs().seg_grid_tile : d::kSegTilePerCu * c.n_cu; }         //  and 524 288)
// stages: 1 plan, 2 parse, 3 seam, 4 tilesum, 5 scan, 6 records (+ levels), 8 resolve (all when upto >= 8)
// seg_launch_prep: the stages that look at every job of the call; seg_launch_front: the chunk / tile stages of the group the context
// names (ranks g_off .. g_off + g_n) up to the scan; seg_launch_records, seg_launch_resolve: its last two stages.
int seg_launch_prep(const lzf::seg_ctx& c, hipStream_t st) {
    if (c.by_len && !c.grouped) LAUNCH(lzf::lzf_seg_by_len_kernel, dim3(1), dim3(1024), 0, st, c);
    LAUNCH(lzf::lzf_seg_plan_kernel, dim3((c.n_jobs + 255u) / 256u), dim3(256), 0, st, c);
    return LZF_OK;
}
int seg_launch_front(const lzf::seg_ctx& c, uint32_t upto, hipStream_t st) {
    const uint32_t n = c.g_n;
    if (upto >= 2) LAUNCH(lzf::lzf_seg_parse_kernel, dim3(seg_grid(seg_parse_target(c), n, c.maxch), n), dim3(64), 0, st, c);
    if (upto >= 3) LAUNCH(lzf::lzf_seg_seam_kernel, dim3(n), dim3(64), 0, st, c);
    if (upto >= 4) LAUNCH(lzf::lzf_seg_tilesum_kernel, dim3(seg_grid(seg_tile_target(c), n, c.maxtile), n), dim3(64), 0, st, c);
    if (upto >= 5) LAUNCH(lzf::lzf_seg_scan_kernel, dim3(n), dim3(64), 0, st, c);
    return LZF_OK;
}
// pad: bytes of unused LDS per workgroup (a grouped call's records stage under the resolve stages: the residency experiment)
int seg_launch_records(const lzf::seg_ctx& c, uint32_t pad, hipStream_t st) {
    if (c.order && !c.grouped) LAUNCH(lzf::lzf_seg_order_kernel, dim3(1), dim3(1024), 0, st, c);
    LAUNCH(lzf::lzf_seg_records_kernel, dim3(seg_grid(seg_tile_target(c), c.g_n, c.maxtile), c.g_n), dim3(64), pad, st, c);
    return LZF_OK;
}
int seg_launch_resolve(const lzf::seg_ctx& c, hipStream_t st) {
    const uint32_t n = c.g_n;
    if (c.ring_bytes == 131072u) LAUNCH(lzf::lzf_seg_resolve_pair_kernel<131072>, dim3(n), dim3(128), 0, st, c);
    else if (c.ring_bytes == 65536u) LAUNCH(lzf::lzf_seg_resolve_pair_kernel<65536>, dim3(n), dim3(128), 0, st, c);
    else LAUNCH(lzf::lzf_seg_resolve_pair_kernel<32768>, dim3(n), dim3(128), 0, st, c);
    return LZF_OK;
}
int seg_launch(const lzf::seg_ctx& c, uint32_t upto, hipStream_t st) {
    int rc = seg_launch_prep(c, st);
    if (rc == LZF_OK) rc = seg_launch_front(c, upto, st);
    if (rc == LZF_OK && upto >= 6) rc = seg_launch_records(c, 0u, st);
    if (rc == LZF_OK && upto >= 8) rc = seg_launch_resolve(c, st);
    return rc;
}

// ---- groups: the records stage of a group runs under the resolve stage of the groups before it -------------------------------
// The resolve stage is a chain per block (one pair of wavefronts, 7 ms for a 4 MiB text block whatever the batch) and leaves most
// of the chip idle; the stages before it are throughput kernels.  A call of several hundred blocks therefore takes its last two
// stages in groups, by sequences (known once the tiles are counted: lzf_seg_rank_kernel), most first: the caller's stream
// carries every group's records stage back to back, each group's resolve stage starts on a stream of its own as soon as its
// records are written (an event), and the caller's stream waits for all of them before the pair kernel looks for jobs the
// pipeline left.  The call then takes records(first group) + resolve(longest block) instead of records(all) + resolve(longest
// block), as long as the later groups — the blocks with fewer sequences — are through their shorter resolve stages by then.
// (The lanes are made at the highest stream priority: the runtime keeps a pool of hardware queues per priority, so they do not share
//  a queue with the application's streams; a fifth group measured slower: 8.9 -> 13.2 ms at 196 blocks.)
inline bool hip_ok(hipError_t e) { if (e != hipSuccess) { (void)hipGetLastError(); return false; } return true; }
inline void lane_drain(hipStream_t s) { (void)hip_ok(hipStreamSynchronize(s)); }
constexpr uint32_t kSegPauseUs = 10u;      // between a group's resolve stage and the next group's records stage (5 .. 80 us measured alike)
int seg_enqueue_groups(const SegCall& s, const d::SegGroups& g, SegLanes& L, uint32_t wall_khz, hipStream_t st) {
    lzf::seg_ctx c = s.ctx;
    std::lock_guard<std::mutex> lk(L.mu);
    int rc = seg_launch_prep(c, st);
    if (rc == LZF_OK) rc = seg_launch_front(c, 5u, st);         // plan .. scan over the whole call
    if (rc != LZF_OK) return rc;
    static_assert(d::kSegMaxGroups == 4, "lzf_seg_rank_kernel takes the group sizes as a uint4");
    LAUNCH(lzf::lzf_seg_rank_kernel, dim3(1), dim3(1024), 0, st, c, s.est, make_uint4(g.size[0], g.n > 1u ? g.size[1] : 0u, g.n > 2u ? g.size[2] : 0u, g.n > 3u ? g.size[3] : 0u));      // s.est: the jobs by sequences, most first; + every group's workgroup order
    c.by_len = s.est; c.grouped = 1u; c.res_prio = 1u;
    uint32_t off = 0, forked = 0;
    const uint32_t pause_ticks = kSegPauseUs * (wall_khz / 1000u);       // (the device's wall clock: 100 ticks per microsecond on MI355X)
    for (uint32_t k = 0; k < g.n && rc == LZF_OK; ++k) {
        c.g_off = off; c.g_n = g.size[k]; off += g.size[k];
        rc = seg_launch_records(c, knobs().seg_rec_pad, st);
        if (rc != LZF_OK) break;
        if (k + 1u == g.n) { rc = seg_launch_resolve(c, st); break; }      // the last group: on the caller's stream
        if (!hip_ok(hipEventRecord(L.front[k], st)) || !hip_ok(hipStreamWaitEvent(L.s[k], L.front[k], 0))) { rc = LZF_E_HIP; break; }
        rc = seg_launch_resolve(c, L.s[k]);
        ++forked;                                                // (whatever was enqueued on the lane is joined below)
        if (pause_ticks && rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_seg_pause_kernel, dim3(1), dim3(64), 0, st, pause_ticks);      // the resolve stage's workgroups first, then the next records stage
        if (!hip_ok(hipEventRecord(L.done[k], L.s[k]))) { --forked; if (rc == LZF_OK) rc = LZF_E_HIP; lane_drain(L.s[k]); }
    }
    for (uint32_t k = 0; k < forked; ++k)
        if (!hip_ok(hipStreamWaitEvent(st, L.done[k], 0))) { lane_drain(L.s[k]); if (rc == LZF_OK) rc = LZF_E_HIP; }
    return rc;
}
int seg_launch_grouped(const SegCall& s, const d::SegGroups& g, SegLanes& L, uint32_t wall_khz, hipStream_t st) {
    const int rc = seg_enqueue_groups(s, g, L, wall_khz, st);
    if (rc != LZF_OK)                                            // (a launch failed part-way: nothing may still be running on a lane when the caller frees the scratch)
        for (uint32_t k = 0; k < d::kSegMaxGroups - 1u; ++k) lane_drain(L.s[k]);
    return rc;
}

}  // namespace

// The whole call: pipeline, then the pair kernel over what the pipeline did not finish.
int seg_decompress(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::DecompressPlan& plan, hipStream_t st, bool* used, uint64_t max_in_hint) {
    SegCall s(st);
    *used = seg_alloc(s, dv.geo, d_jobs, d_results, n, plan.seg_min_in, plan.seg_ring, max_in_hint);
    if (!*used) return LZF_OK;                                   // (no scratch: the caller launches the pair kernel over everything)
    SegLanes* lanes = plan.groups.n > 1u ? seg_lanes(dv) : nullptr;
    int rc = lanes ? seg_launch_grouped(s, plan.groups, *lanes, dv.geo.wall_khz, st) : seg_launch(s.ctx, 8u, st);
    if (rc == LZF_OK) LAUNCH_RC(rc, k_paired48, dim3(n), dim3(128), 0, st, d_jobs, d_results, n, (const uint32_t*)nullptr, (const lzf::seg_job*)s.ctx.st);
    if (s.mem.release() != hipSuccess && rc == LZF_OK) rc = LZF_E_HIP;
    if (rc != LZF_OK) g_last_error = "segmented decompress: launch failed";
    return rc;
}

// ---- the size call's latency class (lz4_decoded_size_seg.hip) -------------------------------------------------------------------
// plan, parse and seam of the pipeline over the whole call — `out` is not needed, prefix and existing output are lengths — then the
// tiles summed up and every job's tiles added up and checked.  Enqueue only; the scratch stays with the caller until the one-wave
// kernel behind this has looked at the state array.
int size_seg_front(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::SizePlan& plan, AsyncScratch& mem, hipStream_t st,
                   const lzf::seg_job** done, uint64_t max_in_hint) {
    *done = nullptr;
    const d::SizeLayout l = d::size_layout(n, max_in_hint);
    if (knobs().size_force == 1u || !mem.alloc(l.total)) return LZF_OK;      // (no scratch — or the analysis library's forced refusal: the one-wave kernel takes the call as it always did)
    lzf::seg_ctx c{};
    c.jobs = d_jobs; c.results = d_results; c.n_jobs = n;
    c.max_in = l.d.max_in; c.min_in = plan.min_in; c.maxch = l.d.maxch; c.maxtile = l.d.maxtile;
    c.st = area<lzf::seg_job>(mem, l.o_st);
    c.xexit = area<uint32_t>(mem, l.o_xexit);
    c.vfrom = area<uint32_t>(mem, l.o_vfrom);
    c.tile_sum = area<lzf::u32x4>(mem, l.o_tile_sum);
    c.bits = area<uint32_t>(mem, l.o_bits);
    c.by_len = plan.by_len ? area<uint32_t>(mem, l.o_by_len) : nullptr;
    c.n_cu = dv.geo.cu; c.g_off = 0u; c.g_n = n; c.size_only = 1u;
    int rc = seg_launch_prep(c, st);
    if (rc == LZF_OK) rc = seg_launch_front(c, 3u, st);           // parse, seam
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_size_tile_kernel, dim3(seg_grid(seg_tile_target(c), n, c.maxtile), n), dim3(64), 0, st, c);
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_size_finish_kernel, dim3(n), dim3(64), 0, st, c);
    if (rc != LZF_OK) g_last_error = "decoded sizes, latency class: launch failed";
    *done = c.st;
    return rc;
}

// ---- the verify call's latency class (lz4_verify.hip) -----------------------------------------------------------------------------
// The size call's front and tile sums as they are, then the finish kernel that keeps every tile's base, the compares tile by tile
// and the verdicts of the jobs of clean tiles.  Enqueue only; the scratch stays with the caller until the one-wave kernel behind
// this has looked at the state array.
int verify_seg_front(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::VerifyPlan& plan, AsyncScratch& mem, hipStream_t st,
                     const lzf::seg_job** done, uint64_t max_in_hint) {
    *done = nullptr;
    const d::VerifyLayout l = d::verify_layout(n, max_in_hint);
    if (!mem.alloc(l.total)) return LZF_OK;                      // (no scratch: the one-wave kernel takes the whole call)
    lzf::seg_ctx c{};
    c.jobs = d_jobs; c.results = d_results; c.n_jobs = n;
    c.max_in = l.s.d.max_in; c.min_in = plan.min_in; c.maxch = l.s.d.maxch; c.maxtile = l.s.d.maxtile;
    c.st = area<lzf::seg_job>(mem, l.s.o_st);
    c.xexit = area<uint32_t>(mem, l.s.o_xexit);
    c.vfrom = area<uint32_t>(mem, l.s.o_vfrom);
    c.tile_sum = area<lzf::u32x4>(mem, l.s.o_tile_sum);
    c.bits = area<uint32_t>(mem, l.s.o_bits);
    c.by_len = plan.by_len ? area<uint32_t>(mem, l.s.o_by_len) : nullptr;
    c.n_cu = dv.geo.cu; c.g_off = 0u; c.g_n = n; c.size_only = 1u;
    uint64_t* const tile_base = area<uint64_t>(mem, l.o_tile_base);
    unsigned long long* const job_min = area<unsigned long long>(mem, l.o_job_min);
    if (hipMemsetAsync(job_min, 0xFF, 8u * (size_t)n, st) != hipSuccess) { g_last_error = "verify, latency class: memset failed"; return LZF_E_HIP; }
    int rc = seg_launch_prep(c, st);
    if (rc == LZF_OK) rc = seg_launch_front(c, 3u, st);           // parse, seam
    const dim3 tiles(seg_grid(seg_tile_target(c), n, c.maxtile), n);
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_size_tile_kernel, tiles, dim3(64), 0, st, c);
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_verify_finish_kernel, dim3(n), dim3(64), 0, st, c, tile_base);
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_verify_tile_kernel, tiles, dim3(64), 0, st, c, (const uint64_t*)tile_base, job_min);
    if (rc == LZF_OK) LAUNCH_RC(rc, lzf::lzf_verify_end_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, c, (const unsigned long long*)job_min);
    if (rc != LZF_OK) g_last_error = "verify, latency class: launch failed";
    *done = c.st;
    return rc;
}

// ---- the bitmap-fed kernel (lz4_decompress_fed.hip): batches beyond the segmented pipeline's ----------------------------------
// plan + parse of the segmented pipeline over the whole batch (the token bit map of every block: one bit per compressed byte;
// no seam stage — the fed wavefront carries the true chain and masks or walks what a chunk's parse marked before it fell in step),
// then one wavefront per block that lists its tokens from the map and copies — the in-kernel parse of the pair kernel is
// 13.0 of its 27.8 wave-instructions per sequence, the hop parse 3.8 — then the pair kernel over whatever that left (errors,
// sizes outside the map's window).  The launch order comes from the parse as well: it counts every job's tokens.
namespace {
// Workgroups of the kernel the current device holds at once, COUNTED (lz4_decompress_fed.hip, census mode): the occupancy query
// does not know the LDS allocation granule (an earlier build's 6 912 bytes took 7 680: 21 per CU where the query said 23; today's
// 5 952 take 6 400: 25 per CU counted with the registers bounded to seven waves per SIMD), and a schedule with more slots than
// residents runs its surplus slots after the others.  As built the REGISTERS limit the kernel: LZF_FED_WAVES (kernels.h) waves on
// each of a CU's four SIMDs, 24 per CU counted.  Once per device and process: one launch of ~0.1 ms and a 4-byte copy (the one
// place a batch call waits for the device).
constexpr uint32_t kFedWavesPerCu = 4u * (LZF_FED_WAVES > 0 ? (uint32_t)LZF_FED_WAVES : 5u);   // (no bound: 82 VGPRs, five per SIMD)
struct FedCensus { uint32_t slots, xcc_mask; };
FedCensus fed_census(Device& dev, hipStream_t st) {
    const uint32_t cu = dev.geo.cu;
    {
        std::lock_guard<std::mutex> lk(device_mutex());
        if (dev.fed_slots) return FedCensus{dev.fed_slots, dev.fed_xcc_mask};
    }
    // (counted with the mutex free: it waits for the device; two first calls at once both count, and get the same answer)
    FedCensus answer{0u, 0u};
    uint32_t* dmem = nullptr;
    if (hipMalloc(&dmem, 4u * sizeof(uint32_t)) == hipSuccess) {
        const uint32_t init[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
        lzf::fed_args a{}; a.census = dmem;
        if (hipMemcpyAsync(dmem, init, sizeof init, hipMemcpyHostToDevice, st) == hipSuccess) {
            hipLaunchKernelGGL(k_fed32, dim3(40u * cu), dim3(64), 0, st, a);
            uint32_t got[4] = {0, 0, 0, 0};
            if (hipGetLastError() == hipSuccess && hipMemcpyAsync(got, dmem, sizeof got, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess &&
                got[1] != 0xFFFFFFFFu && got[1] >= cu) { answer.slots = got[1]; answer.xcc_mask = got[2]; }
        }
        (void)hipFree(dmem);
    }
    (void)hipGetLastError();
    if (!answer.slots) {             // (the census failed: the smaller of the LDS's and the registers' answer; no XCD mask: jobs stay whole)
        const uint32_t by_lds = d::per_cu(dev.geo, d::kFedLdsAlloc);
        answer.slots = (by_lds < kFedWavesPerCu ? by_lds : kFedWavesPerCu) * cu;
    }
    if (knobs().fed_verbose) fprintf(stderr, "[lzf] bitmap-fed kernel: %u workgroups resident at once (%u compute units), XCD mask 0x%x\n", answer.slots, cu, answer.xcc_mask);
    std::lock_guard<std::mutex> lk(device_mutex());
    if (!dev.spare) { dev.fed_slots = answer.slots; dev.fed_xcc_mask = answer.xcc_mask; }
    return answer;
}
}  // namespace

// The front of a fed call, in the scratch `mem` holds: plan + parse over the whole batch and, when an order is asked for (est not
// null), the launch order from the estimates the two stages leave in est[].  *ctx = the context the stages ran with.
int fed_front(const d::Geometry& geo, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::FedLayout& l, const AsyncScratch& mem,
              uint32_t min_in, uint32_t len_shift, uint32_t* perm, uint32_t* est, hipStream_t st, lzf::seg_ctx* ctx) {
    lzf::seg_ctx& c = *ctx;
    c = seg_ctx_of(geo, d_jobs, d_results, n, l.d, min_in, mem, l.o_st, l.o_top, l.o_bits);
    c.fed = 1u; c.est = perm ? est : nullptr; c.len_shift = len_shift;
    int rc = seg_launch(c, 2u, st);                              // plan, parse
    if (rc == LZF_OK && c.est) rc = launch_order_by_estimate(est, perm, n, st);
    return rc;
}

// scratch, plan + parse, the launch order, reset, the fed kernel, the pair kernel, scratch back.
// perm + est (both or neither): the launch order is wanted and nobody has worked it out yet — est[] is filled here, by the plan stage
// (the bytes' share) and the parse (the sequences: counted, where lzf_decompress_cost_kernel samples — the block's exact number when every
// chunk's chain falls in step with the block's inside its overlap, marks off the chain included otherwise: tests/launch_order_cases.py), and
// perm[] ordered by it.
namespace {
// what a fed call launched with: the state array of the front, the kernel's arguments and its geometry (lzf_debug_fed reads them back)
struct FedLaunch { lzf::seg_ctx c{}; lzf::fed_args a{}; uint32_t slots = 0, grid = 0, census_mask = 0; };
// plan + parse, the launch order, reset, the fed kernel — everything of a fed call in front of the pair kernel, in the scratch `mem` holds.
// stop_piece: lzf::fed_args::stop_piece (the analysis library's lzf_debug_fed; 0 in every product call).
int fed_launch(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, const d::FedLayout& l, const AsyncScratch& mem,
               uint32_t* perm, uint32_t* est, uint32_t stop_piece, hipStream_t st, FedLaunch* fl) {
    const d::Knobs& kn = knobs();
    lzf::seg_ctx& c = fl->c;
    int rc = fed_front(dv.geo, d_jobs, d_results, n, l, mem, kn.fed_min_in, kn.order_len_shift, perm, est, st, &c);
    if (rc != LZF_OK) return rc;
    // The kernel runs as one wavefront per SLOT — as many as the device holds at once — and the slots share the jobs out in pieces
    // (lz4_decompress_fed.hip): a call with more jobs than slots cuts every job into 16 (measured at 2.2 jobs per slot: 107.4 ms whole,
    // 97.3 / 97.2 / 97.8 / 99.0 / 101.7 ms with 8 / 16 / 32 / 64 / 128 pieces), a smaller one leaves them whole.
    const FedCensus fc = fed_census(dv, st);
    const uint32_t slots = kn.fed_slots ? kn.fed_slots * c.n_cu : fc.slots;
    uint32_t pieces = kn.fed_pieces ? kn.fed_pieces : n > fc.slots ? d::kFedPieces : 1u;
    if ((uint64_t)n * pieces > 0xFFFFFFF0ull || !fc.xcc_mask) pieces = 1u;       // (no XCD mask: jobs stay whole)
    fl->a = lzf::fed_args{d_jobs, d_results, c.st, c.bits, perm, area<lzf::fed_state>(mem, l.o_state), area<uint32_t>(mem, l.o_ticket), fc.xcc_mask ? fc.xcc_mask : 1u, n, c.maxch, pieces, kn.fed_carry, nullptr, stop_piece};
    fl->slots = slots; fl->grid = slots < n ? slots : n; fl->census_mask = fc.xcc_mask;
    LAUNCH_RC(rc, lzf::lzf_fed_reset_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, fl->a);
    if (rc == LZF_OK) LAUNCH_RC(rc, k_fed32, dim3(fl->grid), dim3(64), kn.fed_pad_lds, st, fl->a);
    return rc;
}
}  // namespace

int fed_decompress(Device& dv, const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, uint32_t* perm, uint32_t* est, hipStream_t st, bool* used, uint64_t max_in_hint) {
    const d::FedLayout l = d::fed_layout(n, max_in_hint);
    AsyncScratch mem(st);
    *used = mem.alloc(l.total);
    if (!*used) return LZF_OK;                                   // (no room for the bit maps: the pair kernel takes the call, the order is still to make)
    FedLaunch fl;
    int rc = fed_launch(dv, d_jobs, d_results, n, l, mem, perm, est, 0u, st, &fl);
    if (rc == LZF_OK) LAUNCH_RC(rc, k_paired24, dim3(n), dim3(128), 0, st, d_jobs, d_results, n, (const uint32_t*)perm, (const lzf::seg_job*)fl.c.st);
    if (mem.release() != hipSuccess && rc == LZF_OK) rc = LZF_E_HIP;
    if (rc != LZF_OK) g_last_error = "bitmap-fed decompress: launch failed";
    return rc;
}

}  // namespace lzf_capi

using namespace lzf_capi;
#ifdef LZF_ANALYSIS
extern "C"
// Analysis only: run the segmented pipeline up to a stage and copy its scratch areas to host buffers (NULL = skip).
// geom[0..3] = maxch, maxtile, chunk words, records in the arena.
int lzf_debug_seg(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, uint32_t min_in, uint32_t upto,
                  void* h_state, void* h_bits, void* h_xexit, void* h_vfrom, void* h_tile_tok, void* h_tile_out, void* h_recs, uint64_t recs_bytes,
                  uint32_t* geom) {
    int rc = ensure_device();
    if (rc < 0) return rc;
    SegCall s(nullptr);
    const d::Geometry& geo = device().geo;
    if (knobs().seg_force == 3u || !seg_alloc(s, geo, d_jobs, d_results, n, min_in, d::seg_ring(geo, knobs(), n), ~0ull)) return LZF_E_HIP;
    const lzf::seg_ctx& c = s.ctx;
    rc = seg_launch(c, upto, nullptr);
    HIP_TRY(hipDeviceSynchronize());
    if (geom) { geom[0] = c.maxch; geom[1] = c.maxtile; geom[2] = lzf::kSegChunkWords; geom[3] = (uint32_t)c.rec_cap; }
    if (h_state) HIP_TRY(hipMemcpy(h_state, c.st, sizeof(lzf::seg_job) * n, hipMemcpyDeviceToHost));
    if (h_bits) HIP_TRY(hipMemcpy(h_bits, c.bits, sizeof(uint32_t) * (size_t)n * c.maxch * lzf::kSegChunkWords, hipMemcpyDeviceToHost));
    if (h_xexit) HIP_TRY(hipMemcpy(h_xexit, c.xexit, sizeof(uint32_t) * (size_t)n * c.maxch, hipMemcpyDeviceToHost));
    if (h_vfrom) HIP_TRY(hipMemcpy(h_vfrom, c.vfrom, sizeof(uint32_t) * (size_t)n * c.maxch, hipMemcpyDeviceToHost));
    if (h_tile_tok) HIP_TRY(hipMemcpy(h_tile_tok, c.tile_tok, sizeof(uint32_t) * (size_t)n * c.maxtile, hipMemcpyDeviceToHost));
    if (h_tile_out) HIP_TRY(hipMemcpy(h_tile_out, c.tile_out, sizeof(uint32_t) * (size_t)n * c.maxtile, hipMemcpyDeviceToHost));
    if (h_recs) { uint64_t nb = sizeof(lzf::u32x4) * c.rec_cap; if (nb > recs_bytes) nb = recs_bytes; HIP_TRY(hipMemcpy(h_recs, c.recs, nb, hipMemcpyDeviceToHost)); }
    HIP_TRY(s.mem.release());
    return rc;
}

// Analysis only: one piece of the launch-order stage on its own, on the default stream, through the launch lines the batch calls use
// (capi_order.h, fed_front above); the results are copied to host buffers.  d_jobs is a device array of n jobs, h_* are host buffers.
//   what 0  lzf_order_by_estimate_kernel over h_in = est[n]                                         -> h_perm[n]
//        1  lzf_order_by_input_len_kernel over d_jobs (decompress jobs; only input_len is read)      -> h_perm[n]
//        2  lzf_order_by_cost_kernel over d_jobs (compress jobs), h_in = lzf_job_result[n * b],
//           a = piece, b = parts                                                                     -> h_perm[n]
//        3  lzf_decompress_cost_kernel over d_jobs, a = len_shift                                    -> h_est[n]
//        4  the front of fed_decompress over d_jobs: scratch, plan + parse with fed = 1 and est set,
//           a = min_in, b = len_shift, then the order; no fed kernel, no pair kernel                 -> h_est[n], h_perm[n]
//        5  lzf_cost_probe_jobs_kernel over d_jobs (compress jobs) and the dry run of the probes,
//           a = piece, b = parts                     -> h_probes = lzf_compress_job[n * b], h_probe_results = lzf_job_result[n * b]
extern "C"
int lzf_debug_order(uint32_t what, const void* d_jobs, uint32_t n, const void* h_in, uint32_t a, uint32_t b,
                    uint32_t* h_est, uint32_t* h_perm, void* h_probes, void* h_probe_results) {
    int rc = ensure_device();
    if (rc < 0) return rc;
    if (n == 0 || what > 5u || (what >= 1u && !d_jobs) || ((what == 0u || what == 2u) && !h_in) || ((what == 2u || what == 5u) && (!a || !b))) return LZF_E_INVALID;
    const size_t n_probes = (size_t)n * (what == 2u || what == 5u ? b : 0u);
    // [est or the caller's est][perm][probe jobs][probe results][results of the fed front]
    d::Carver cv;
    const uint64_t o_est = cv.take(4ull * n), o_perm = cv.take(4ull * n), o_probes = cv.take(sizeof(lzf_compress_job) * n_probes),
                   o_pres = cv.take(sizeof(lzf_job_result) * n_probes), o_res = cv.take(sizeof(lzf_job_result) * (what == 4u ? n : 0u));
    AsyncScratch buf(nullptr), fed_mem(nullptr);
    if (!buf.alloc(cv.off + 256u)) return LZF_E_HIP;
    uint32_t* const est = area<uint32_t>(buf, o_est);
    uint32_t* const perm = area<uint32_t>(buf, o_perm);
    lzf_compress_job* const probes = area<lzf_compress_job>(buf, o_probes);
    lzf_job_result* const pres = area<lzf_job_result>(buf, o_pres);
    const lzf_decompress_job* const dj = static_cast<const lzf_decompress_job*>(d_jobs);
    const lzf_compress_job* const cj = static_cast<const lzf_compress_job*>(d_jobs);
    hipStream_t st = nullptr;
    rc = LZF_OK;
    if (what == 0u) {
        HIP_TRY(hipMemcpy(est, h_in, 4ull * n, hipMemcpyHostToDevice));
        rc = launch_order_by_estimate(est, perm, n, st);
    } else if (what == 1u) {
        rc = launch_order_by_input_len(dj, perm, n, st);
    } else if (what == 2u) {
        HIP_TRY(hipMemcpy(pres, h_in, sizeof(lzf_job_result) * n_probes, hipMemcpyHostToDevice));
        rc = launch_order_by_cost(cj, pres, perm, n, a, b, st);
    } else if (what == 3u) {
        rc = launch_decompress_cost(dj, n, est, a, st);
    } else if (what == 4u) {
        const d::FedLayout l = d::fed_layout(n, ~0ull);
        if (!fed_mem.alloc(l.total)) return LZF_E_HIP;
        lzf::seg_ctx c{};
        rc = fed_front(device().geo, dj, area<lzf_job_result>(buf, o_res), n, l, fed_mem, a, b, perm, est, st, &c);
    } else {
        rc = launch_cost_probes(cj, probes, pres, n, a, b, st);
    }
    HIP_TRY(hipDeviceSynchronize());
    if (rc != LZF_OK) return rc;
    if (h_est && (what == 3u || what == 4u)) HIP_TRY(hipMemcpy(h_est, est, 4ull * n, hipMemcpyDeviceToHost));
    if (h_perm && what != 3u && what != 5u) HIP_TRY(hipMemcpy(h_perm, perm, 4ull * n, hipMemcpyDeviceToHost));
    if (h_probes && what == 5u) HIP_TRY(hipMemcpy(h_probes, probes, sizeof(lzf_compress_job) * n_probes, hipMemcpyDeviceToHost));
    if (h_probe_results && what == 5u) HIP_TRY(hipMemcpy(h_probe_results, pres, sizeof(lzf_job_result) * n_probes, hipMemcpyDeviceToHost));
    HIP_TRY(fed_mem.release());
    HIP_TRY(buf.release());
    return LZF_OK;
}

// Analysis only: a fed call WITHOUT the pair kernel behind it, on the default stream: scratch, fed_front, lzf_fed_reset_kernel and the fed kernel through
// fed_launch — the launch lines of fed_decompress, the census and LZF_FED_PIECES / LZF_FED_SLOTS / LZF_FED_CARRY / LZF_FED_MIN_IN included; the launch
// order is made as the batch call makes it (LZF_DECOMPRESS_ORDER).  stop_piece as fed_args::stop_piece (0: every ticket is drawn).  Copied to host
// buffers (NULL = skip): h_state = seg_job[n], h_fed = fed_state[n], h_perm = perm[n] (all ~0 when no order was made),
// geom[0..3] = pieces used, slots, grid, the census's XCD mask (0: it gave none).  What the kernel did not finish is left as the caller put it: d_results too.
extern "C"
int lzf_debug_fed(const lzf_decompress_job* d_jobs, lzf_job_result* d_results, uint32_t n, uint64_t max_input_len, uint32_t stop_piece,
                  void* h_state, void* h_fed, uint32_t* h_perm, uint32_t* geom) {
    int rc = ensure_device();
    if (rc < 0) return rc;
    if (n == 0 || !d_jobs || !d_results) return LZF_E_INVALID;
    Device& dv = device();
    hipStream_t st = nullptr;
    const d::FedLayout l = d::fed_layout(n, max_input_len ? max_input_len : ~0ull);      // (the caller's bound of its inputs, as lzf_decompress_batch_sized takes it; 0: none)
    AsyncScratch mem(st), perm_mem(st);
    if (!mem.alloc(l.total)) return LZF_E_HIP;
    const bool want_order = d::decompress_plan(dv.geo, knobs(), n, ~0ull).want_order;
    uint32_t* const perm = want_order && perm_mem.alloc(2u * sizeof(uint32_t) * (size_t)n) ? static_cast<uint32_t*>(perm_mem.p) : nullptr;
    FedLaunch fl;
    rc = fed_launch(dv, d_jobs, d_results, n, l, mem, perm, perm ? perm + n : nullptr, stop_piece, st, &fl);
    HIP_TRY(hipDeviceSynchronize());
    if (rc != LZF_OK) return rc;
    if (geom) { geom[0] = fl.a.pieces; geom[1] = fl.slots; geom[2] = fl.grid; geom[3] = fl.census_mask; }
    if (h_state) HIP_TRY(hipMemcpy(h_state, fl.c.st, sizeof(lzf::seg_job) * n, hipMemcpyDeviceToHost));
    if (h_fed) HIP_TRY(hipMemcpy(h_fed, fl.a.state, sizeof(lzf::fed_state) * n, hipMemcpyDeviceToHost));
    if (h_perm) { if (perm) HIP_TRY(hipMemcpy(h_perm, perm, sizeof(uint32_t) * n, hipMemcpyDeviceToHost)); else memset(h_perm, 0xFF, sizeof(uint32_t) * n); }
    HIP_TRY(perm_mem.release());
    HIP_TRY(mem.release());
    return LZF_OK;
}
#endif
