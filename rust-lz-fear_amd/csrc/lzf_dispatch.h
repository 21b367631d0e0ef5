// lzf_dispatch.h — the DISPATCH RULES of the two batch calls as plain host C++: which kernels a call of n jobs launches on a device
// of a given geometry, in which classes, with which scratch.  No HIP and no environment here: the library compiles this header
// (capi.hip, capi_drivers.hip: the drivers execute a plan, they decide nothing) and so does a CPU test (tests/emu/emu_dispatch.cpp).
//
//   Geometry         compute units, LDS bytes per CU and wall-clock rate of a device — every threshold is a function of the first two
//   Knobs            every tuning value; the defaults ARE the product (the analysis library fills them from the environment, once)
//   decompress_plan  order wanted?  pipeline tried (window, ring, groups)?  fed path tried?  which pair / staged kernel last?
//   compress_plan    team / compact / general, fresh-only, probe order wanted?
//   size_plan        the size call: the latency class (a block summed up by many wavefronts) tried?  which form of the one-wave kernel last?
//   seg_layout / fed_layout / size_layout   the areas of the scratch allocations
#ifndef LZF_DISPATCH_H
#define LZF_DISPATCH_H

#include <stdint.h>
#include "lzfear_hip.h"
#include "lzf_fed_window.h"

namespace lzf_dispatch __attribute__((visibility("hidden"))) {      // (nothing of this is exported from a library that compiles it)

// MI355X: 256 compute units, 160 KiB of LDS each, wall_clock64() at 100 MHz
struct Geometry { uint32_t cu = 256u, lds = 160u * 1024u, wall_khz = 100000u; };
// workgroups of `lds_bytes` of LDS each that one CU holds
constexpr uint32_t per_cu(const Geometry& g, uint32_t lds_bytes) { return g.lds / lds_bytes ? g.lds / lds_bytes : 1u; }

// ---- LDS footprints the classes are derived from (each kernel's file asserts its own against these) -----------------------------
constexpr uint32_t lds_alloc(uint32_t bytes) { return (bytes + 1279u) / 1280u * 1280u; }     // what a workgroup's LDS takes: whole granules of 1 280 bytes (counted: 6 912 took 7 680)
constexpr uint32_t kPaired48Lds = 20u * 1024u;       // a pair of the 48-byte form (20 132 bytes): 8 per CU, 2 048 on MI355X
constexpr uint32_t kPaired24Lds = 12800u;            // a pair of the 24-byte form (12 452 bytes): 12 per CU, 3 072 on MI355X
constexpr uint32_t kStagedBeyond = 8u;               // more than this many residencies of 48-byte pairs: the one-wave staged16 kernel
constexpr uint32_t kFedLdsAlloc = 6400u;             // what the fed kernel's 5 952 bytes of LDS take
constexpr uint32_t kCompactLds = (4096u / 2u + 4096u / 32u + 64u) * 4u;      // lzf_compress_compact_kernel (= kernels.h kCompactLdsBytes)
constexpr uint32_t kTeamLds = 163840u;               // lzf_compress_team_kernel: a CU's whole LDS (lz4_compress_team.hip asserts it)
constexpr uint32_t kTeamRounds = 1u;                 // calls of up to this many jobs per CU take the team kernel
constexpr uint32_t kOrderFreshPerCu = 4u;            // fresh-only compress calls are probed and ordered from this many jobs per CU on

// ---- the segmented pipeline ------------------------------------------------------------------------------------------------------
constexpr uint32_t kSegChunk = (uint32_t)kFedwChunk, kSegStride = (uint32_t)kFedwStride, kSegChunkWords = kSegChunk / 32u, kSegTile = 2048u;
constexpr uint32_t kSegMaxIn = 4u * 1024u * 1024u + 32u * 1024u;     // a 4 MiB block at LZ4's worst case, rounded up
constexpr uint32_t kSegMinIn = 64u * 1024u;                          // smaller blocks are done sooner by one workgroup
// LDS of one workgroup of the resolve stage: its ring + flags, tickets and slack.  The pipeline takes batches of up to one block per
// 32 KiB ring the chip's LDS holds (MI355X: 4 per CU = 1 024 blocks) and gives a block the largest ring that still leaves every
// block of the batch resident at once.
constexpr uint32_t kSegRingSlack = 8u * 1024u;
constexpr uint32_t kSegRankMax = 1024u;              // one 1024-thread workgroup ranks the batch (lzf_seg_by_len_kernel / _order_ / _rank_)
constexpr uint64_t kSegRecsPerJob = 448u * 1024u;    // arena: records per job on average (16 bytes each)
constexpr uint32_t kSegMaxGroups = 4u;               // the caller's stream + three of the library's own
constexpr uint32_t kSegParsePerCu = 1024u, kSegTilePerCu = 2048u;    // workgroups per launch of the chunk / tile kernels, per CU
constexpr uint32_t kSegJobBytes = 48u, kSegRecBytes = 16u;           // sizeof(lzf::seg_job), sizeof(lzf::u32x4) (capi_drivers.hip asserts both)

// ---- the bitmap-fed path ---------------------------------------------------------------------------------------------------------
constexpr uint32_t kFedMinIn = 65536u;               // per job: smaller inputs are left to the pair kernel behind the fed kernel
constexpr uint64_t kFedMinHint = 262144u;            // per call: a caller that bounds its inputs at this keeps the call off the path
constexpr uint64_t kFedMaxScratch = 24ull << 30;     // bit maps of a call: 1 bit per compressed byte of the largest job x jobs
constexpr uint32_t kFedMaxJobs = 65535u;             // (the chunk stage's grid has one row per job)
constexpr uint32_t kFedPieces = 16u;                 // a call with more jobs than slots cuts every job into this many pieces
constexpr uint32_t kFedStateBytes = 16u, kFedTicketBytes = 4u * 32u * 32u;   // sizeof(lzf::fed_state); 32 counters, kFedTicketStride words apart

enum Mode : uint32_t { kByRule = 0u, kForced = 1u, kOff = 2u };
enum Order : uint32_t { kOrderNatural = 0u, kOrderByRule = 1u, kOrderAlways = 2u };
enum CompressKernel : uint32_t { kCompressByRule = 0u, kCompressGeneral = 1u, kCompressCompact = 3u };

struct Knobs {
    uint32_t fake_cu = 0u;                           // dispatch as if the device had this many compute units (0: as it has)
    int variant = -1;                                // a kernel variant by number, launched whatever the batch (-1: the rules below)
    uint32_t decompress_order = kOrderByRule, compress_order = kOrderByRule;
    uint32_t order_len_shift = 2u;                   // a decompress job's cost: its sequences + input length >> this
    // segmented pipeline
    uint32_t seg = kByRule;
    uint32_t seg_min_in = kSegMinIn;
    uint32_t seg_force = 0u;                         // its fall-backs, forced: 1 stager, 2 resolver, 3 no scratch, 8 swait
    uint32_t seg_ring = 0u;                          // 32768 / 65536 / 131072 whatever the batch (0: by residency)
    uint32_t seg_grid_parse = 0u, seg_grid_tile = 0u;        // workgroups per launch of the chunk / tile kernels (0: per CU, above)
    uint32_t seg_rec_pad = 0u;                       // unused LDS per workgroup of a grouped call's records stage
    uint32_t seg_group_n = 0u, seg_group_pct[kSegMaxGroups] = {};    // per cent of the jobs per group (0 groups: quarters from cu / 8 jobs on)
    // bitmap-fed path
    uint32_t fed = kByRule;
    uint32_t fed_min_in = kFedMinIn;
    bool fed_open = false;                           // the path is open to every call, whatever bound of its inputs the caller gives
    uint32_t fed_pieces = 0u, fed_slots = 0u;        // pieces per job, slots per CU (0: by rule / as counted)
    uint32_t fed_pad_lds = 0u;                       // unused LDS per wavefront
    uint32_t fed_carry = (uint32_t)kFedwCarry;
    bool fed_verbose = false;
    // the size call's latency class
    uint32_t size_seg = kByRule;
    uint32_t size_seg_min_in = kSegMinIn;
    uint32_t verify_seg = kByRule;                   // the verify call's latency class (its smallest input is size_seg_min_in)
    uint32_t size_force = 0u;                        // 1: its scratch refused, where the pool would refuse it (capi_drivers.hip); 2: no one-wave kernel behind it (tests: what the class finished itself)
    // compress
    uint32_t compress_kernel = kCompressByRule;
    long team_max = -1;                              // jobs per call the team kernel takes (-1: one per CU)
    uint32_t compact_pad_lds = 0u;
    uint32_t probe_piece = 65536u, probe_parts = 1u; // the cost probe: one 64 KiB piece from the middle of each payload
};

// ---- launch strings (lzf_last_decompress_launch / lzf_last_compress_launch) ---------------------------------------------------------
constexpr const char* kLaunchVariant = "analysis variant (LZF_DECOMPRESS_KERNEL)";
constexpr const char* kLaunchFed = "bitmap-fed: lzf_seg_parse_kernel + lzf_decompress_fed_kernel<4096,32,352> + lzf_decompress_paired_kernel<4096,24,384>";
enum Last : uint32_t { kPaired48 = 0u, kPaired24 = 1u, kStaged16 = 2u };
constexpr const char* launch_last(uint32_t last) {
    return last == kPaired48 ? "lzf_decompress_paired_kernel<4096,48,640>" : last == kPaired24 ? "lzf_decompress_paired_kernel<4096,24,384>"
                                                                                                 : "lzf_decompress_batched_kernel<4096,16,256,staged>";
}
constexpr const char* launch_seg(uint32_t ring) {
    return ring == 131072u ? "segmented: lzf_seg_resolve_pair_kernel<131072> + lzf_decompress_paired_kernel<4096,48,640>"
         : ring == 65536u ? "segmented: lzf_seg_resolve_pair_kernel<65536> + lzf_decompress_paired_kernel<4096,48,640>"
                          : "segmented: lzf_seg_resolve_pair_kernel<32768> + lzf_decompress_paired_kernel<4096,48,640>";
}

// lzf_last_size_launch: the latency class in front of the one-wave kernel / the one-wave kernel alone
constexpr const char* kLaunchSizeSeg = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_size_finish_kernel + lzf_decoded_size_kernel<48,768>";
constexpr const char* kLaunchSizeWave = "lzf_decoded_size_kernel<48,768>";
// lzf_last_verify_launch: the latency class in front of the one-wave kernel / the one-wave kernel alone
constexpr const char* kLaunchVerifySeg = "latency: lzf_seg_parse_kernel + lzf_size_tile_kernel + lzf_verify_finish_kernel + lzf_verify_tile_kernel + lzf_verify_kernel<48,768>";
constexpr const char* kLaunchVerifyWave = "lzf_verify_kernel<48,768>";

// ---- segmented pipeline: batch limit, ring, ranks, groups ----------------------------------------------------------------------------
constexpr uint32_t seg_blocks_per_cu(const Geometry& g, uint32_t ring) { return per_cu(g, ring + kSegRingSlack); }
constexpr uint32_t seg_max_jobs(const Geometry& g) { return seg_blocks_per_cu(g, 32768u) * g.cu < kSegRankMax ? seg_blocks_per_cu(g, 32768u) * g.cu : kSegRankMax; }
// the ring of a block: 128 KiB holds every distance LZ4 can express (no read-backs from HBM) while a CU has one block,
// 64 / 32 KiB with read-backs for the oldest few per cent of the sources beyond that
constexpr uint32_t seg_ring(const Geometry& g, const Knobs& k, uint32_t n) {
    return k.seg_ring == 32768u || k.seg_ring == 65536u || k.seg_ring == 131072u ? k.seg_ring
         : n <= seg_blocks_per_cu(g, 131072u) * g.cu && g.lds >= 131072u + kSegRingSlack ? 131072u
         : n <= seg_blocks_per_cu(g, 65536u) * g.cu && g.lds >= 65536u + kSegRingSlack ? 65536u : 32768u;
}
// which of the pipeline's stages follow an order of the jobs
struct SegRanks { bool order, by_len, rec_by_len; };
constexpr SegRanks seg_ranks(const Geometry& g, uint32_t n) {
    return SegRanks{n > g.cu && n <= seg_max_jobs(g),                      // resolve stage (one block per CU: nothing to balance)
                    n >= (g.cu + 7u) / 8u && n <= seg_max_jobs(g),         // chunk / tile stages, longest input first (MI355X: 32 jobs and more)
                    n >= (g.cu + 3u) / 4u};                                // the records stage follows it too (64 and more)
}
// A call of several hundred blocks takes its last two stages in groups, by sequences, most first (capi_drivers.hip: seg_enqueue_groups).
struct SegGroups { uint32_t n = 1u; uint32_t size[kSegMaxGroups] = {}; };
inline SegGroups seg_groups(const Geometry& g, const Knobs& kn, uint32_t n_jobs) {
    SegGroups r; r.size[0] = n_jobs;
    // (beyond what the rank kernels' one workgroup takes — only a forced pipeline gets here — one group, in the caller's order)
    if (n_jobs > seg_max_jobs(g)) return r;
    uint32_t pct[kSegMaxGroups] = {100u}; uint32_t k = 1u;
    if (n_jobs >= (g.cu + 7u) / 8u) { pct[0] = pct[1] = pct[2] = pct[3] = 25u; k = 4u; }      // (MI355X: 32 jobs and more; measured 49 .. 980 blocks: quarters beat halves and thirds)
    if (kn.seg_group_n) { for (uint32_t i = 0; i < kSegMaxGroups; ++i) pct[i] = kn.seg_group_pct[i]; k = kn.seg_group_n; }
    if (k <= 1u || n_jobs < 2u * k) return r;
    uint32_t left = n_jobs; r.n = 0u;
    for (uint32_t i = 0; i < k && left; ++i) {
        uint32_t sz = i + 1u == k ? left : (uint32_t)((uint64_t)n_jobs * pct[i] / 100u);
        if (sz > left) sz = left;
        if (!sz) continue;
        r.size[r.n++] = sz; left -= sz;
    }
    if (left && r.n) r.size[r.n - 1u] += left;
    return r;
}

// ---- scratch layouts -----------------------------------------------------------------------------------------------------------------
// chunks of the parse over `len` compressed bytes (the device's seg_nch, lz4_seg_front.hip, is asserted against this one)
constexpr uint32_t seg_nch(uint32_t len) { return len <= kSegChunk ? 1u : 1u + (len - kSegChunk + kSegStride - 1u) / kSegStride; }
// A caller that knows an upper bound of its jobs' input sizes gets scratch sized for it (the job array is in HBM, the host cannot look).
struct SegDims { uint32_t max_in, maxch, maxtile; };
constexpr SegDims seg_dims(uint64_t max_in_hint) {
    const uint32_t m = max_in_hint < kSegMaxIn ? (uint32_t)(max_in_hint < kSegChunk ? kSegChunk : max_in_hint) : kSegMaxIn;
    return SegDims{m, seg_nch(m), (m + kSegTile - 1u) / kSegTile};
}
struct Carver {          // areas of one allocation, 256-aligned, in the order they are taken
    uint64_t off = 0;
    uint64_t take(uint64_t bytes) { const uint64_t o = off; off = (off + bytes + 255u) / 256u * 256u; return o; }
};
struct SegLayout { SegDims d; uint64_t rec_cap, o_st, o_top, o_xexit, o_vfrom, o_tile_tok, o_tile_out, o_bits, o_recs, o_order, o_by_len, o_est, total; };
inline SegLayout seg_layout(uint32_t n, uint64_t max_in_hint) {
    SegLayout l{}; Carver c;
    l.d = seg_dims(max_in_hint);
    const uint64_t per_job = (uint64_t)l.d.max_in / 3u + 192u;
    l.rec_cap = (uint64_t)n * (per_job < kSegRecsPerJob ? per_job : kSegRecsPerJob);
    l.o_st = c.take((uint64_t)kSegJobBytes * n);
    l.o_top = c.take(8u);
    l.o_xexit = c.take(4ull * n * l.d.maxch);
    l.o_vfrom = c.take(4ull * n * l.d.maxch);
    l.o_tile_tok = c.take(4ull * n * l.d.maxtile);
    l.o_tile_out = c.take(4ull * n * l.d.maxtile);
    l.o_bits = c.take(4ull * n * l.d.maxch * kSegChunkWords);
    l.o_recs = c.take((uint64_t)kSegRecBytes * l.rec_cap);
    l.o_order = c.take(4ull * n);
    l.o_by_len = c.take(4ull * n);
    l.o_est = c.take(4ull * n);
    l.total = c.off;
    return l;
}
// (no xexit, no vfrom: there is no seam stage on the fed path)
struct FedLayout { SegDims d; uint64_t o_st, o_top, o_bits, o_ticket, o_state, total; };
inline FedLayout fed_layout(uint32_t n, uint64_t max_in_hint) {
    FedLayout l{}; Carver c;
    l.d = seg_dims(max_in_hint);
    l.o_st = c.take((uint64_t)kSegJobBytes * n);
    l.o_top = c.take(8u);
    l.o_bits = c.take(4ull * n * l.d.maxch * kSegChunkWords);
    l.o_ticket = c.take(kFedTicketBytes);
    l.o_state = c.take((uint64_t)kFedStateBytes * n);
    l.total = c.off;
    return l;
}

// The size call's latency class: the pipeline's front (state, exits, vfrom, bit maps) and 16 bytes per tile in place of
// tile_tok / tile_out; no arena, no arena top, no resolve order.
struct SizeLayout { SegDims d; uint64_t o_st, o_xexit, o_vfrom, o_tile_sum, o_bits, o_by_len, total; };
inline SizeLayout size_layout(uint32_t n, uint64_t max_in_hint) {
    SizeLayout l{}; Carver c;
    l.d = seg_dims(max_in_hint);
    l.o_st = c.take((uint64_t)kSegJobBytes * n);
    l.o_xexit = c.take(4ull * n * l.d.maxch);
    l.o_vfrom = c.take(4ull * n * l.d.maxch);
    l.o_tile_sum = c.take(16ull * n * l.d.maxtile);
    l.o_bits = c.take(4ull * n * l.d.maxch * kSegChunkWords);
    l.o_by_len = c.take(4ull * n);
    l.total = c.off;
    return l;
}

// ---- the size call -------------------------------------------------------------------------------------------------------------------
// lzf_decoded_size_kernel is one wavefront per job: a 4 MiB block takes it about 20 ms whatever the batch, and it fills the chip
// from 16 x 256 jobs on.  A call that leaves the chip mostly empty therefore goes through the LATENCY CLASS first: the pipeline's
// plan, parse and seam, then lzf_size_tile_kernel and lzf_size_finish_kernel, which finish every job that decodes cleanly; the
// one-wave kernel runs last over the whole call and skips those.  The class is every call of up to 16 jobs per CU (4 096 on MI355X: where
// the one-wave kernel begins to fill the chip, and the last count of the sweep at which every run of the class was shorter than every
// run of the one-wave kernel: profiles/size_latency_class.txt) with at least one input of size_seg_min_in bytes by the caller's bound.
constexpr uint32_t kSizeJobsPerCu = 16u;
constexpr uint32_t size_seg_max_jobs(const Geometry& g) { return kSizeJobsPerCu * g.cu; }
// The scratch is about 1.2 bits per compressed byte of the largest job x jobs (4 096 jobs at kSegMaxIn: 2.5 GiB).  3 GiB holds the
// whole class of an MI355X at the largest input — an eighth of what the bitmap-fed path may take (kFedMaxScratch); a larger device's or
// a forced class of more jobs gets it only with a caller's bound that keeps it below.
constexpr uint64_t kSizeMaxScratch = 3ull << 30;
constexpr uint32_t kSizeMaxJobs = 65535u;            // (the chunk / tile stages' grids have one row per job)
struct SizePlan {
    bool try_seg;            // the latency class in front (it may still decline: no scratch from the pool — never an error)
    uint32_t min_in;
    bool by_len;             // its chunk / tile stages take the jobs longest input first
    bool last;               // the one-wave kernel behind it (always, but for size_force == 2)
    const char* seg_launch; const char* last_launch;
};
inline SizePlan size_plan(const Geometry& g, const Knobs& k, uint32_t n_jobs, uint64_t max_input_len) {
    SizePlan p{};
    const bool in_class = k.size_seg == kForced || (k.size_seg == kByRule && n_jobs <= size_seg_max_jobs(g));
    p.min_in = k.size_seg_min_in;
    p.try_seg = in_class && n_jobs <= kSizeMaxJobs && max_input_len >= p.min_in &&
                size_layout(n_jobs, max_input_len).total <= kSizeMaxScratch;
    p.by_len = seg_ranks(g, n_jobs).by_len;
    p.last = k.size_force != 2u;
    p.seg_launch = kLaunchSizeSeg; p.last_launch = kLaunchSizeWave;
    return p;
}

// ---- the verify call -----------------------------------------------------------------------------------------------------------------
// The size call's arrangement: the latency class in front for a call of up to 16 jobs per CU with an input bound of at least 64 KiB,
// the one-wave kernel last over whatever the class left.  The class needs the size layout plus, for every tile, its base position
// (8 bytes) and, for every job, its smallest failing position (8 bytes); the same scratch cap.  The job count and the smallest
// input are size_plan's, measured for the size call and inherited here; profiles/verify.txt has the class against the one-wave
// kernel alone at 49 and 980 blocks of 4 MiB.
struct VerifyLayout { SizeLayout s; uint64_t o_tile_base, o_job_min, total; };
inline VerifyLayout verify_layout(uint32_t n, uint64_t max_in_hint) {
    VerifyLayout l{}; Carver c;
    l.s = size_layout(n, max_in_hint);
    c.off = l.s.total;
    l.o_tile_base = c.take(8ull * n * l.s.d.maxtile);
    l.o_job_min = c.take(8ull * n);
    l.total = c.off;
    return l;
}
struct VerifyPlan {
    bool try_seg;            // the latency class in front (it may still decline: no scratch from the pool — never an error)
    uint32_t min_in;
    bool by_len;             // its chunk / tile stages take the jobs longest input first
    const char* seg_launch; const char* last_launch;
};
inline VerifyPlan verify_plan(const Geometry& g, const Knobs& k, uint32_t n_jobs, uint64_t max_input_len) {
    VerifyPlan p{};
    const bool in_class = k.verify_seg == kForced || (k.verify_seg == kByRule && n_jobs <= size_seg_max_jobs(g));
    p.min_in = k.size_seg_min_in;
    p.try_seg = in_class && n_jobs <= kSizeMaxJobs && max_input_len >= p.min_in &&
                verify_layout(n_jobs, max_input_len).total <= kSizeMaxScratch;
    p.by_len = seg_ranks(g, n_jobs).by_len;
    p.seg_launch = kLaunchVerifySeg; p.last_launch = kLaunchVerifyWave;
    return p;
}

// ---- the decompress call -----------------------------------------------------------------------------------------------------------
// Tried in this order; a path that is tried may still decline (no scratch from the pool) and leave the call to the next one.
struct DecompressPlan {
    bool want_order;         // more blocks than the chip holds at once: longest first (perm + est scratch)
    bool seg_class;          // a batch of the pipeline's class: the sampled order, if wanted, runs in front of whatever takes the call
    bool try_seg;            // the segmented pipeline, then paired48 over what it left
    uint32_t seg_min_in, seg_ring;
    SegGroups groups;
    bool try_fed;            // plan + parse, the fed kernel, then paired24 over what it left
    uint32_t last;           // the last resort: Last
    const char* seg_launch; const char* fed_launch; const char* last_launch;
};
inline DecompressPlan decompress_plan(const Geometry& g, const Knobs& k, uint32_t n_jobs, uint64_t max_input_len) {
    DecompressPlan p{};
    // The producer/consumer pair kernel, with 48-byte regions while every block's workgroup is resident at once (lowest latency per
    // block: the copy stage is the critical path, the parse rides along) and 24-byte regions beyond that (smaller LDS footprint, more
    // blocks in flight); batches of more than eight times that many blocks (small blocks, typically) go to the one-wave staged16
    // kernel, which has no per-block pipeline to fill.
    const uint32_t resident48 = per_cu(g, kPaired48Lds) * g.cu;
    // the bitmap-fed path beyond what the 24-byte pair kernel holds at once (12 per CU, 3 072 on MI355X): up to there every block has
    // its pair of wavefronts for itself and the pair kernel is quicker (2 107 jobs 30.5 against 36.0 ms, 3 038 jobs 34.0 against 38.0;
    // 4 214 jobs 51.1 against 46.1, 8 085 jobs 81.6 against 73.5: profiles/r06_fed_kernel_study.txt)
    const uint32_t resident24 = per_cu(g, kPaired24Lds) * g.cu;
    p.want_order = k.decompress_order == kOrderAlways || (k.decompress_order == kOrderByRule && n_jobs > resident48);
    // Batches that leave the chip mostly empty with one workgroup per block: the segmented pipeline (a block decoded by many wavefronts)
    p.seg_class = k.seg == kForced || (k.seg == kByRule && n_jobs <= seg_max_jobs(g));
    p.seg_min_in = k.seg_min_in;
    p.try_seg = p.seg_class && max_input_len >= p.seg_min_in && k.seg_force != 3u;      // (no job can be in the pipeline's window / its scratch refused)
    p.seg_ring = seg_ring(g, k, n_jobs);
    p.groups = seg_groups(g, k, n_jobs);
    // The fed path per call: a caller that bounds its inputs keeps batches of small blocks off it altogether — per job the feed costs a
    // census of pieces, a chunk's parse and a ring re-fill: 16 384 jobs of ~32 KiB ran at 380 GiB/s through it and at 484 through the
    // pair kernel; 18 000 blocks of 256 KiB (inputs ~128 KiB) 12.97 against 12.43 ms; 4 536 blocks of 1 MiB 12.72 against 14.05.
    const bool fed_on = k.fed == kForced || (k.fed == kByRule && n_jobs > resident24);
    p.try_fed = fed_on && n_jobs <= kFedMaxJobs && max_input_len > k.fed_min_in && max_input_len > (k.fed_open ? 0u : kFedMinHint) &&
                fed_layout(n_jobs, max_input_len).total <= kFedMaxScratch;
    p.last = n_jobs <= resident48 ? kPaired48 : n_jobs <= kStagedBeyond * resident48 ? kPaired24 : kStaged16;
    p.seg_launch = launch_seg(p.seg_ring); p.fed_launch = kLaunchFed; p.last_launch = launch_last(p.last);
    return p;
}

// ---- the compress call -------------------------------------------------------------------------------------------------------------
// U32 jobs with a fresh or read-only template table go to the compact-table kernel (18 instead of 10 waves per CU), the others to the
// general kernel; which is which is in the job array, i.e. in HBM, so both are launched unless the caller vouches for the batch with
// LZF_KINDS_U32_FRESH_ONLY.  The latency class: a call with no more jobs than the chip has compute units gives every compact-table
// job a CU of its own (lzf_compress_team_kernel; needs a CU's whole LDS).
struct CompressPlan {
    uint32_t kinds;          // table_kinds with "either" resolved
    bool use_compact, use_team, fresh_only;
    bool want_order;         // probe the jobs' cost, then longest first
    uint32_t general_skip;   // what the general kernel leaves to the kernels in front of it: 0 nothing, 1 compact jobs, 2 the team's jobs
    const char* launch;
};
inline CompressPlan compress_plan(const Geometry& g, const Knobs& k, uint32_t n_jobs, uint32_t table_kinds) {
    CompressPlan p{};
    p.kinds = (table_kinds & (LZF_KINDS_U32 | LZF_KINDS_U16)) == 0 ? table_kinds | LZF_KINDS_U32 | LZF_KINDS_U16 : table_kinds;
    p.use_compact = k.compress_kernel != kCompressGeneral;
    uint32_t team_max = g.lds >= kTeamLds ? kTeamRounds * g.cu : 0u;
    if (k.team_max >= 0 && g.lds >= kTeamLds) team_max = (uint32_t)k.team_max;
    if (k.compress_kernel != kCompressByRule) team_max = 0u;
    p.use_team = p.use_compact && n_jobs <= team_max;
    p.fresh_only = p.use_compact && (p.kinds & LZF_KINDS_U32_FRESH_ONLY);
    // from four jobs per CU on for calls that vouch for fresh tables — not only beyond the 18 per CU the chip holds at once: the order
    // also spreads the expensive blocks over the compute units of a launch that is resident as a whole; a call of carried tables is
    // typically thousands of 64 KiB blocks of linked streams, too small to be probed
    p.want_order = k.compress_order && p.use_compact && (p.kinds & LZF_KINDS_U32) &&
                   (k.compress_order == kOrderAlways || n_jobs > per_cu(g, kCompactLds) * g.cu || (p.fresh_only && n_jobs > kOrderFreshPerCu * g.cu));
    p.general_skip = p.use_team ? 2u : p.use_compact ? 1u : 0u;
    p.launch = !(p.kinds & LZF_KINDS_U32) ? "lzf_compress_wave_kernel<U16>"
             : !p.use_compact ? "lzf_compress_wave_kernel (analysis: general)"
             : p.use_team ? (p.fresh_only ? "lzf_compress_team_kernel" : "lzf_compress_team_kernel + lzf_compress_team_carry_kernel + lzf_compress_wave_kernel")
                          : (p.fresh_only ? "lzf_compress_compact_kernel" : "lzf_compress_compact_kernel + lzf_compress_wave_kernel");
    return p;
}

}  // namespace lzf_dispatch
#endif  // LZF_DISPATCH_H
