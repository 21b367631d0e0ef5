// frame_device.hip — the frame layer for frames that live in device memory (include/lzfear_frame.h, "frames in device memory").
//
// lzf_frame_decompress_many's work without the host round trip of the bytes: the host sees only what it needs to plan.
//   1. scan, pass 1 (lzf_frame_scan_kernel, one lane per frame): header (decompress.rs:102-161) and block walk (:198-235) of
//      lzf_frame_scan.h; a 64-byte summary per frame comes back (wait 1).
//   2. scan, pass 2 (lzf_frame_table_kernel): the block table, 24 bytes per block, comes back (wait 2).
//   3. the host builds the decode jobs from the table (frame_jobs.h, the same layout as the host driver), uploads them and
//      enqueues, pass after pass of the memory budget: block checksums (lzf_xxh32_batch), decode (lzf_decompress_batch_sized /
//      lzf_chain_decompress_step), delivery (lzf_frame_deliver_kernel: the reader's stop rules in stream order, :198-288),
//      the copy into the caller's outputs (lzf_copy_ranges), content checksums (lzf_xxh32_batch + lzf_frame_content_check_kernel).
// Results (status, out_len, consumed) are written to device arrays in stream order; scratch comes from the stream-ordered pool.
//
// lzf_frame_compress_device_many is lzf_frame_compress_many's work on inputs in device memory.  The host plans the whole call
// from in_len[] and the settings (frame_jobs.h's input windows, the same as the host driver's) and reads nothing back; per
// pass of the memory budget it enqueues: the dict ++ block copies (lzf_copy_ranges), the tables (lzf_table_seed_from_dictionary
// once, copied into every linked stream's table), the compression (lzf_compress_batch; linked streams in lock-step with
// lzf_table_offset_batch between the steps), assembly (lzf_frame_assemble_kernel: header, length words, EndMark, status and
// out_len, and the lists of the steps behind it, by lzf_frame_layout.h's rule), the payload copy (lzf_copy_ranges), block and
// content checksums (lzf_xxh32_batch) and the checksum words (lzf_frame_patch_kernel).
//
// lzf_frame_compressed_size_device / lzf_frame_compress_stream_size_device: the compress plan with `sizes_only` — no output slots,
// jobs without `out` through lzf_compressed_size_batch, then lzf_frame_size_fold_kernel (per frame) or lzf_stream_pack_kernel (per
// stream) over the job results alone: the (status, out_len) of the compress calls, nothing written, no checksum computed.
//
// lzf_frame_decompress_stream_device / lzf_frame_compress_stream_device: streams of back-to-back frames.  Decode: the stream scan
// (lzf_stream_scan_kernel, lzf_stream_walk.h, one lane per stream, two launches and two waits) lists the frames, which then go
// through the decode above (decode_frames); per pass, behind the decode launches, the count-only delivery finds every frame's
// length, lzf_stream_place_kernel gives every frame its place and the room left in its stream's output, and at the end
// lzf_stream_fold_kernel folds the frames' results into the streams'.  Compress: the pieces of every input are frames of the
// compress call above (compress_frames); lzf_stream_pack_kernel, in front of the assembly, puts each frame behind the one before.
// lzf_frame_stream_decompressed_size_device: the stream scan, the size query over every frame it lists (size_frames, the body of
// lzf_frame_decompressed_size_device), the decode's fold, and lzf_stream_index_kernel (lzf_stream_index.h's rules, one wavefront
// per stream) for the frame index; lzf_stream_index_locate is that header's locate on the host.
// lzf_frame_block_index_device: the size query over the caller's frames, then lzf_frame_block_index_kernel — the delivery body
// in its index mode, over the size query's descriptors, job results and block checksums — for the block index of every frame
// (lzf_block_index.h's rules).  lzf_frame_decompress_blocks_device: runs of consecutive blocks, planned from the caller's copies of
// the entries alone (no scan, no read-back): checksums, the decode of every block at its final place with its exact length as
// capacity, the stored copies, and lzf_block_run_fold_kernel, one wavefront per run, for status and out_len.
//
// One copy of each rule.  The walk is lzf_frame_scan.h's (the host driver runs the same header).  The passes of the memory budget
// are frame_jobs.h's split_passes, for all four *_many drivers.  The decode plan is plan_frames (the scan's summaries and table
// as frame_jobs.h's frames) and plan_pass (jobs, descriptors, checksum lists): decode_frames runs them per pass, the size query
// once with sizes_only.  The small arrays of a call travel in one Meta: one image, one upload, one event, typed accessors.  The
// one-wavefront-per-frame / per-stream / per-run kernels share wave_incl_scan.
#include <hip/hip_runtime.h>
#include <cstring>
#include <map>
#include <vector>
#include "../../include/lzfear_frame.h"
#include "lzf_frame_scan.h"
#include "lzf_stream_walk.h"
#include "lzf_stream_index.h"
#include "lzf_block_index.h"
#include "frame_jobs.h"
#include "lzf_frame_layout.h"
#include "lzf_chain_step.h"

namespace {

// per frame, scan pass 1 (fixed size: the host reads n of them back)
struct FSum {
    int32_t status;             // header error, or the walk's structural error (OK: the walk reached the EndMark)
    uint32_t flags;             // FLG byte | kLive (the header parsed) | kEndmark
    uint64_t consumed;          // bytes read when the header parse or the walk ended
    uint64_t n_blocks, n_compressed;
    uint64_t out_bound;         // sum of (compressed ? block_out_bound : len): the most the blocks can decode to
    uint64_t need;              // sum of (compressed ? block_out_bound : 0) + len + 256: the host driver's device memory accounting
    uint32_t max_len;           // largest block (compressed bytes)
    uint32_t want_content;      // content checksum behind the EndMark
    uint64_t block_maxsize;
};
static_assert(sizeof(FSum) == 64, "scan summary");
constexpr uint32_t kLive = 0x100u, kEndmark = 0x200u;

// per block, scan pass 2
struct TBlk { uint64_t off; uint32_t len; uint32_t want_sum; uint64_t end_off; };      // len | INCOMPRESSIBLE for a stored block
static_assert(sizeof(TBlk) == 24, "block table entry");

// per frame and per block of a pass, for the delivery kernel
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLinked = 1u, kCheckContent = 2u;
struct DFrameDesc {
    uint8_t* dst;               // the caller's output
    const uint8_t* stream;      // linked: the stream buffer
    uint64_t out_cap, scan_consumed, bmax;
    uint32_t blk0, nb;          // the frame's blocks: DBlkDesc [blk0, blk0 + nb) of the pass
    int32_t scan_err;
    uint32_t flags;             // kLinked | kCheckContent (EndMark read, content checksum present, walk ended without error)
    uint32_t frame, hash_idx, link_idx, pad;
};
struct DBlkDesc {
    const uint8_t* src;         // independent: the decoded block's slot, or the stored block in the input
    uint64_t end_off;           // input read once the block's checksum word is
    uint32_t job;               // decode job of the pass, kNone: stored
    uint32_t sum_idx;           // block checksum of the pass, kNone: none
    uint32_t want_sum, len;     // len: a stored block's length
};

// ---- the wave-wide sums of the one-wavefront-per-frame / per-stream kernels below
__device__ inline uint64_t wave_sum(uint64_t v) {
    for (int d = 32; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
    return v;
}
// inclusive scan over the 64 lanes: lane l gets v of lanes 0..l (the exclusive one is the result minus the lane's own v; lane 63
// holds the round's total, the carry into the next round of 64)
__device__ inline uint64_t wave_incl_scan(uint64_t v, uint32_t lane) {
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint64_t u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

__global__ __launch_bounds__(64) void lzf_frame_scan_kernel(const uint8_t* const* __restrict__ in, const uint64_t* __restrict__ in_len, uint32_t n,
                                                            FSum* __restrict__ sums, int32_t* __restrict__ d_status,
                                                            uint64_t* __restrict__ d_out_len, uint64_t* __restrict__ d_consumed) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= n) return;
    const uint8_t* p = in[f];
    const uint64_t len = in_len[f];
    const lzf_scan::Header h = lzf_scan::read_header(p, len);
    FSum s;
    memset(&s, 0, sizeof s);
    if (h.status != lzf_scan::OK) {
        s.status = h.status; s.consumed = h.consumed;
    } else {
        const uint64_t bmax = h.block_maxsize;
        const lzf_scan::Walk w = lzf_scan::walk_blocks(p, len, h, [&](const lzf_scan::Block& b) {
            const uint64_t bob = lzf_scan::block_out_bound(bmax, b.len);
            ++s.n_blocks;
            if (b.compressed) { ++s.n_compressed; s.out_bound += bob; s.need += bob; } else s.out_bound += b.len;
            s.need += (uint64_t)b.len + 256u;
            if (b.len > s.max_len) s.max_len = b.len;
        });
        s.status = w.status; s.consumed = w.consumed; s.want_content = w.want_content; s.block_maxsize = bmax;
        s.flags = h.flags | kLive | (w.endmark ? kEndmark : 0u);
    }
    sums[f] = s;
    if (d_status) {                     // final for a frame whose header fails; the delivery kernel overwrites the others
        d_status[f] = h.status; d_out_len[f] = 0; d_consumed[f] = h.status != lzf_scan::OK ? h.consumed : s.consumed;
    }
}

__global__ __launch_bounds__(64) void lzf_frame_table_kernel(const uint8_t* const* __restrict__ in, const uint64_t* __restrict__ in_len,
                                                             const uint64_t* __restrict__ blk0, const uint64_t* __restrict__ cnt, uint32_t n,
                                                             TBlk* __restrict__ table) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= n || blk0[f] == ~0ull) return;
    const uint8_t* p = in[f];
    const uint64_t len = in_len[f];
    const lzf_scan::Header h = lzf_scan::read_header(p, len);
    if (h.status != lzf_scan::OK) return;
    TBlk* t = table + blk0[f];
    const uint64_t room = cnt[f];       // what pass 1 found: never more entries than the host allocated
    uint64_t k = 0;
    lzf_scan::walk_blocks(p, len, h, [&](const lzf_scan::Block& b) {
        if (k < room) t[k] = TBlk{b.off, b.len | (b.compressed ? 0u : lzf_scan::INCOMPRESSIBLE), b.want_sum, b.end_off};
        ++k;
    });
}

// The reader's delivery loop (decompress.rs:198-288; frame.cpp's decompress_group) for one frame per wavefront, 64 blocks per
// round.  Per block, in stream order: block checksum (:228-235), codec status (CodecError), n > block_maxsize (:272-274), room
// in the caller's output (LZF_OUT_CAPACITY), n == 0 (the io::Read adapter stops at an empty block, :52-71,:286).  The first
// stop fixes status, out_len and consumed; without one the scan's status and consumed stand and the content checksum is due.
__global__ __launch_bounds__(64) void lzf_frame_deliver_kernel(const DFrameDesc* __restrict__ frames, const DBlkDesc* __restrict__ blks,
                                                               const lzf_decompress_job* __restrict__ jobs, const lzf_job_result* __restrict__ res,
                                                               const uint32_t* __restrict__ sums,
                                                               const uint8_t** __restrict__ r_src, uint8_t** __restrict__ r_dst, uint64_t* __restrict__ r_len,
                                                               const uint8_t** __restrict__ l_src, uint8_t** __restrict__ l_dst, uint64_t* __restrict__ l_len,
                                                               uint64_t* __restrict__ h_len, uint32_t* __restrict__ h_check,
                                                               int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len, uint64_t* __restrict__ d_consumed) {
#define LZF_DELIVER_COUNT_ONLY 0
#define LZF_DELIVER_INDEX 0
#include "frame_deliver_body.inc"
#undef LZF_DELIVER_INDEX
#undef LZF_DELIVER_COUNT_ONLY
}
// The size query's twins: delivery without the lists, and the chain step that carries the history as a length (lzf_chain_step.h).
__global__ __launch_bounds__(64) void lzf_frame_size_deliver_kernel(const DFrameDesc* __restrict__ frames, const DBlkDesc* __restrict__ blks,
                                                                    const lzf_decompress_job* __restrict__ jobs, const lzf_job_result* __restrict__ res,
                                                                    const uint32_t* __restrict__ sums,
                                                                    int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len, uint64_t* __restrict__ d_consumed) {
#define LZF_DELIVER_COUNT_ONLY 1
#define LZF_DELIVER_INDEX 0
#include "frame_deliver_body.inc"
#undef LZF_DELIVER_INDEX
#undef LZF_DELIVER_COUNT_ONLY
}
// The block index of a frame (lzf_frame_block_index_device): the delivery body once more, counting only, in its index mode.  One
// wavefront per frame, 64 blocks per round; the running output offset and the stop carry from round to round as in the delivery,
// and the rounds go on behind the stop.  Lane i writes entry i of the round (lzf_block_index.h's fill_entry, 48 bytes in vector
// stores) if the caller's room holds it; lane 0 writes the number of blocks found.
__global__ __launch_bounds__(64) void lzf_frame_block_index_kernel(const DFrameDesc* __restrict__ frames, const DBlkDesc* __restrict__ blks,
                                                                   const lzf_decompress_job* __restrict__ jobs, const lzf_job_result* __restrict__ res,
                                                                   const uint32_t* __restrict__ sums,
                                                                   lzf_frame_block* const* __restrict__ x_index, const uint64_t* __restrict__ x_cap,
                                                                   uint64_t* __restrict__ d_n_listed) {
#define LZF_DELIVER_COUNT_ONLY 1
#define LZF_DELIVER_INDEX 1
#include "frame_deliver_body.inc"
#undef LZF_DELIVER_INDEX
#undef LZF_DELIVER_COUNT_ONLY
}
__global__ __launch_bounds__(256) void lzf_chain_size_step_kernel(const lzf_chain_step* __restrict__ steps, lzf_chain_state* __restrict__ state,
                                                                  uint32_t n, lzf_decompress_job* __restrict__ jobs,
                                                                  const lzf_job_result* __restrict__ results) {
    lzf::chain_step<true, true>(steps, state, n, jobs, results);
}

// decompress.rs:207-211: FrameChecksumFail where the EndMark was read, nothing stopped the frame and the hash differs
__global__ __launch_bounds__(256) void lzf_frame_content_check_kernel(const uint32_t* __restrict__ got, const uint32_t* __restrict__ want,
                                                                      const uint32_t* __restrict__ check, const uint32_t* __restrict__ frame,
                                                                      uint32_t n, int32_t* __restrict__ d_status) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n && check[k] && got[k] != want[k]) d_status[frame[k]] = LZF_F_FRAME_CHECKSUM_FAIL;
}

// a frame that does not fit the memory budget alone
__global__ void lzf_frame_no_memory_kernel(uint32_t f, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed) {
    if (threadIdx.x == 0) { d_status[f] = LZF_E_NO_MEMORY; d_out_len[f] = 0; d_consumed[f] = 0; }
}

// ---- streams of back-to-back frames (lzf_stream_walk.h): the frames of a stream are consecutive frames of the call
// Stream scan, one lane per stream.  Launch one counts the frames of every stream (the failing last one included); launch two,
// with `starts`, lists where they begin: frame k of stream s at starts[first[s] + k].
__global__ __launch_bounds__(64) void lzf_stream_scan_kernel(const uint8_t* const* __restrict__ in, const uint64_t* __restrict__ in_len, uint32_t n,
                                                             uint64_t* __restrict__ counts, const uint64_t* __restrict__ first,
                                                             uint64_t* __restrict__ starts) {
    const uint32_t s = blockIdx.x * 64u + threadIdx.x;
    if (s >= n) return;
    if (!starts) { counts[s] = lzf_scan::walk_frames(in[s], in_len[s], [](uint64_t) {}).n_frames; return; }
    uint64_t* const t = starts + first[s];
    const uint64_t room = counts[s];    // what launch one found: never more entries than the host allocated
    uint64_t k = 0;
    lzf_scan::walk_frames(in[s], in_len[s], [&](uint64_t at) { if (k < room) t[k] = at; ++k; });
}

// the frames of one stream in one pass that have blocks to deliver: DFrameDesc [fd0, fd0 + nf) of the pass, in stream order
struct SSeg { uint32_t stream, fd0, nf, pad; };
// what a stream carries from pass to pass: the bytes placed so far, and whether a frame has ended it
struct SState { uint64_t run; uint32_t stopped, pad; };

// Placement, one wavefront per stream and pass, 64 frames per round.  f_status / f_len / f_consumed hold what the count-only
// delivery found for every frame with unlimited room.  The exclusive prefix of the lengths, behind the stream's running
// length, is where each frame goes; the stream goes on behind a frame only if that frame ended at its EndMark with LZF_OK and
// fits what is left of the stream's capacity.  The frame that ends the stream still gets its place and the room left — the
// delivery behind this kernel stops it at the right block — every frame behind it gets no blocks at all.
__global__ __launch_bounds__(64) void lzf_stream_place_kernel(const SSeg* __restrict__ segs, DFrameDesc* __restrict__ frames,
                                                              const uint8_t** __restrict__ hptr,
                                                              uint8_t* const* __restrict__ s_out, const uint64_t* __restrict__ s_cap,
                                                              SState* __restrict__ sstate, const int32_t* __restrict__ f_status,
                                                              const uint64_t* __restrict__ f_len, const uint64_t* __restrict__ f_consumed) {
    const SSeg G = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint8_t* const out = s_out[G.stream];
    const uint64_t cap = s_cap[G.stream];
    uint64_t run = sstate[G.stream].run;
    bool stopped = sstate[G.stream].stopped != 0;
    for (uint32_t base = 0; base < G.nf; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < G.nf;
        DFrameDesc* const F = frames + G.fd0 + (act ? i : 0u);
        uint64_t n = 0;
        bool complete = false;
        if (act) {
            const uint32_t f = F->frame;
            n = f_len[f];
            complete = f_status[f] == LZF_OK && F->scan_err == LZF_OK && f_consumed[f] == F->scan_consumed;
        }
        const uint64_t incl = wave_incl_scan(n, lane);
        const uint64_t at = run + (incl - n);                   // (at <= cap up to the first stop: every frame before it fits)
        const bool fits = at <= cap && cap - at >= n;
        const uint64_t stops = __ballot(act && !(complete && fits));
        const uint32_t first = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
        if (act) {
            const bool live = !stopped && lane <= first;
            uint8_t* const dst = live ? out + at : out;
            F->dst = dst; F->out_cap = live ? cap - at : 0ull;
            if (!live) { F->nb = 0u; F->flags &= ~kCheckContent; }
            if (F->hash_idx != kNone) hptr[F->hash_idx] = dst;
        }
        if (stops) stopped = true;
        else run += __shfl(incl, 63, 64);
    }
    if (lane == 0) { sstate[G.stream].run = run; sstate[G.stream].stopped = stopped ? 1u : 0u; }
}

// a frame that does not fit the memory budget alone ends its stream
__global__ void lzf_stream_no_memory_kernel(uint32_t f, uint32_t stream, SState* sstate, int32_t* f_status, uint64_t* f_len, uint64_t* f_consumed) {
    if (threadIdx.x == 0) { f_status[f] = LZF_E_NO_MEMORY; f_len[f] = 0; f_consumed[f] = 0; sstate[stream].stopped = 1u; }
}

// The stream rule over the frames' final results, one wavefront per stream: stream s is frames [first[s], first[s + 1]).  Every
// frame up to and including the first one that does not end at its EndMark with LZF_OK (f_full: the frame's length up to
// there, ~0 where the scan already failed) adds its output and its consumed bytes; the frames before it are the stream's frames.
__global__ __launch_bounds__(64) void lzf_stream_fold_kernel(const uint64_t* __restrict__ first, const int32_t* __restrict__ f_status,
                                                             const uint64_t* __restrict__ f_len, const uint64_t* __restrict__ f_consumed,
                                                             const uint64_t* __restrict__ f_full,
                                                             int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len,
                                                             uint64_t* __restrict__ d_consumed, uint64_t* __restrict__ d_n_frames) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint64_t a = first[s], b = first[s + 1];
    uint64_t out = 0, pos = 0, good = 0;
    int st = LZF_OK;
    for (uint64_t base = a; base < b; base += 64u) {
        const uint64_t f = base + lane;
        const bool act = f < b;
        const uint64_t n = act ? f_len[f] : 0ull, c = act ? f_consumed[f] : 0ull;
        const int code = act ? f_status[f] : LZF_OK;
        const uint64_t stops = __ballot(act && (code != LZF_OK || c != f_full[f]));
        const uint32_t stop_at = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
        const bool take = act && lane <= stop_at;
        out += wave_sum(take ? n : 0ull); pos += wave_sum(take ? c : 0ull);
        good += (uint64_t)__popcll(__ballot(act && lane < stop_at));
        if (stops) { st = __shfl(code, (int)stop_at, 64); break; }
    }
    if (lane != 0) return;
    d_status[s] = st; d_out_len[s] = out; d_consumed[s] = pos;
    if (d_n_frames) d_n_frames[s] = good;
}

// ---- compress: per frame and per block of a pass, for the assembly kernel
struct CFrameDesc {
    uint8_t* dst;               // the caller's output
    uint32_t blk0, nb;          // the frame's blocks: CBlkDesc [blk0, blk0 + nb) of the pass, in block order
    int32_t status0;            // what the host decided: LZF_OK, LZF_OUT_CAPACITY or the block size's error (then nb = 0)
    uint32_t frame, hash_idx;   // hash_idx: the frame's content checksum in the pass, kNone: none
    uint32_t hdr_idx;           // the frame's header image (streams with a content size: one per piece length), 0: the call's one
};
static_assert(sizeof(CFrameDesc) == 32, "compress frame descriptor");
struct CBlkDesc {
    const uint8_t* raw;         // the block in the caller's input: a stored block's payload
    const uint8_t* slot;        // its job's output: a compressed block's payload
    uint32_t job, raw_len;      // job of the pass (its result), the block's length
};
constexpr uint32_t kBlockSums = 1u, kContentSum = 2u;

// compress.rs:221-281 once the blocks are compressed, one frame per wavefront, 64 blocks per round (lzf_frame_layout.h's rule).
// Round one finds the frame's status: the first block, in block order, whose status is neither LZF_OK nor LZF_OUTPUT_FULL.
// Round two is a wave-wide exclusive scan of block_span: where each block's length word, payload and checksum go.  A frame that
// stays LZF_OK gets its header (the call's one image), length words and EndMark here; the payload copies (r_*), the checksum
// words (s_at: block i's, c_at: the content's) are left to the launches behind.  A failed frame gets no byte: empty ranges and
// NULL checksum places.  Every word is written bytewise: frames start at any address.
__global__ __launch_bounds__(64) void lzf_frame_assemble_kernel(const CFrameDesc* __restrict__ frames, const CBlkDesc* __restrict__ blks,
                                                                const lzf_job_result* __restrict__ res, const uint8_t* __restrict__ hdr,
                                                                uint32_t hdr_len, uint32_t flags,
                                                                const uint8_t** __restrict__ r_src, uint8_t** __restrict__ r_dst,
                                                                uint64_t* __restrict__ r_len, uint8_t** __restrict__ s_at, uint8_t** __restrict__ c_at,
                                                                int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len) {
    const CFrameDesc F = frames[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const bool bsum = (flags & kBlockSums) != 0, csum = (flags & kContentSum) != 0;
    int st = F.status0;
    for (uint32_t base = 0; st == LZF_OK && base < F.nb; base += 64u) {
        const uint32_t i = base + lane;
        lzf_layout::Block b{0u, false, false, LZF_OK};
        if (i < F.nb) { const CBlkDesc c = blks[F.blk0 + i]; const lzf_job_result r = res[c.job]; b = lzf_layout::block_of(r.status, r.out_len, c.raw_len); }
        const uint64_t bad = __ballot(b.bad);
        if (bad) st = __shfl(b.status, (int)__builtin_ctzll(bad), 64);
    }
    const bool ok = st == LZF_OK;
    uint64_t w = hdr_len;
    for (uint32_t base = 0; base < F.nb; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < F.nb;
        CBlkDesc c{nullptr, nullptr, 0u, 0u};
        lzf_layout::Block b{0u, false, false, LZF_OK};
        if (act) { c = blks[F.blk0 + i]; const lzf_job_result r = res[c.job]; b = lzf_layout::block_of(r.status, r.out_len, c.raw_len); }
        const uint64_t span = act ? lzf_layout::block_span(b.len, bsum) : 0ull;
        const uint64_t incl = wave_incl_scan(span, lane);
        if (act) {
            const uint32_t g = F.blk0 + i;
            uint8_t* const at = F.dst + (w + incl - span);      // the block's length word
            if (ok) {
                lzf_layout::wr32(at, lzf_layout::size_word(b));
                r_src[g] = b.stored ? c.raw : c.slot; r_dst[g] = at + 4; r_len[g] = b.len;
            } else { r_src[g] = c.raw; r_dst[g] = F.dst; r_len[g] = 0; }
            if (bsum) s_at[g] = ok ? at + 4 + b.len : nullptr;
        }
        w += __shfl(incl, 63, 64);
    }
    if (ok && lane < hdr_len) F.dst[lane] = hdr[F.hdr_idx * lzf_layout::kMaxHeader + lane];
    if (ok && lane < 4u) F.dst[w + lane] = 0;                   // EndMark (:277)
    if (lane != 0) return;
    d_status[F.frame] = st;
    d_out_len[F.frame] = ok ? w + lzf_layout::tail_len(csum) : 0ull;
    if (F.hash_idx != kNone) c_at[F.hash_idx] = ok ? F.dst + w + 4 : nullptr;     // (:279-281)
}

// lzf_frame_compressed_size_device: the assembly kernel's rule with nothing assembled.  One wavefront per frame, 64 blocks per
// round: the first block, in block order, whose status is neither LZF_OK nor LZF_OUTPUT_FULL fails the frame with out_len 0;
// otherwise the frame is its header, every block's block_span (a refused block counts its raw length: stored), the EndMark and
// the content checksum's 4 bytes when the settings ask for one.  Nothing but d_status / d_out_len is written.
__global__ __launch_bounds__(64) void lzf_frame_size_fold_kernel(const CFrameDesc* __restrict__ frames, const CBlkDesc* __restrict__ blks,
                                                                 const lzf_job_result* __restrict__ res, uint32_t hdr_len, uint32_t flags,
                                                                 int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len) {
    const CFrameDesc F = frames[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const bool bsum = (flags & kBlockSums) != 0, csum = (flags & kContentSum) != 0;
    int st = F.status0;
    uint64_t w = hdr_len;
    for (uint32_t base = 0; st == LZF_OK && base < F.nb; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < F.nb;
        lzf_layout::Block b{0u, false, false, LZF_OK};
        if (act) { const CBlkDesc c = blks[F.blk0 + i]; const lzf_job_result r = res[c.job]; b = lzf_layout::block_of(r.status, r.out_len, c.raw_len); }
        const uint64_t bad = __ballot(b.bad);
        if (bad) { st = __shfl(b.status, (int)__builtin_ctzll(bad), 64); break; }
        w += wave_sum(act ? lzf_layout::block_span(b.len, bsum) : 0ull);
    }
    if (lane != 0) return;
    d_status[F.frame] = st;
    d_out_len[F.frame] = st == LZF_OK ? w + lzf_layout::tail_len(csum) : 0ull;
}

// Streams of frames (lzf_frame_compress_stream_device): the frames of one stream, CFrameDesc [fd0, fd0 + nf) of the pass, go
// back to back into the stream's output.  One wavefront per stream, a lane per frame, 64 frames per round: every frame's exact
// length from its blocks' job results (lzf_frame_layout.h's rule, the assembly kernel's), a wave-wide exclusive scan of the
// lengths for its place.  The first block status, in stream order, that is neither LZF_OK nor LZF_OUTPUT_FULL fails the whole
// stream: every frame gets it as status0, and the assembly kernel behind writes no byte of them.
struct CSeg { uint8_t* out; uint32_t fd0, nf, stream; int32_t status0; };
__global__ __launch_bounds__(64) void lzf_stream_pack_kernel(const CSeg* __restrict__ segs, CFrameDesc* __restrict__ frames,
                                                             const CBlkDesc* __restrict__ blks, const lzf_job_result* __restrict__ res,
                                                             uint32_t hdr_len, uint32_t flags,
                                                             int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len) {
    const CSeg G = segs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    const bool bsum = (flags & kBlockSums) != 0, csum = (flags & kContentSum) != 0;
    int st = G.status0;
    uint64_t w = 0;
    if (st == LZF_OK) {
        for (uint32_t base = 0; base < G.nf; base += 64u) {
            const uint32_t i = base + lane;
            const bool act = i < G.nf;
            uint64_t len = 0;
            int bad = LZF_OK;
            if (act) {
                const CFrameDesc F = frames[G.fd0 + i];
                len = hdr_len + lzf_layout::tail_len(csum);
                for (uint32_t k = 0; k < F.nb; ++k) {
                    const CBlkDesc c = blks[F.blk0 + k];
                    const lzf_job_result r = res[c.job];
                    const lzf_layout::Block b = lzf_layout::block_of(r.status, r.out_len, c.raw_len);
                    if (b.bad && bad == LZF_OK) bad = b.status;
                    len += lzf_layout::block_span(b.len, bsum);
                }
            }
            const uint64_t incl = wave_incl_scan(len, lane);
            if (act) frames[G.fd0 + i].dst = G.out + (w + incl - len);
            const uint64_t bads = __ballot(act && bad != LZF_OK);
            if (bads && st == LZF_OK) st = __shfl(bad, (int)__builtin_ctzll(bads), 64);
            w += __shfl(incl, 63, 64);
        }
        if (st != LZF_OK) for (uint32_t i = lane; i < G.nf; i += 64u) frames[G.fd0 + i].status0 = st;
    }
    if (lane != 0) return;
    d_status[G.stream] = st;
    d_out_len[G.stream] = st == LZF_OK ? w : 0ull;
}

// the checksum words at their unaligned places (NULL: the frame failed)
__global__ __launch_bounds__(256) void lzf_frame_patch_kernel(uint8_t* const* __restrict__ at, const uint32_t* __restrict__ val, uint32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n && at[k]) lzf_layout::wr32(at[k], val[k]);
}

// ---- runs of blocks (lzf_frame_decompress_blocks_device): per run and per block, for the fold kernel
struct RRunDesc { uint32_t blk0, nb; int32_t status0; uint32_t run; };      // status0: LZF_OK, or LZF_OUT_CAPACITY (then nb = 0)
struct RBlkDesc {
    const uint8_t* sum_at;      // the block's checksum word in the input (any alignment), NULL: none
    uint64_t out_len;           // the entry's
    uint32_t job;               // decode job of the call, kNone: stored
    uint32_t sum_idx;           // block checksum of the call, kNone: none
};
static_assert(sizeof(RBlkDesc) == 24, "run block descriptor");

// The results of the runs, one wavefront per run, 64 blocks per round.  Per block, in block order: the checksum of its payload
// against the word in the input, its job's status, its job's length against the entry's.  The first block that fails fixes the
// run's status; out_len is the exclusive prefix of the entries' lengths at that block (wave_incl_scan within the round, the
// running sum from round to round), or the total.  A stored block cannot fail but for its checksum.
__global__ __launch_bounds__(64) void lzf_block_run_fold_kernel(const RRunDesc* __restrict__ runs, const RBlkDesc* __restrict__ blks,
                                                                const lzf_job_result* __restrict__ res, const uint32_t* __restrict__ sums,
                                                                int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len) {
    const RRunDesc R = runs[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint64_t w = 0;
    int st = R.status0;
    for (uint32_t base = 0; base < R.nb; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < R.nb;
        uint64_t n = 0;
        int code = LZF_OK;
        if (act) {
            const RBlkDesc b = blks[R.blk0 + i];
            n = b.out_len;
            if (b.sum_idx != kNone && sums[b.sum_idx] != lzf_scan::rd32(b.sum_at)) code = LZF_F_BLOCK_CHECKSUM_FAIL;
            else if (b.job != kNone) {
                const lzf_job_result r = res[b.job];
                if (r.status >= LZF_UNEXPECTED_END && r.status <= LZF_INVALID_DEDUP_OFFSET) code = r.status;
                else if (r.status != LZF_OK || r.out_len != n) code = LZF_CONTRACT;      // (LZF_OUT_CAPACITY: no room in out_len bytes)
            }
        }
        const uint64_t incl = wave_incl_scan(n, lane);
        const uint64_t fails = __ballot(act && code != LZF_OK);
        if (fails) {
            const int first = (int)__builtin_ctzll(fails);
            st = __shfl(code, first, 64);
            w += __shfl(incl - n, first, 64);
            break;
        }
        w += __shfl(incl, 63, 64);
    }
    if (lane != 0) return;
    d_status[R.run] = st; d_out_len[R.run] = w;
}

// ---- host side ------------------------------------------------------------------------------------------------------
struct PoolAlloc {                      // stream-ordered scratch, handed back in stream order on every way out
    void* p = nullptr; hipStream_t st = nullptr;
    explicit PoolAlloc(hipStream_t s) : st(s) {}
    ~PoolAlloc() { if (p) (void)hipFreeAsync(p, st); }
    bool get(size_t bytes) { if (hipMallocAsync(&p, bytes ? bytes : 256, st) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; } return true; }
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(p) + off); }
};
// (on failure: nothing enqueued may still read host memory of the call when it returns)
#define DEV_TRY(e) do { if ((e) != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(st); return LZF_E_HIP; } } while (0)
#define RC_TRY(e) do { const int rc__ = (e); if (rc__ != LZF_OK) { (void)hipStreamSynchronize(st); return rc__; } } while (0)
#define KERNEL(...) do { hipLaunchKernelGGL(__VA_ARGS__); DEV_TRY(hipGetLastError()); } while (0)

int usable_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return LZF_E_NO_DEVICE; }
    return LZF_OK;
}
using lzf_frame_jobs::up256;

// The small arrays of a call in one pool allocation: the host image (every list the host builds: one upload) and, behind it, the
// scratch that only kernels write.  add / room hand out offsets while the call is planned; after upload(), img<T>(off) and
// scr<T>(off) are their typed device addresses.  wait() returns once the image has left host memory (the kernels run on).
struct Meta {
    hipStream_t st;
    std::vector<uint8_t> image; size_t scratch = 0;
    PoolAlloc mem; hipEvent_t uploaded = nullptr;
    explicit Meta(hipStream_t s) : st(s), mem(s) {}
    ~Meta() { if (uploaded) (void)hipEventDestroy(uploaded); }
    size_t add(const void* p, size_t bytes) { const size_t o = image.size(); image.resize(up256(o + bytes)); if (bytes && p) memcpy(image.data() + o, p, bytes); return o; }
    template <class T> size_t add(const std::vector<T>& v) { return add(v.data(), sizeof(T) * v.size()); }
    size_t room(size_t bytes) { const size_t o = scratch; scratch = up256(scratch + bytes); return o; }
    template <class T> T* img(size_t off) const { return mem.at<T>(off); }
    template <class T> T* scr(size_t off) const { return mem.at<T>(image.size() + off); }
    int upload(bool zero_scratch) {         // zero_scratch: chain states, range and hash lengths start at 0
        if (!mem.get(image.size() + scratch)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
        DEV_TRY(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        if (!image.empty()) DEV_TRY(hipMemcpyAsync(mem.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
        DEV_TRY(hipEventRecord(uploaded, st));
        if (zero_scratch && scratch) DEV_TRY(hipMemsetAsync(scr<uint8_t>(0), 0, scratch, st));
        return LZF_OK;
    }
    int wait() { if (uploaded) DEV_TRY(hipEventSynchronize(uploaded)); return LZF_OK; }     // (nothing uploaded: nothing to wait for)
};

// lzf_frame_set_memory_budget's value, or half of the free device memory
int pass_budget(hipStream_t st, size_t* budget) {
    *budget = lzf_frame_jobs::memory_budget();
    if (!*budget) { size_t free_b = 0, total_b = 0; DEV_TRY(hipMemGetInfo(&free_b, &total_b)); *budget = free_b / 2; }
    return LZF_OK;
}
// frames [first[s], first[s + 1]) are stream s: the stream of every frame
std::vector<uint32_t> streams_of(uint32_t n_streams, const uint64_t* first) {
    std::vector<uint32_t> of((size_t)first[n_streams]);
    for (uint32_t s = 0; s < n_streams; ++s) for (uint64_t f = first[s]; f < first[s + 1]; ++f) of[(size_t)f] = s;
    return of;
}

// What the scan of n frames brings back to the host: the summaries (pass 1) and, with scan_table, the block table (pass 2):
// frame f's blocks are table[blk0[f], blk0[f] + cnt[f]).  `args` keeps [ptrs | lens | blk0 | cnt] on the device between the two.
struct Scan {
    PoolAlloc args;
    std::vector<FSum> sum;
    std::vector<uint64_t> blk0, cnt;
    std::vector<TBlk> table;
    explicit Scan(hipStream_t st) : args(st) {}
    bool live(uint32_t f) const { return (sum[f].flags & kLive) != 0; }
};

// Scan pass 1 of n frames: summaries back on the host (the call's first wait).
int scan_summaries(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, Scan& sc,
                   int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed) {
    PoolAlloc& args = sc.args;
    const size_t o_sum = up256(32 * (size_t)n);
    if (!args.get(o_sum + sizeof(FSum) * (size_t)n)) return LZF_E_HIP;
    std::vector<uint64_t> h(2 * (size_t)n);
    for (uint32_t f = 0; f < n; ++f) { h[f] = reinterpret_cast<uintptr_t>(d_in[f]); h[n + f] = in_len[f]; }
    DEV_TRY(hipMemcpyAsync(args.p, h.data(), 16 * (size_t)n, hipMemcpyHostToDevice, st));
    KERNEL(lzf_frame_scan_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, args.at<const uint8_t* const>(0), args.at<const uint64_t>(8 * (size_t)n), n,
           args.at<FSum>(o_sum), d_status, d_out_len, d_consumed);
    sc.sum.resize(n);
    DEV_TRY(hipMemcpyAsync(sc.sum.data(), args.at<FSum>(o_sum), sizeof(FSum) * (size_t)n, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    return LZF_OK;
}

// Scan pass 2: the block table of every frame whose header parses, back on the host (the call's second wait).
int scan_table(uint32_t n, hipStream_t st, Scan& sc) {
    sc.blk0.assign(n, ~0ull); sc.cnt.assign(n, 0);
    uint64_t n_table = 0;
    for (uint32_t f = 0; f < n; ++f) if (sc.live(f)) { sc.blk0[f] = n_table; sc.cnt[f] = sc.sum[f].n_blocks; n_table += sc.sum[f].n_blocks; }
    if (n_table > 0x7FFFFFFFull) { (void)hipStreamSynchronize(st); return LZF_E_INVALID; }
    sc.table.resize((size_t)n_table);
    if (n_table) {
        std::vector<uint64_t> h(2 * (size_t)n);
        memcpy(h.data(), sc.blk0.data(), 8 * (size_t)n); memcpy(h.data() + n, sc.cnt.data(), 8 * (size_t)n);
        DEV_TRY(hipMemcpyAsync(sc.args.at<uint64_t>(16 * (size_t)n), h.data(), 16 * (size_t)n, hipMemcpyHostToDevice, st));
        PoolAlloc tab(st);
        if (!tab.get(sizeof(TBlk) * (size_t)n_table)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
        KERNEL(lzf_frame_table_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, sc.args.at<const uint8_t* const>(0), sc.args.at<const uint64_t>(8 * (size_t)n),
               sc.args.at<const uint64_t>(16 * (size_t)n), sc.args.at<const uint64_t>(24 * (size_t)n), n, tab.at<TBlk>(0));
        DEV_TRY(hipMemcpyAsync(sc.table.data(), tab.p, sizeof(TBlk) * (size_t)n_table, hipMemcpyDeviceToHost, st));
        DEV_TRY(hipStreamSynchronize(st));
    }
    return LZF_OK;
}

// One pass of the decode plan: frames [f0, f1) of the call, everything the kernels read in the call's image (i_*) and everything
// they write in its scratch (s_*).
struct Pass {
    uint32_t f0 = 0, f1 = 0;
    bool no_memory = false;
    std::vector<lzf_frame_jobs::Frame> jf;          // the frames whose header parsed, jf_frame: which frame of the call each is
    std::vector<uint32_t> jf_frame;
    lzf_frame_jobs::Plan plan;
    uint32_t n_frames = 0, n_blks = 0, n_sums = 0, n_hash = 0, n_link = 0;
    uint64_t ind_max = 0, link_max = 0;
    // image offsets
    size_t i_jobs = 0, i_steps = 0, i_sptr = 0, i_slen = 0, i_frames = 0, i_blks = 0, i_hptr = 0, i_hwant = 0, i_hframe = 0, i_segs = 0;
    uint32_t n_segs = 0;                // streams: the pass's SSeg list
    // scratch offsets
    size_t s_res = 0, s_state = 0, s_sums = 0, s_rsrc = 0, s_rdst = 0, s_rlen = 0, s_lsrc = 0, s_ldst = 0, s_llen = 0, s_hlen = 0, s_hcheck = 0, s_hout = 0;
    std::vector<lzf_frame_jobs::Frame*> frames() { std::vector<lzf_frame_jobs::Frame*> l; for (auto& J : jf) l.push_back(&J); return l; }
};

// The decode plan, step one: the pass's frames as frame_jobs.h's frames, from the scan summaries and the block table (the blocks
// as device addresses in the caller's input), and their output layout.
void plan_frames(Pass& P, const uint8_t* const* d_in, const Scan& sc) {
    P.jf.reserve(P.f1 - P.f0);
    for (uint32_t f = P.f0; f < P.f1; ++f) {
        if (!sc.live(f)) continue;
        const FSum& S = sc.sum[f];
        P.jf.emplace_back();
        lzf_frame_jobs::Frame& J = P.jf.back();
        J.linked = !(S.flags & lzf_scan::FL_INDEP); J.bmax = (size_t)S.block_maxsize; J.consumed = (size_t)S.consumed;
        for (uint64_t k = 0; k < sc.cnt[f]; ++k) {
            const TBlk& t = sc.table[sc.blk0[f] + k];
            J.blocks.push_back({d_in[f] + t.off, t.len & ~lzf_scan::INCOMPRESSIBLE, (t.len & lzf_scan::INCOMPRESSIBLE) == 0});
        }
        P.jf_frame.push_back(f);
    }
    lzf_frame_jobs::layout(P.frames(), P.plan);
}

// What the plan's step two is told about the call.  The size query (lzf_frame_decompressed_size_device) has neither outputs nor
// slots: sizes_only, every address NULL, unlimited room, no copy lists and no content checksum.
struct DecodeCall {
    bool sizes_only;
    uint8_t* dslots; const uint8_t* d_dict; size_t dict_len;
    uint8_t* const* d_out; const size_t* out_cap;
    const uint32_t* stream_of;          // streams: the stream of every frame (unlimited room for the count; the placement sets dst and out_cap)
};

// The decode plan, step two: jobs and chain steps (frame_jobs.h), the delivery kernel's descriptors and the checksum lists of the
// pass, into the call's image; room for what the kernels write, in its scratch.
int plan_pass(Pass& P, const Scan& sc, const DecodeCall& c, Meta& meta) {
    lzf_frame_jobs::build(P.frames(), P.plan, c.dslots, c.d_dict, c.dict_len, c.sizes_only);
    if (P.plan.jobs.size() > 0x7FFFFFFFull) return LZF_E_INVALID;
    std::vector<DFrameDesc> fd; std::vector<DBlkDesc> bd;
    std::vector<const uint8_t*> sptr; std::vector<uint64_t> slen;
    std::vector<const uint8_t*> hptr; std::vector<uint32_t> hwant, hframe;
    std::vector<SSeg> segs;
    for (size_t q = 0; q < P.jf.size(); ++q) {
        const lzf_frame_jobs::Frame& J = P.jf[q];
        const uint32_t f = P.jf_frame[q];
        const FSum& S = sc.sum[f];
        const bool chained = J.linked && !J.blocks.empty();
        DFrameDesc d;
        memset(&d, 0, sizeof d);
        d.out_cap = c.sizes_only || c.stream_of ? ~0ull : c.out_cap[f]; d.scan_consumed = S.consumed; d.bmax = J.bmax;
        d.blk0 = (uint32_t)bd.size(); d.nb = (uint32_t)J.blocks.size(); d.scan_err = S.status;
        d.flags = (J.linked ? kLinked : 0u);
        d.frame = f; d.hash_idx = kNone; d.link_idx = kNone;
        if (!c.sizes_only) {
            d.dst = c.d_out[f]; d.stream = chained ? c.dslots + J.out_off : nullptr;
            if ((S.flags & kEndmark) && (S.flags & lzf_scan::FL_CSUM) && S.status == LZF_OK) {
                d.flags |= kCheckContent; d.hash_idx = (uint32_t)hptr.size();
                hptr.push_back(c.d_out[f]); hwant.push_back(S.want_content); hframe.push_back(f);
            }
            if (chained) {
                d.link_idx = P.n_link++;
                const uint64_t m = (uint64_t)J.blocks.size() * J.bmax, cap = c.out_cap[f] < m ? c.out_cap[f] : m;
                if (cap > P.link_max) P.link_max = cap;
            } else if (!J.blocks.empty() && J.bmax > P.ind_max) P.ind_max = J.bmax;
        }
        const bool bsum = (S.flags & lzf_scan::FL_BLOCKSUM) != 0;
        for (size_t i = 0; i < J.blocks.size(); ++i) {
            const TBlk& t = sc.table[sc.blk0[f] + i];
            DBlkDesc b;
            b.src = c.sizes_only ? nullptr : J.blocks[i].compressed ? (J.linked ? nullptr : c.dslots + J.slot[i]) : J.blocks[i].src;
            b.end_off = t.end_off; b.job = J.job[i] == SIZE_MAX ? kNone : (uint32_t)J.job[i];
            b.sum_idx = kNone; b.want_sum = t.want_sum; b.len = J.blocks[i].len;
            if (bsum) { b.sum_idx = (uint32_t)sptr.size(); sptr.push_back(J.blocks[i].src); slen.push_back(J.blocks[i].len); }
            bd.push_back(b);
        }
        if (c.stream_of) {
            if (segs.empty() || segs.back().stream != c.stream_of[f]) segs.push_back(SSeg{c.stream_of[f], (uint32_t)fd.size(), 0u, 0u});
            ++segs.back().nf;
        }
        fd.push_back(d);
    }
    P.n_segs = (uint32_t)segs.size(); P.i_segs = meta.add(segs);
    P.n_frames = (uint32_t)fd.size(); P.n_blks = (uint32_t)bd.size(); P.n_sums = (uint32_t)sptr.size(); P.n_hash = (uint32_t)hptr.size();
    P.i_jobs = meta.add(P.plan.jobs); P.i_steps = meta.add(P.plan.csteps);
    P.i_sptr = meta.add(sptr); P.i_slen = meta.add(slen);
    P.i_frames = meta.add(fd); P.i_blks = meta.add(bd);
    P.i_hptr = meta.add(hptr); P.i_hwant = meta.add(hwant); P.i_hframe = meta.add(hframe);
    P.s_res = meta.room(sizeof(lzf_job_result) * P.plan.jobs.size()); P.s_state = meta.room(sizeof(lzf_chain_state) * P.plan.n_chain);
    P.s_sums = meta.room(4 * (size_t)P.n_sums);
    if (c.sizes_only) return LZF_OK;
    P.s_rsrc = meta.room(8 * (size_t)P.n_blks); P.s_rdst = meta.room(8 * (size_t)P.n_blks); P.s_rlen = meta.room(8 * (size_t)P.n_blks);
    P.s_lsrc = meta.room(8 * (size_t)P.n_link); P.s_ldst = meta.room(8 * (size_t)P.n_link); P.s_llen = meta.room(8 * (size_t)P.n_link);
    P.s_hlen = meta.room(8 * (size_t)P.n_hash); P.s_hcheck = meta.room(4 * (size_t)P.n_hash); P.s_hout = meta.room(4 * (size_t)P.n_hash);
    return LZF_OK;
}

// What makes the frames of a decode call the frames of streams (lzf_frame_decompress_stream_device): stream s is frames
// [first[s], first[s + 1]) of the call and owns one output.  d_out / out_cap of decode_frames then hold, per frame, its stream's
// output and capacity; d_status / d_out_len / d_consumed are per-frame scratch, the s_* arrays get the streams' results.
struct StreamCtx {
    uint32_t n_streams;
    const uint64_t* first;              // host, n_streams + 1 entries
    uint8_t* const* s_out;              // host, per stream: device address of its output
    const size_t* s_cap;
    SState* d_sstate;                   // device, zeroed: carried from pass to pass
    int32_t* s_status; uint64_t* s_out_len; uint64_t* s_consumed; uint64_t* s_n_frames;    // device, per stream
};

// lzf_frame_decompress_device_many's work for n >= 1 frames on a usable device; with `sx` the frames are placed behind each
// other in their streams' outputs on the device (count-only delivery, lzf_stream_place_kernel) and folded into per-stream
// results at the end (lzf_stream_fold_kernel).
int decode_frames(const uint32_t n, const uint8_t* const* d_in, const size_t* in_len, const uint8_t* d_dict, size_t dict_len,
                  uint8_t* const* d_out, const size_t* out_cap, uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status,
                  hipStream_t st, const StreamCtx* sx) {
    // ---- scan: summaries (wait 1), the block table of every frame whose header parses (wait 2)
    Scan sc(st);
    RC_TRY(scan_summaries(n, d_in, in_len, st, sc, d_status, d_out_len, d_consumed));
    RC_TRY(scan_table(n, st, sc));
    // ---- passes: as many frames as the memory budget holds (frame_jobs.h's split_passes), with the host driver's accounting
    //      (frame.cpp); a frame that does not fit alone gets LZF_E_NO_MEMORY
    std::vector<size_t> need(n, 0);
    for (uint32_t f = 0; f < n; ++f) if (sc.live(f)) need[f] = (size_t)sc.sum[f].consumed + 2 * (size_t)sc.sum[f].need + 4096;
    size_t budget = 0;
    RC_TRY(pass_budget(st, &budget));
    std::vector<std::pair<uint32_t, uint32_t>> cuts;
    lzf_frame_jobs::split_passes(need.data(), n, budget, nullptr, cuts);
    std::vector<Pass> passes(cuts.size());
    // ---- output layout of every pass; the passes share one slot allocation (stream order: pass p + 1 decodes after pass p's copy)
    size_t slots_bytes = 0;
    for (size_t p = 0; p < cuts.size(); ++p) {
        Pass& P = passes[p];
        P.f0 = cuts[p].first; P.f1 = cuts[p].second;
        P.no_memory = P.f1 == P.f0 + 1 && need[P.f0] > budget;
        if (P.no_memory) continue;
        plan_frames(P, d_in, sc);
        if (P.plan.out_total > slots_bytes) slots_bytes = P.plan.out_total;
    }
    PoolAlloc slots(st);
    if (slots_bytes && !slots.get(slots_bytes)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
    // ---- jobs and descriptors of every pass into one image
    const std::vector<uint32_t> stream_of = sx ? streams_of(sx->n_streams, sx->first) : std::vector<uint32_t>();
    const DecodeCall call{false, slots.at<uint8_t>(0), d_dict, dict_len, d_out, out_cap, sx ? stream_of.data() : nullptr};
    Meta meta(st);
    for (Pass& P : passes) if (!P.no_memory) RC_TRY(plan_pass(P, sc, call, meta));
    size_t i_sout = 0, i_scap = 0, i_first = 0, i_full = 0;
    if (sx) {
        std::vector<uint64_t> cap(sx->s_cap, sx->s_cap + sx->n_streams), full(n);
        for (uint32_t f = 0; f < n; ++f) full[f] = sc.live(f) && sc.sum[f].status == LZF_OK ? sc.sum[f].consumed : ~0ull;
        i_sout = meta.add(sx->s_out, sizeof(void*) * sx->n_streams); i_scap = meta.add(cap);
        i_first = meta.add(sx->first, 8 * ((size_t)sx->n_streams + 1)); i_full = meta.add(full);
    }
    // ---- one upload, then the kernels of every pass
    RC_TRY(meta.upload(true));
    for (Pass& P : passes) {
        if (P.no_memory && sx) { KERNEL(lzf_stream_no_memory_kernel, dim3(1), dim3(64), 0, st, P.f0, stream_of[P.f0], sx->d_sstate, d_status, d_out_len, d_consumed); continue; }
        if (P.no_memory) { KERNEL(lzf_frame_no_memory_kernel, dim3(1), dim3(64), 0, st, P.f0, d_status, d_out_len, d_consumed); continue; }
        if (!P.n_frames) continue;
        lzf_decompress_job* const d_jobs = meta.img<lzf_decompress_job>(P.i_jobs);
        lzf_job_result* const d_res = meta.scr<lzf_job_result>(P.s_res);
        uint32_t* const d_sums = meta.scr<uint32_t>(P.s_sums);
        const DFrameDesc* const d_frames = meta.img<const DFrameDesc>(P.i_frames);
        const DBlkDesc* const d_blks = meta.img<const DBlkDesc>(P.i_blks);
        if (P.n_sums) RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_sptr), meta.img<const uint64_t>(P.i_slen), d_sums, P.n_sums, st));
        const lzf_frame_jobs::Plan& pl = P.plan;
        for (size_t k = 0; k < pl.n_steps; ++k) {
            if (pl.n_chain) RC_TRY(lzf_chain_decompress_step_trimmed(meta.img<const lzf_chain_step>(P.i_steps) + k * pl.n_chain, meta.scr<lzf_chain_state>(P.s_state),
                                                             pl.n_chain, d_jobs, d_res, st));
            const size_t a = pl.step_off[k], c = pl.step_off[k + 1] - a;
            if (c) RC_TRY(lzf_decompress_batch_sized(d_jobs + a, d_res + a, (uint32_t)c, lzf_frame_jobs::step_max_input(pl, k), st));
        }
        if (sx) {                           // where every frame goes is known only now: count, then place
            KERNEL(lzf_frame_size_deliver_kernel, dim3(P.n_frames), dim3(64), 0, st, d_frames, d_blks, (const lzf_decompress_job*)d_jobs,
                   (const lzf_job_result*)d_res, (const uint32_t*)d_sums, d_status, d_out_len, d_consumed);
            KERNEL(lzf_stream_place_kernel, dim3(P.n_segs), dim3(64), 0, st, meta.img<const SSeg>(P.i_segs), meta.img<DFrameDesc>(P.i_frames),
                   meta.img<const uint8_t*>(P.i_hptr), meta.img<uint8_t* const>(i_sout), meta.img<const uint64_t>(i_scap), sx->d_sstate,
                   (const int32_t*)d_status, (const uint64_t*)d_out_len, (const uint64_t*)d_consumed);
        }
        KERNEL(lzf_frame_deliver_kernel, dim3(P.n_frames), dim3(64), 0, st, d_frames, d_blks, (const lzf_decompress_job*)d_jobs,
               (const lzf_job_result*)d_res, (const uint32_t*)d_sums,
               meta.scr<const uint8_t*>(P.s_rsrc), meta.scr<uint8_t*>(P.s_rdst), meta.scr<uint64_t>(P.s_rlen),
               meta.scr<const uint8_t*>(P.s_lsrc), meta.scr<uint8_t*>(P.s_ldst), meta.scr<uint64_t>(P.s_llen),
               meta.scr<uint64_t>(P.s_hlen), meta.scr<uint32_t>(P.s_hcheck), d_status, d_out_len, d_consumed);
        if (P.n_blks && P.ind_max)
            RC_TRY(lzf_copy_ranges(meta.scr<const uint8_t* const>(P.s_rsrc), meta.scr<uint8_t* const>(P.s_rdst), meta.scr<const uint64_t>(P.s_rlen), P.n_blks, P.ind_max, st));
        if (P.n_link && P.link_max)
            RC_TRY(lzf_copy_ranges(meta.scr<const uint8_t* const>(P.s_lsrc), meta.scr<uint8_t* const>(P.s_ldst), meta.scr<const uint64_t>(P.s_llen), P.n_link, P.link_max, st));
        if (P.n_hash) {
            RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_hptr), meta.scr<const uint64_t>(P.s_hlen), meta.scr<uint32_t>(P.s_hout), P.n_hash, st));
            KERNEL(lzf_frame_content_check_kernel, dim3((P.n_hash + 255u) / 256u), dim3(256), 0, st, meta.scr<const uint32_t>(P.s_hout),
                   meta.img<const uint32_t>(P.i_hwant), meta.scr<const uint32_t>(P.s_hcheck), meta.img<const uint32_t>(P.i_hframe), P.n_hash, d_status);
        }
    }
    if (sx)
        KERNEL(lzf_stream_fold_kernel, dim3(sx->n_streams), dim3(64), 0, st, meta.img<const uint64_t>(i_first), (const int32_t*)d_status,
               (const uint64_t*)d_out_len, (const uint64_t*)d_consumed, meta.img<const uint64_t>(i_full),
               sx->s_status, sx->s_out_len, sx->s_consumed, sx->s_n_frames);
    // the image left host memory long ago (it was first in the stream behind the table read-back); the kernels run on
    return meta.wait();
}

// The stream scan's first launch: the frame count of every stream back on the host (one wait).  `args` keeps
// [ptrs | lens | counts | first] on the device for the second launch.
int count_streams(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, PoolAlloc& args, std::vector<uint64_t>& counts) {
    if (!args.get(32 * (size_t)n)) return LZF_E_HIP;
    std::vector<uint64_t> h(2 * (size_t)n);
    counts.resize(n);
    for (uint32_t s = 0; s < n; ++s) { h[s] = reinterpret_cast<uintptr_t>(d_in[s]); h[n + s] = in_len[s]; }
    DEV_TRY(hipMemcpyAsync(args.p, h.data(), 16 * (size_t)n, hipMemcpyHostToDevice, st));
    KERNEL(lzf_stream_scan_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, args.at<const uint8_t* const>(0), args.at<const uint64_t>(8 * (size_t)n), n,
           args.at<uint64_t>(16 * (size_t)n), (const uint64_t*)nullptr, (uint64_t*)nullptr);
    DEV_TRY(hipMemcpyAsync(counts.data(), args.at<uint64_t>(16 * (size_t)n), 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    return LZF_OK;
}

// The stream scan of n streams: the frames of every stream back on the host (two waits: the counts, then the starts).  Stream s
// is frames [first[s], first[s + 1]); frame f is f_in[f][0, f_len[f]): everything from its start to the end of its stream, as the
// reader of the frame sees it.
int scan_streams(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, std::vector<uint64_t>& first,
                 std::vector<const uint8_t*>& f_in, std::vector<size_t>& f_len) {
    PoolAlloc args(st);
    std::vector<uint64_t> counts;
    if (const int rc = count_streams(n, d_in, in_len, st, args, counts)) return rc;
    first.assign((size_t)n + 1, 0);
    for (uint32_t s = 0; s < n; ++s) first[s + 1] = first[s] + counts[s];
    const uint64_t total = first[n];
    if (total > 0x7FFFFFFFull) return LZF_E_INVALID;
    f_in.resize((size_t)total); f_len.resize((size_t)total);
    if (!total) return LZF_OK;
    std::vector<uint64_t> starts((size_t)total);
    PoolAlloc tab(st);
    if (!tab.get(8 * (size_t)total)) return LZF_E_HIP;
    DEV_TRY(hipMemcpyAsync(args.at<uint64_t>(24 * (size_t)n), first.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    KERNEL(lzf_stream_scan_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, args.at<const uint8_t* const>(0), args.at<const uint64_t>(8 * (size_t)n), n,
           args.at<uint64_t>(16 * (size_t)n), args.at<const uint64_t>(24 * (size_t)n), tab.at<uint64_t>(0));
    DEV_TRY(hipMemcpyAsync(starts.data(), tab.p, 8 * (size_t)total, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    for (uint32_t s = 0; s < n; ++s)
        for (uint64_t f = first[s]; f < first[s + 1]; ++f) {
            const uint64_t at = starts[(size_t)f] < in_len[s] ? starts[(size_t)f] : in_len[s];     // (never beyond the stream, whatever came back)
            f_in[(size_t)f] = d_in[s] + at; f_len[(size_t)f] = in_len[s] - (size_t)at;
        }
    return LZF_OK;
}

// a call whose streams are all empty: LZF_OK, 0, 0, 0 for every stream
__global__ __launch_bounds__(256) void lzf_stream_empty_kernel(uint32_t n, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    d_status[s] = LZF_OK; d_out_len[s] = 0; d_consumed[s] = 0;
    if (d_n_frames) d_n_frames[s] = 0;
}

// The frame index of a stream (lzf_frame_stream_decompressed_size_device), one wavefront per stream, 64 frames per round: stream
// s is frames [first[s], first[s + 1]) of the call, frame f starts at in[s] + in_off[f], and f_status / f_len / f_consumed hold
// what the size query found for it.  The exclusive prefix of the lengths, behind the stream's running length, is every frame's
// out_off; the first frame that ends the stream (lzf_stream_index.h's ends_stream, the fold's predicate) still gets its place
// and adds its length, every frame behind it gets the stream's length and LZF_SFRAME_BEHIND_STOP.  The running length and the
// stop carry from round to round.  Lane i writes entry i of the round, 48 bytes, if the caller's room holds it.
__global__ __launch_bounds__(64) void lzf_stream_index_kernel(const uint8_t* const* __restrict__ in, const uint64_t* __restrict__ first,
                                                              const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ f_flags,
                                                              const int32_t* __restrict__ f_status, const uint64_t* __restrict__ f_len,
                                                              const uint64_t* __restrict__ f_consumed, const uint64_t* __restrict__ f_full,
                                                              lzf_stream_frame* const* __restrict__ index, const uint64_t* __restrict__ cap,
                                                              uint64_t* __restrict__ d_n_listed) {
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    const uint64_t a = first[s], b = first[s + 1];
    lzf_stream_frame* const out = index ? index[s] : nullptr;
    const uint64_t room = out ? cap[s] : 0ull;
    const uint8_t* const src = in[s];
    uint64_t run = 0;
    bool stopped = false;
    for (uint64_t base = a; base < b; base += 64u) {
        const uint64_t f = base + lane;
        const bool act = f < b;
        const uint64_t n = act ? f_len[f] : 0ull, c = act ? f_consumed[f] : 0ull, full = act ? f_full[f] : 0ull;
        const int code = act ? f_status[f] : LZF_OK;
        const uint64_t incl = wave_incl_scan(n, lane);
        const uint64_t stops = __ballot(act && lzf_sindex::ends_stream(code, c, full));
        const uint32_t stop_at = stops ? (uint32_t)__builtin_ctzll(stops) : 64u;
        // the stream's length once a frame of this round ends it: everything up to and including that frame
        const uint64_t total = stopped ? run : run + __shfl(incl, (int)(stop_at & 63u), 64);
        if (act && f - a < room) {
            const bool behind = stopped || lane > stop_at;
            const uint32_t fl = f_flags[f];
            out[f - a] = lzf_sindex::fill_entry(src + in_off[f], (fl & kLive) != 0, fl, in_off[f], code, n, c, full,
                                                behind ? total : run + (incl - n), behind);
        }
        if (!stopped) {
            if (stops) { run = total; stopped = true; }
            else run += __shfl(incl, 63, 64);
        }
    }
    if (lane == 0 && d_n_listed) d_n_listed[s] = b - a;
}

// The size query of n frames (lzf_frame_decompressed_size_device's body, and the per-frame half of the stream size query): the
// decode call's scan (two waits), its plan with sizes_only (plan_frames, plan_pass: jobs' lengths and descriptors, no addresses),
// block checksums (they decide where delivery stops), lzf_decompressed_size_batch for the decode (linked frames in lock-step,
// lzf_chain_size_step_kernel between the steps), lzf_frame_size_deliver_kernel for the delivery.  No output slots, hence one pass
// whatever the memory budget is.  `more(sc)` puts what the caller's own kernels behind this need into the call's image before
// its one upload; the caller ends with meta.wait().  Where every header failed and `more` added nothing, nothing is uploaded:
// the scan kernel wrote the results.  `P` is the call's one pass: a caller whose kernels read the descriptors, the job results
// or the block checksums (the block index) finds them there once the call has returned; P.n_frames == 0: nothing was planned.
template <class More>
int size_frames(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len, uint64_t* d_out_len, uint64_t* d_consumed,
                int32_t* d_status, hipStream_t st, Scan& sc, Meta& meta, Pass& P, More&& more) {
    // ---- scan: summaries (wait 1), block table (wait 2)
    RC_TRY(scan_summaries(n, d_in, in_len, st, sc, d_status, d_out_len, d_consumed));
    RC_TRY(scan_table(n, st, sc));
    // ---- the decode's plan with sizes_only; the content checksum needs the content: not verified
    P.f0 = 0; P.f1 = n;
    plan_frames(P, d_in, sc);
    if (!P.jf.empty()) RC_TRY(plan_pass(P, sc, DecodeCall{true, nullptr, nullptr, dict_len, nullptr, nullptr, nullptr}, meta));
    more(sc);
    if (meta.image.empty() && !meta.scratch) return LZF_OK;
    RC_TRY(meta.upload(true));
    if (P.jf.empty()) return LZF_OK;
    lzf_decompress_job* const d_jobs = meta.img<lzf_decompress_job>(P.i_jobs);
    lzf_job_result* const d_res = meta.scr<lzf_job_result>(P.s_res);
    uint32_t* const d_sums = meta.scr<uint32_t>(P.s_sums);
    const lzf_frame_jobs::Plan& pl = P.plan;
    if (P.n_sums) RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_sptr), meta.img<const uint64_t>(P.i_slen), d_sums, P.n_sums, st));
    for (size_t k = 0; k < pl.n_steps; ++k) {
        if (pl.n_chain) KERNEL(lzf_chain_size_step_kernel, dim3(pl.n_chain), dim3(256), 0, st, meta.img<const lzf_chain_step>(P.i_steps) + k * pl.n_chain,
                               meta.scr<lzf_chain_state>(P.s_state), pl.n_chain, d_jobs, (const lzf_job_result*)d_res);
        const size_t a = pl.step_off[k], c = pl.step_off[k + 1] - a;
        if (c) RC_TRY(lzf_decompressed_size_batch(d_jobs + a, d_res + a, (uint32_t)c, lzf_frame_jobs::step_max_input(pl, k), st));
    }
    KERNEL(lzf_frame_size_deliver_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const DFrameDesc>(P.i_frames), meta.img<const DBlkDesc>(P.i_blks),
           (const lzf_decompress_job*)d_jobs, (const lzf_job_result*)d_res, (const uint32_t*)d_sums, d_status, d_out_len, d_consumed);
    return LZF_OK;
}

}  // namespace

extern "C" {

int lzf_frame_decompress_bound_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, size_t* out_bound, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !out_bound)) return LZF_E_INVALID;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Scan sc(st);
    RC_TRY(scan_summaries(n_frames, d_in, in_len, st, sc, nullptr, nullptr, nullptr));
    for (uint32_t f = 0; f < n_frames; ++f) out_bound[f] = sc.live(f) ? (size_t)sc.sum[f].out_bound : 0;
    return LZF_OK;
}

int lzf_frame_decompress_device_many(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len,
                                     uint8_t* const* d_out, const size_t* out_cap,
                                     uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_out || !out_cap || !d_out_len || !d_consumed || !d_status)) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    return decode_frames(n_frames, d_in, in_len, d_dict, dict_len, d_out, out_cap, d_out_len, d_consumed, d_status,
                         static_cast<hipStream_t>(hip_stream), nullptr);
}

// Streams of back-to-back frames: the stream scan lists the frames (two waits), the frames then go through decode_frames (the
// per-frame scan summary and the block table: two more waits) with their places found on the device.
int lzf_frame_stream_bound_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len, size_t* out_bound, void* hip_stream) {
    if (n_streams && (!d_in || !in_len || !out_bound)) return LZF_E_INVALID;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_streams == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<uint64_t> first;
    std::vector<const uint8_t*> f_in; std::vector<size_t> f_len;
    RC_TRY(scan_streams(n_streams, d_in, in_len, st, first, f_in, f_len));
    Scan sc(st);
    if (!f_in.empty()) RC_TRY(scan_summaries((uint32_t)f_in.size(), f_in.data(), f_len.data(), st, sc, nullptr, nullptr, nullptr));
    for (uint32_t s = 0; s < n_streams; ++s) {
        size_t b = 0;
        for (uint64_t f = first[s]; f < first[s + 1]; ++f) if (sc.live((uint32_t)f)) b += (size_t)sc.sum[(size_t)f].out_bound;
        out_bound[s] = b;
    }
    return LZF_OK;
}

int lzf_frame_decompress_stream_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                                       const uint8_t* d_dict, size_t dict_len,
                                       uint8_t* const* d_out, const size_t* out_cap,
                                       uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint64_t* d_n_frames,
                                       void* hip_stream) {
    if (n_streams && (!d_in || !in_len || !d_out || !out_cap || !d_out_len || !d_consumed || !d_status)) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_streams == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<uint64_t> first;
    std::vector<const uint8_t*> f_in; std::vector<size_t> f_len;
    RC_TRY(scan_streams(n_streams, d_in, in_len, st, first, f_in, f_len));
    const size_t n = f_in.size();
    if (n == 0) {
        KERNEL(lzf_stream_empty_kernel, dim3((n_streams + 255u) / 256u), dim3(256), 0, st, n_streams, d_status, d_out_len, d_consumed, d_n_frames);
        return LZF_OK;
    }
    // per frame: its stream's output and capacity (the placement kernel cuts them up), and scratch for its own results
    std::vector<uint8_t*> f_out(n); std::vector<size_t> f_cap(n);
    for (uint32_t s = 0; s < n_streams; ++s) for (uint64_t f = first[s]; f < first[s + 1]; ++f) { f_out[(size_t)f] = d_out[s]; f_cap[(size_t)f] = out_cap[s]; }
    const size_t o_len = up256(4 * n), o_cons = o_len + up256(8 * n), o_state = o_cons + up256(8 * n);
    PoolAlloc per(st);
    if (!per.get(o_state + sizeof(SState) * (size_t)n_streams)) return LZF_E_HIP;
    DEV_TRY(hipMemsetAsync(per.at<uint8_t>(o_state), 0, sizeof(SState) * (size_t)n_streams, st));
    const StreamCtx sx{n_streams, first.data(), d_out, out_cap, per.at<SState>(o_state), d_status, d_out_len, d_consumed, d_n_frames};
    return decode_frames((uint32_t)n, f_in.data(), f_len.data(), d_dict, dict_len, f_out.data(), f_cap.data(),
                         per.at<uint64_t>(o_len), per.at<uint64_t>(o_cons), per.at<int32_t>(0), st, &sx);
}

// The size query: size_frames over the caller's frames (the decode call's scan, jobs and stop rules with lengths in the place
// of bytes).
int lzf_frame_decompressed_size_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len,
                                       uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_out_len || !d_status)) return LZF_E_INVALID;
    if (n_frames == 0) return LZF_OK;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PoolAlloc own_consumed(st);                      // the kernels write `consumed` of every frame; a caller who passes NULL does not get it
    if (!d_consumed) { if (!own_consumed.get(8 * (size_t)n_frames)) return LZF_E_HIP; d_consumed = own_consumed.at<uint64_t>(0); }
    Scan sc(st);
    Meta meta(st);
    Pass P;
    RC_TRY(size_frames(n_frames, d_in, in_len, dict_len, d_out_len, d_consumed, d_status, st, sc, meta, P, [](const Scan&) {}));
    return meta.wait();                              // the image has left host memory; the kernels run on
}

int lzf_frame_stream_count_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len, size_t* n_found, void* hip_stream) {
    if (n_streams && (!d_in || !in_len || !n_found)) return LZF_E_INVALID;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_streams == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PoolAlloc args(st);
    std::vector<uint64_t> counts;
    RC_TRY(count_streams(n_streams, d_in, in_len, st, args, counts));
    for (uint32_t s = 0; s < n_streams; ++s) n_found[s] = (size_t)counts[s];
    return LZF_OK;
}

// The stream scan lists the frames (two waits); size_frames finds every frame's results, the frames behind a stop included (two
// more waits); lzf_stream_fold_kernel, the decode call's, folds them into the streams' results, and lzf_stream_index_kernel
// writes the entries.  What the two kernels read travels in size_frames' image: one upload.
int lzf_frame_stream_decompressed_size_device(uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len,
                                              lzf_stream_frame* const* d_index, const size_t* index_cap,
                                              uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status,
                                              uint64_t* d_n_frames, uint64_t* d_n_listed, void* hip_stream) {
    if (n_streams && (!d_in || !in_len || !d_out_len || !d_consumed || !d_status)) return LZF_E_INVALID;
    if ((d_index == nullptr) != (index_cap == nullptr)) return LZF_E_INVALID;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_streams == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<uint64_t> first;
    std::vector<const uint8_t*> f_in; std::vector<size_t> f_len;
    RC_TRY(scan_streams(n_streams, d_in, in_len, st, first, f_in, f_len));
    const size_t n = f_in.size();
    if (n == 0) {
        KERNEL(lzf_stream_empty_kernel, dim3((n_streams + 255u) / 256u), dim3(256), 0, st, n_streams, d_status, d_out_len, d_consumed, d_n_frames);
        if (d_n_listed) DEV_TRY(hipMemsetAsync(d_n_listed, 0, 8 * (size_t)n_streams, st));
        return LZF_OK;
    }
    const size_t o_len = up256(4 * n), o_cons = o_len + up256(8 * n);
    PoolAlloc per(st);                               // the frames' own status, length and consumed: scratch
    if (!per.get(o_cons + 8 * n)) return LZF_E_HIP;
    int32_t* const f_status = per.at<int32_t>(0);
    uint64_t* const f_out_len = per.at<uint64_t>(o_len);
    uint64_t* const f_consumed = per.at<uint64_t>(o_cons);
    Scan sc(st);
    Meta meta(st);
    size_t i_in = 0, i_first = 0, i_off = 0, i_flags = 0, i_full = 0, i_index = 0, i_cap = 0;
    const auto more = [&](const Scan& got) {            // what the fold and the index kernel read
        std::vector<uint64_t> full(n), off(n);
        std::vector<uint32_t> flags(n);
        for (uint32_t s = 0; s < n_streams; ++s)
            for (uint64_t f = first[s]; f < first[s + 1]; ++f) off[(size_t)f] = (uint64_t)(f_in[(size_t)f] - d_in[s]);
        for (uint32_t f = 0; f < n; ++f) {              // (full: decode_frames' rule for the fold)
            full[f] = got.live(f) && got.sum[f].status == LZF_OK ? got.sum[f].consumed : ~0ull;
            flags[f] = got.sum[f].flags;
        }
        i_in = meta.add(d_in, sizeof(void*) * (size_t)n_streams); i_first = meta.add(first);
        i_off = meta.add(off); i_flags = meta.add(flags); i_full = meta.add(full);
        if (d_index) {
            const std::vector<uint64_t> cap(index_cap, index_cap + n_streams);
            i_index = meta.add(d_index, sizeof(void*) * (size_t)n_streams); i_cap = meta.add(cap);
        }
    };
    Pass P;
    RC_TRY(size_frames((uint32_t)n, f_in.data(), f_len.data(), dict_len, f_out_len, f_consumed, f_status, st, sc, meta, P, more));
    KERNEL(lzf_stream_fold_kernel, dim3(n_streams), dim3(64), 0, st, meta.img<const uint64_t>(i_first), (const int32_t*)f_status,
           (const uint64_t*)f_out_len, (const uint64_t*)f_consumed, meta.img<const uint64_t>(i_full), d_status, d_out_len, d_consumed, d_n_frames);
    KERNEL(lzf_stream_index_kernel, dim3(n_streams), dim3(64), 0, st, meta.img<const uint8_t* const>(i_in), meta.img<const uint64_t>(i_first),
           meta.img<const uint64_t>(i_off), meta.img<const uint32_t>(i_flags), (const int32_t*)f_status, (const uint64_t*)f_out_len,
           (const uint64_t*)f_consumed, meta.img<const uint64_t>(i_full),
           d_index ? meta.img<lzf_stream_frame* const>(i_index) : (lzf_stream_frame* const*)nullptr,
           d_index ? meta.img<const uint64_t>(i_cap) : (const uint64_t*)nullptr, d_n_listed);
    return meta.wait();                              // the image has left host memory; the kernels run on
}

int lzf_stream_index_locate(const lzf_stream_frame* index, size_t n, uint64_t a, uint64_t b, size_t* first, size_t* count) {
    if (!first || !count || (n && !index)) return LZF_E_INVALID;
    uint64_t lo = 0, cnt = 0;
    lzf_sindex::locate(index, n, a, b, &lo, &cnt);
    *first = (size_t)lo; *count = (size_t)cnt;
    return LZF_OK;
}

// ---- the block index of a frame, and runs of its blocks
int lzf_frame_block_count_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, size_t* n_found, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !n_found)) return LZF_E_INVALID;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    Scan sc(st);
    RC_TRY(scan_summaries(n_frames, d_in, in_len, st, sc, nullptr, nullptr, nullptr));
    for (uint32_t f = 0; f < n_frames; ++f) n_found[f] = sc.live(f) ? (size_t)sc.sum[f].n_blocks : 0;
    return LZF_OK;
}

// size_frames over the caller's frames, then the delivery body in its index mode over the same descriptors, job results and block
// checksums: the entries.  What that kernel reads of the caller's travels in size_frames' image: one upload.
int lzf_frame_block_index_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len,
                                 lzf_frame_block* const* d_index, const size_t* index_cap,
                                 uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint64_t* d_n_listed, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_out_len || !d_status)) return LZF_E_INVALID;
    if ((d_index == nullptr) != (index_cap == nullptr)) return LZF_E_INVALID;
    if (d_index) for (uint32_t f = 0; f < n_frames; ++f) if (index_cap[f] && (!d_index[f] || (reinterpret_cast<uintptr_t>(d_index[f]) & 7u))) return LZF_E_INVALID;
    if (n_frames == 0) return LZF_OK;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PoolAlloc own_consumed(st);                      // (as the size query: the kernels write `consumed` of every frame)
    if (!d_consumed) { if (!own_consumed.get(8 * (size_t)n_frames)) return LZF_E_HIP; d_consumed = own_consumed.at<uint64_t>(0); }
    if (d_n_listed) DEV_TRY(hipMemsetAsync(d_n_listed, 0, 8 * (size_t)n_frames, st));       // a frame whose header fails lists nothing
    Scan sc(st);
    Meta meta(st);
    Pass P;
    size_t i_index = 0, i_cap = 0;
    const auto more = [&](const Scan&) {
        if (!d_index) return;
        const std::vector<uint64_t> cap(index_cap, index_cap + n_frames);
        i_index = meta.add(d_index, sizeof(void*) * (size_t)n_frames); i_cap = meta.add(cap);
    };
    RC_TRY(size_frames(n_frames, d_in, in_len, dict_len, d_out_len, d_consumed, d_status, st, sc, meta, P, more));
    if (P.n_frames && (d_index || d_n_listed))
        KERNEL(lzf_frame_block_index_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const DFrameDesc>(P.i_frames), meta.img<const DBlkDesc>(P.i_blks),
               meta.img<const lzf_decompress_job>(P.i_jobs), meta.scr<const lzf_job_result>(P.s_res), meta.scr<const uint32_t>(P.s_sums),
               d_index ? meta.img<lzf_frame_block* const>(i_index) : (lzf_frame_block* const*)nullptr,
               d_index ? meta.img<const uint64_t>(i_cap) : (const uint64_t*)nullptr, d_n_listed);
    return meta.wait();                              // the image has left host memory; the kernels run on
}

int lzf_block_index_locate(const lzf_frame_block* index, size_t n, uint64_t a, uint64_t b, size_t* first, size_t* count) {
    if (!first || !count || (n && !index)) return LZF_E_INVALID;
    uint64_t lo = 0, cnt = 0;
    lzf_bindex::locate(index, n, a, b, &lo, &cnt);
    *first = (size_t)lo; *count = (size_t)cnt;
    return LZF_OK;
}

// Runs of blocks, planned from the caller's entries alone: every compressed block a job at its final place, every stored block
// a copy, every checksum a hash; lzf_block_run_fold_kernel folds the results per run.  One image, one upload, no read-back.
int lzf_frame_decompress_blocks_device(uint32_t n_runs, const uint8_t* const* d_in, const size_t* in_len,
                                       const lzf_frame_block* const* runs, const size_t* count,
                                       const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (n_runs && (!d_in || !in_len || !runs || !count || !d_out || !out_cap || !d_out_len || !d_status)) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    uint64_t n_blocks = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        if (count[r] && (!runs[r] || !d_in[r])) return LZF_E_INVALID;
        if (lzf_bindex::check_run(runs[r], count[r], in_len[r]) != lzf_bindex::RUN_OK) return LZF_E_INVALID;
        n_blocks += count[r];
    }
    if (n_blocks > 0x7FFFFFFFull) return LZF_E_INVALID;
    if (n_runs == 0) return LZF_OK;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    std::vector<RRunDesc> rd(n_runs);
    std::vector<RBlkDesc> bd;
    std::vector<lzf_decompress_job> jobs;
    std::vector<const uint8_t*> sptr, csrc; std::vector<uint8_t*> cdst; std::vector<uint64_t> slen, clen;
    uint64_t max_in = 0, max_copy = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint64_t total = lzf_bindex::run_total(runs[r], count[r]);
        rd[r] = RRunDesc{(uint32_t)bd.size(), 0u, LZF_OK, r};
        if (out_cap[r] < total) { rd[r].status0 = LZF_OUT_CAPACITY; continue; }       // no block of the run is touched
        if (count[r] && !d_out[r] && total) return LZF_E_INVALID;
        rd[r].nb = (uint32_t)count[r];
        uint64_t at = 0;                                // e[k].out_off - e[0].out_off: check_run found the places contiguous
        for (size_t k = 0; k < count[r]; ++k) {
            const lzf_frame_block& e = runs[r][k];
            const uint8_t* const src = d_in[r] + e.in_off;
            RBlkDesc b{nullptr, e.out_len, kNone, kNone};
            if (e.flags & LZF_FBLOCK_HAS_SUM) { b.sum_at = src + e.in_len; b.sum_idx = (uint32_t)sptr.size(); sptr.push_back(src); slen.push_back(e.in_len); }
            if (e.flags & LZF_FBLOCK_STORED) {
                csrc.push_back(src); cdst.push_back(d_out[r] + at); clen.push_back(e.in_len);
                if (e.in_len > max_copy) max_copy = e.in_len;
            } else {
                lzf_decompress_job j;
                memset(&j, 0, sizeof j);
                j.input = src; j.input_len = e.in_len; j.prefix = d_dict; j.prefix_len = dict_len;
                j.out = d_out[r] + at; j.out_existing_len = 0; j.out_cap = e.out_len; j.output_limit = e.out_len;
                b.job = (uint32_t)jobs.size(); jobs.push_back(j);
                if (e.in_len > max_in) max_in = e.in_len;
            }
            bd.push_back(b);
            at += e.out_len;
        }
    }
    Meta meta(st);
    const size_t i_runs = meta.add(rd), i_blks = meta.add(bd), i_jobs = meta.add(jobs), i_sptr = meta.add(sptr), i_slen = meta.add(slen),
                 i_csrc = meta.add(csrc), i_cdst = meta.add(cdst), i_clen = meta.add(clen);
    const size_t s_res = meta.room(sizeof(lzf_job_result) * jobs.size()), s_sums = meta.room(4 * sptr.size());
    RC_TRY(meta.upload(true));
    lzf_job_result* const d_res = meta.scr<lzf_job_result>(s_res);
    uint32_t* const d_sums = meta.scr<uint32_t>(s_sums);
    if (!sptr.empty()) RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(i_sptr), meta.img<const uint64_t>(i_slen), d_sums, (uint32_t)sptr.size(), st));
    if (!jobs.empty()) RC_TRY(lzf_decompress_batch_sized(meta.img<const lzf_decompress_job>(i_jobs), d_res, (uint32_t)jobs.size(), max_in, st));
    if (!csrc.empty() && max_copy)
        RC_TRY(lzf_copy_ranges(meta.img<const uint8_t* const>(i_csrc), meta.img<uint8_t* const>(i_cdst), meta.img<const uint64_t>(i_clen), (uint32_t)csrc.size(), max_copy, st));
    KERNEL(lzf_block_run_fold_kernel, dim3(n_runs), dim3(64), 0, st, meta.img<const RRunDesc>(i_runs), meta.img<const RBlkDesc>(i_blks),
           (const lzf_job_result*)d_res, (const uint32_t*)d_sums, d_status, d_out_len);
    return meta.wait();                              // the image has left host memory; the kernels run on
}

}  // extern "C"

namespace {
// one pass of lzf_frame_compress_device_many: frames [f0, f1), everything in the image (i_*) and the scratch (s_*)
struct CPass {
    uint32_t f0 = 0, f1 = 0;
    uint32_t n_jobs = 0, n_copies = 0, n_linked = 0, n_hash = 0, n_frames = 0;
    size_t slots = 0, copies = 0, tables = 0;                   // bytes of the pass's part of the work allocation
    std::vector<size_t> step_off;                               // linked: jobs of step k are [step_off[k], step_off[k + 1])
    size_t i_jobs = 0, i_tabptr = 0, i_adds = 0, i_cps = 0, i_cpd = 0, i_cpl = 0, i_tps = 0, i_tpd = 0, i_tpl = 0, i_frames = 0, i_blks = 0,
           i_hptr = 0, i_hlen = 0, i_segs = 0;
    uint32_t n_segs = 0;                                        // streams: the pass's CSeg list
    size_t s_res = 0, s_rsrc = 0, s_rdst = 0, s_rlen = 0, s_at = 0, s_val = 0;
};

// What makes the frames of a compress call the pieces of streams (lzf_frame_compress_stream_device): stream q is frames
// [first[q], first[q + 1]) of the call, written back to back.  d_out / out_cap of compress_frames then hold, per frame, its
// stream's output and SIZE_MAX or 0 (the stream's capacity holds the bound, or not); d_status / d_out_len are per-frame scratch.
struct CStreamCtx {
    uint32_t n_streams;
    const uint64_t* first;              // host, n_streams + 1 entries
    int32_t* s_status; uint64_t* s_out_len;     // device, per stream
};

// lzf_frame_compress_device_many's work for n >= 1 frames on a usable device; with `cx` the frames of a stream are packed
// behind each other on the device (lzf_stream_pack_kernel in front of the assembly).
// sizes_only (lzf_frame_compressed_size_device, lzf_frame_compress_stream_size_device): the same plan without output — d_out and
// out_cap are NULL, no frame is short of capacity, no output slots are taken, the jobs have no `out` and go through
// lzf_compressed_size_batch, and behind them only the results are folded: lzf_frame_size_fold_kernel per frame, or, with `cx`,
// lzf_stream_pack_kernel per stream (its places are offsets from NULL that nobody reads).  No copy, no checksum, no patch.
int compress_frames(const lzf_settings* s, const uint32_t n, const uint8_t* const* d_in, const size_t* in_len,
                    const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap,
                    uint64_t* d_out_len, int32_t* d_status, hipStream_t st, const CStreamCtx* cx, const bool sizes_only) {
    const auto batch_call = sizes_only ? lzf_compressed_size_batch : lzf_compress_batch;
    uint8_t bd = 0;
    const int bd_rc = lzf_layout::bd_new(s->block_size, &bd);  // compress.rs:183
    const size_t bs = bd_rc == LZF_OK ? (size_t)s->block_size : 1;
    const bool indep = s->independent_blocks != 0, bsum = s->block_checksums != 0, csum = s->content_checksum != 0;
    const bool per_block_prefix = indep && dict_len > 0;       // :218,:268 in_buffer = dict ++ block, for every block
    uint8_t hdr[lzf_layout::kMaxHeader] = {0};
    const uint32_t hdr_len = bd_rc == LZF_OK ? (uint32_t)lzf_layout::write_header(s, bd, hdr) : 0u;
    // streams with a content size: every frame's header carries its own length, one header image per distinct length
    std::vector<uint8_t> hdrs; std::vector<uint32_t> hdr_idx;
    if (cx && s->has_content_size && bd_rc == LZF_OK) {
        std::map<size_t, uint32_t> seen;
        hdr_idx.resize(n);
        for (uint32_t f = 0; f < n; ++f) {
            auto it = seen.find(in_len[f]);
            if (it == seen.end()) {
                it = seen.emplace(in_len[f], (uint32_t)seen.size()).first;
                lzf_settings own = *s; own.content_size = in_len[f];
                hdrs.resize(hdrs.size() + lzf_layout::kMaxHeader, 0);
                lzf_layout::write_header(&own, bd, hdrs.data() + (size_t)it->second * lzf_layout::kMaxHeader);
            }
            hdr_idx[f] = it->second;
        }
    }
    // ---- per frame: the host driver's status up front, the blocks and the scratch they need
    std::vector<int32_t> status0(n);
    std::vector<size_t> nb(n, 0), need(n, 0);
    // the scratch copies of frame f: dict ++ block of every block (independent blocks with a dictionary), dict ++ block 0 (linked)
    auto copies_of = [&](uint32_t f) -> size_t {
        return per_block_prefix ? nb[f] * dict_len + in_len[f] : (!indep && nb[f] && dict_len) ? dict_len + (in_len[f] < bs ? in_len[f] : bs) : 0;
    };
    for (uint32_t f = 0; f < n; ++f) {
        status0[f] = bd_rc != LZF_OK ? bd_rc : !sizes_only && out_cap[f] < lzf_frame_compress_bound(s, in_len[f]) ? LZF_OUT_CAPACITY : LZF_OK;
        if (status0[f] != LZF_OK) continue;
        nb[f] = (in_len[f] + bs - 1) / bs;
        need[f] = (sizes_only ? 0 : in_len[f]) + copies_of(f) + (indep ? 0 : sizeof(lzf_u32_table)) + 256 * nb[f] + 4096;   // output slots, copies, table, lists
    }
    // ---- passes of the memory budget (frame_jobs.h's split_passes); a frame whose scratch alone is over it is a pass of its own;
    //      streams: a pass holds whole streams
    size_t budget = 0;
    RC_TRY(pass_budget(st, &budget));
    const std::vector<uint32_t> stream_of = cx ? streams_of(cx->n_streams, cx->first) : std::vector<uint32_t>();
    std::vector<uint32_t> group_end(stream_of.size());
    for (size_t f = 0; f < group_end.size(); ++f) group_end[f] = (uint32_t)cx->first[stream_of[f] + 1];
    std::vector<std::pair<uint32_t, uint32_t>> cuts;
    lzf_frame_jobs::split_passes(need.data(), n, budget, cx ? group_end.data() : nullptr, cuts);
    std::vector<CPass> passes(cuts.size());
    for (size_t p = 0; p < cuts.size(); ++p) { passes[p].f0 = cuts[p].first; passes[p].f1 = cuts[p].second; }
    // ---- work allocation (output slots | copies | linked tables), shared by the passes (stream order: pass p + 1 compresses
    //      after pass p's payload copy); the template table of a dictionary of >= 8 bytes
    size_t work_bytes = 0;
    for (CPass& P : passes) {
        for (uint32_t f = P.f0; f < P.f1; ++f) {
            if (!nb[f]) continue;
            P.n_jobs += (uint32_t)nb[f]; P.slots += sizes_only ? 0 : in_len[f]; P.copies += copies_of(f);
            if (!indep) ++P.n_linked;
        }
        P.tables = sizeof(lzf_u32_table) * (size_t)P.n_linked;
        const size_t b = up256(P.slots) + up256(P.copies) + P.tables;
        if (b > work_bytes) work_bytes = b;
    }
    PoolAlloc work(st), tmpl(st);
    if (work_bytes && !work.get(work_bytes)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
    lzf_u32_table* d_tmpl = nullptr;
    if (dict_len >= 8 && work_bytes) {                          // compress.rs:202-211, on the caller's stream
        if (!tmpl.get(sizeof(lzf_u32_table))) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
        d_tmpl = tmpl.at<lzf_u32_table>(0);
        RC_TRY(lzf_table_seed_from_dictionary(d_tmpl, d_dict, dict_len, st));
    }
    // ---- jobs, copies and descriptors of every pass into one image
    Meta meta(st);
    const size_t i_hdr = hdrs.empty() ? meta.add(hdr, sizeof hdr) : meta.add(hdrs);
    for (CPass& P : passes) {
        uint8_t* const dslots = work.at<uint8_t>(0);
        uint8_t* const dcopies = work.at<uint8_t>(up256(P.slots));
        lzf_u32_table* const dtabs = work.at<lzf_u32_table>(up256(P.slots) + up256(P.copies));
        std::vector<lzf_compress_job> jobs(P.n_jobs);
        std::vector<void*> tabptr; std::vector<uint64_t> adds;
        std::vector<const uint8_t*> cps, tps, hptr; std::vector<uint8_t*> cpd, tpd; std::vector<uint64_t> cpl, tpl, hlen;
        std::vector<CFrameDesc> fd; std::vector<CBlkDesc> bdesc(P.n_jobs);
        std::vector<CSeg> segs;
        std::vector<std::vector<uint32_t>> frame_job(P.f1 - P.f0);
        size_t slot = 0, copy = 0;
        uint32_t linked = 0;
        // the jobs: independent blocks in frame order, linked streams step after step (block k of every stream in step k)
        std::vector<std::vector<lzf_frame_jobs::CWindow>> wins(P.f1 - P.f0);
        size_t max_nb = 0;
        for (uint32_t f = P.f0; f < P.f1; ++f) if (nb[f]) { lzf_frame_jobs::compress_windows(in_len[f], bs, dict_len, indep, wins[f - P.f0]); if (nb[f] > max_nb) max_nb = nb[f]; }
        std::vector<uint32_t> lf(P.f1 - P.f0, 0);
        if (!indep) for (uint32_t f = P.f0; f < P.f1; ++f) if (nb[f]) {
            lf[f - P.f0] = linked++;
            if (d_tmpl) { tps.push_back(reinterpret_cast<const uint8_t*>(d_tmpl)); tpd.push_back(reinterpret_cast<uint8_t*>(dtabs + lf[f - P.f0])); tpl.push_back(sizeof(lzf_u32_table)); }
        }
        uint32_t jn = 0;
        auto add_job = [&](uint32_t f, size_t k) {
            const lzf_frame_jobs::CWindow& W = wins[f - P.f0][k];
            lzf_compress_job& j = jobs[jn];
            memset(&j, 0, sizeof j);
            const bool copied = per_block_prefix || (!indep && W.lo < dict_len);      // linked: block 0 behind the whole dictionary
            if (copied) {                                                             // S[lo, lo + hist + n) = dict[lo, ..) ++ data[0, ..)
                uint8_t* const c = dcopies + copy;
                const size_t from_dict = per_block_prefix ? dict_len : dict_len - W.lo;
                cps.push_back(d_dict + (per_block_prefix ? 0 : W.lo)); cpd.push_back(c); cpl.push_back(from_dict);
                cps.push_back(d_in[f] + W.off + W.n - (W.hist + W.n - from_dict)); cpd.push_back(c + from_dict); cpl.push_back(W.hist + W.n - from_dict);
                j.input = c; copy += W.hist + W.n;
            } else j.input = d_in[f] + (W.lo - (indep ? 0 : dict_len));
            j.input_len = W.hist + W.n; j.cursor = W.hist;                             // :222,:243
            j.out = sizes_only ? nullptr : dslots + slot; j.out_cap = W.n; j.table_kind = LZF_TABLE_U32;      // :242, :202
            if (indep) { if (d_tmpl) { j.table = d_tmpl; j.flags = LZF_CJOB_TABLE_READONLY; } }   // :220,:270 template.clone()
            else { j.table = dtabs + lf[f - P.f0]; tabptr.push_back(j.table); adds.push_back(W.add); }
            bdesc[jn] = CBlkDesc{d_in[f] + W.off, j.out, jn, (uint32_t)W.n};
            if (!sizes_only) slot += W.n;
            frame_job[f - P.f0].push_back(jn);
            ++jn;
        };
        if (indep) {
            for (uint32_t f = P.f0; f < P.f1; ++f) for (size_t k = 0; k < nb[f]; ++k) add_job(f, k);
            P.step_off = {0, jn};
        } else {
            for (size_t k = 0; k < max_nb; ++k) {
                P.step_off.push_back(jn);
                for (uint32_t f = P.f0; f < P.f1; ++f) if (k < nb[f]) add_job(f, k);
            }
            P.step_off.push_back(jn);
        }
        // the frames: their blocks in block order (CBlkDesc, reordered), content checksums over the caller's input
        std::vector<CBlkDesc> blks; blks.reserve(P.n_jobs);
        for (uint32_t f = P.f0; f < P.f1; ++f) {
            CFrameDesc d;
            memset(&d, 0, sizeof d);
            d.dst = sizes_only ? nullptr : d_out[f]; d.blk0 = (uint32_t)blks.size(); d.nb = (uint32_t)nb[f]; d.status0 = status0[f]; d.frame = f; d.hash_idx = kNone;
            for (uint32_t q : frame_job[f - P.f0]) blks.push_back(bdesc[q]);
            if (csum && !sizes_only && status0[f] == LZF_OK) {                 // (an empty input: no bytes to read, any valid address)
                d.hash_idx = (uint32_t)hptr.size(); hptr.push_back(in_len[f] ? d_in[f] : d_out[f]); hlen.push_back(in_len[f]);
            }
            if (cx) {                                           // (dst: lzf_stream_pack_kernel puts the frame behind the one before it)
                if (!hdr_idx.empty()) d.hdr_idx = hdr_idx[f];
                if (segs.empty() || segs.back().stream != stream_of[f]) segs.push_back(CSeg{d.dst, (uint32_t)fd.size(), 0u, stream_of[f], status0[f]});
                ++segs.back().nf;
            }
            fd.push_back(d);
        }
        P.n_segs = (uint32_t)segs.size(); P.i_segs = meta.add(segs);
        P.n_copies = (uint32_t)cps.size(); P.n_hash = (uint32_t)hptr.size(); P.n_frames = (uint32_t)fd.size();
        P.i_jobs = meta.add(jobs);
        P.i_tabptr = meta.add(tabptr); P.i_adds = meta.add(adds);
        P.i_cps = meta.add(cps); P.i_cpd = meta.add(cpd); P.i_cpl = meta.add(cpl);
        P.i_tps = meta.add(tps); P.i_tpd = meta.add(tpd); P.i_tpl = meta.add(tpl);
        P.i_frames = meta.add(fd); P.i_blks = meta.add(blks);
        P.i_hptr = meta.add(hptr); P.i_hlen = meta.add(hlen);
        const size_t n_at = sizes_only ? 0 : (bsum ? (size_t)P.n_jobs : 0) + P.n_hash;
        const size_t n_ranges = sizes_only ? 0 : (size_t)P.n_jobs;
        P.s_res = meta.room(sizeof(lzf_job_result) * (size_t)P.n_jobs);
        P.s_rsrc = meta.room(8 * n_ranges); P.s_rdst = meta.room(8 * n_ranges); P.s_rlen = meta.room(8 * n_ranges);
        P.s_at = meta.room(8 * n_at); P.s_val = meta.room(4 * n_at);
    }
    // ---- one upload, then the launches of every pass (the kernels write every scratch entry they read: no zeroing)
    RC_TRY(meta.upload(false));
    const uint32_t flags = (bsum ? kBlockSums : 0u) | (csum ? kContentSum : 0u);
    for (CPass& P : passes) {
        lzf_compress_job* const jobs = meta.img<lzf_compress_job>(P.i_jobs);
        lzf_job_result* const res = meta.scr<lzf_job_result>(P.s_res);
        const uint8_t* const* const r_src = meta.scr<const uint8_t* const>(P.s_rsrc);
        uint8_t* const* const r_dst = meta.scr<uint8_t* const>(P.s_rdst);
        const uint64_t* const r_len = meta.scr<const uint64_t>(P.s_rlen);
        if (P.n_copies)
            RC_TRY(lzf_copy_ranges(meta.img<const uint8_t* const>(P.i_cps), meta.img<uint8_t* const>(P.i_cpd), meta.img<const uint64_t>(P.i_cpl), P.n_copies,
                                   dict_len > bs ? dict_len : bs, st));
        if (P.n_linked) {                                       // :213-214 table = template.clone() (U32Table::default() without one)
            if (d_tmpl) RC_TRY(lzf_copy_ranges(meta.img<const uint8_t* const>(P.i_tps), meta.img<uint8_t* const>(P.i_tpd), meta.img<const uint64_t>(P.i_tpl),
                                               P.n_linked, sizeof(lzf_u32_table), st));
            else DEV_TRY(hipMemsetAsync(work.at<uint8_t>(up256(P.slots) + up256(P.copies)), 0, P.tables, st));
        }
        if (P.n_jobs && indep) RC_TRY(batch_call(jobs, res, P.n_jobs, LZF_KINDS_U32 | LZF_KINDS_U32_FRESH_ONLY, st));
        else if (P.n_jobs) {
            for (size_t k = 0; k + 1 < P.step_off.size(); ++k) {    // no host round trip between the steps
                const size_t a = P.step_off[k], c = P.step_off[k + 1] - a;
                if (!c) continue;
                if (k > 0) RC_TRY(lzf_table_offset_batch(meta.img<void* const>(P.i_tabptr) + a, meta.img<const uint64_t>(P.i_adds) + a, (uint32_t)c, LZF_TABLE_U32, st));
                RC_TRY(batch_call(jobs + a, res + a, (uint32_t)c, LZF_KINDS_U32, st));
            }
        }
        if (sizes_only) {                                       // the lengths from the results: nothing is assembled, copied or hashed
            if (cx)
                KERNEL(lzf_stream_pack_kernel, dim3(P.n_segs), dim3(64), 0, st, meta.img<const CSeg>(P.i_segs), meta.img<CFrameDesc>(P.i_frames),
                       meta.img<const CBlkDesc>(P.i_blks), (const lzf_job_result*)res, hdr_len, flags, cx->s_status, cx->s_out_len);
            else
                KERNEL(lzf_frame_size_fold_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const CFrameDesc>(P.i_frames), meta.img<const CBlkDesc>(P.i_blks),
                       (const lzf_job_result*)res, hdr_len, flags, d_status, d_out_len);
            continue;
        }
        const size_t n_sums = bsum ? (size_t)P.n_jobs : 0;
        uint8_t** const at = meta.scr<uint8_t*>(P.s_at);
        uint32_t* const val = meta.scr<uint32_t>(P.s_val);
        if (cx)
            KERNEL(lzf_stream_pack_kernel, dim3(P.n_segs), dim3(64), 0, st, meta.img<const CSeg>(P.i_segs), meta.img<CFrameDesc>(P.i_frames),
                   meta.img<const CBlkDesc>(P.i_blks), (const lzf_job_result*)res, hdr_len, flags, cx->s_status, cx->s_out_len);
        KERNEL(lzf_frame_assemble_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const CFrameDesc>(P.i_frames), meta.img<const CBlkDesc>(P.i_blks),
               (const lzf_job_result*)res, meta.img<const uint8_t>(i_hdr), hdr_len, flags,
               meta.scr<const uint8_t*>(P.s_rsrc), meta.scr<uint8_t*>(P.s_rdst), meta.scr<uint64_t>(P.s_rlen), at, at + n_sums, d_status, d_out_len);
        if (P.n_jobs) RC_TRY(lzf_copy_ranges(r_src, r_dst, r_len, P.n_jobs, bs, st));
        if (n_sums) RC_TRY(lzf_xxh32_batch(r_src, r_len, val, (uint32_t)n_sums, st));
        if (P.n_hash)                                           // (on the caller's stream: a forked checksum stream did not pay)
            RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_hptr), meta.img<const uint64_t>(P.i_hlen), val + n_sums, P.n_hash, st));
        const size_t n_at = n_sums + P.n_hash;
        if (n_at) KERNEL(lzf_frame_patch_kernel, dim3((uint32_t)((n_at + 255u) / 256u)), dim3(256), 0, st, (uint8_t* const*)at, (const uint32_t*)val, (uint32_t)n_at);
    }
    return meta.wait();                                         // the image has left host memory; the launches run on
}

// lzf_frame_compress_stream_device's work behind its argument checks: the pieces of every input as frames of compress_frames.
// sizes_only (lzf_frame_compress_stream_size_device): d_out / out_cap are NULL, and the frames need no status and length of their own.
int compress_streams(const lzf_settings* s, size_t frame_bytes, uint32_t n_streams, const uint8_t* const* d_in, const size_t* in_len,
                     const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap,
                     uint64_t* d_out_len, int32_t* d_status, hipStream_t st, const bool sizes_only) {
    if (s->dictionary) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_streams == 0) return LZF_OK;
    // the pieces: stream q is max(1, ceil(in_len[q] / frame_bytes)) frames of the call
    std::vector<uint64_t> first((size_t)n_streams + 1, 0);
    for (uint32_t q = 0; q < n_streams; ++q) { const uint64_t k = (in_len[q] + frame_bytes - 1) / frame_bytes; first[q + 1] = first[q] + (k ? k : 1); }
    const size_t n = (size_t)first[n_streams];
    if (n > 0x7FFFFFFFull) return LZF_E_INVALID;
    std::vector<const uint8_t*> f_in(n); std::vector<size_t> f_len(n), f_cap(n); std::vector<uint8_t*> f_out(n);
    for (uint32_t q = 0; q < n_streams; ++q) {
        const size_t cap = sizes_only || out_cap[q] >= lzf_frame_compress_stream_bound(s, frame_bytes, in_len[q]) ? SIZE_MAX : 0;
        for (uint64_t f = first[q]; f < first[q + 1]; ++f) {
            const size_t off = (size_t)(f - first[q]) * frame_bytes;
            f_in[(size_t)f] = d_in[q] + off; f_len[(size_t)f] = in_len[q] - off < frame_bytes ? in_len[q] - off : frame_bytes;
            f_out[(size_t)f] = sizes_only ? nullptr : d_out[q]; f_cap[(size_t)f] = cap;
        }
    }
    const CStreamCtx cx{n_streams, first.data(), d_status, d_out_len};
    if (sizes_only) return compress_frames(s, (uint32_t)n, f_in.data(), f_len.data(), d_dict, dict_len, nullptr, nullptr, nullptr, nullptr, st, &cx, true);
    const size_t o_len = up256(4 * n);
    PoolAlloc per(st);                                          // the frames' own status and length: scratch
    if (!per.get(o_len + 8 * n)) return LZF_E_HIP;
    return compress_frames(s, (uint32_t)n, f_in.data(), f_len.data(), d_dict, dict_len, f_out.data(), f_cap.data(),
                           per.at<uint64_t>(o_len), per.at<int32_t>(0), st, &cx, false);
}
}  // namespace

extern "C" {

int lzf_frame_compress_device_many(const lzf_settings* s, uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                   const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap,
                                   uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (!s || (n_frames && (!d_in || !in_len || !d_out || !out_cap || !d_out_len || !d_status))) return LZF_E_INVALID;
    if (s->dictionary) return LZF_E_INVALID;                    // the dictionary is d_dict: no host pointer may reach a kernel
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    return compress_frames(s, n_frames, d_in, in_len, d_dict, dict_len, d_out, out_cap, d_out_len, d_status, static_cast<hipStream_t>(hip_stream), nullptr, false);
}

int lzf_frame_compressed_size_device(const lzf_settings* s, uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len, uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (!s || (n_frames && (!d_in || !in_len || !d_out_len || !d_status))) return LZF_E_INVALID;
    if (s->dictionary) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    return compress_frames(s, n_frames, d_in, in_len, d_dict, dict_len, nullptr, nullptr, d_out_len, d_status, static_cast<hipStream_t>(hip_stream), nullptr, true);
}

size_t lzf_frame_compress_stream_bound(const lzf_settings* s, size_t frame_bytes, size_t in_len) {
    if (!s || !frame_bytes) return 0;
    const size_t whole = in_len / frame_bytes, rest = in_len % frame_bytes;
    return whole * lzf_frame_compress_bound(s, frame_bytes) + (rest || !whole ? lzf_frame_compress_bound(s, rest) : 0);
}

int lzf_frame_compress_stream_device(const lzf_settings* s, size_t frame_bytes, uint32_t n_streams,
                                     const uint8_t* const* d_in, const size_t* in_len,
                                     const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap,
                                     uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (!s || !frame_bytes || (n_streams && (!d_in || !in_len || !d_out || !out_cap || !d_out_len || !d_status))) return LZF_E_INVALID;
    return compress_streams(s, frame_bytes, n_streams, d_in, in_len, d_dict, dict_len, d_out, out_cap, d_out_len, d_status, static_cast<hipStream_t>(hip_stream), false);
}

int lzf_frame_compress_stream_size_device(const lzf_settings* s, size_t frame_bytes, uint32_t n_streams,
                                          const uint8_t* const* d_in, const size_t* in_len,
                                          const uint8_t* d_dict, size_t dict_len,
                                          uint64_t* d_out_len, int32_t* d_status, void* hip_stream) {
    if (!s || !frame_bytes || (n_streams && (!d_in || !in_len || !d_out_len || !d_status))) return LZF_E_INVALID;
    return compress_streams(s, frame_bytes, n_streams, d_in, in_len, d_dict, dict_len, nullptr, nullptr, d_out_len, d_status, static_cast<hipStream_t>(hip_stream), true);
}

}  // extern "C"
