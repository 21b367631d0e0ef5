// frame_device_decode.hip — the decode drivers of the device frame layer (frame_device_common.h has the map).
//
// lzf_frame_decompress_device_many is lzf_frame_decompress_many's work without the host round trip of the bytes: the host sees
// only what it needs to plan.  Behind the scan (frame_device_scan.hip: two waits) decode_frames builds the decode jobs from the
// block table (frame_jobs.h, the same layout as the host driver), uploads them and enqueues, pass after pass of the memory budget:
// block checksums (lzf_xxh32_batch), decode (lzf_decompress_batch_sized / lzf_chain_decompress_step), delivery
// (lzf_frame_deliver_kernel: the reader's stop rules in stream order, decompress.rs:198-288), the copy into the caller's outputs
// (lzf_copy_ranges), content checksums (lzf_xxh32_batch + lzf_frame_content_check_kernel).  Results (status, out_len, consumed)
// are written to device arrays in stream order; scratch comes from the stream-ordered pool.  The plan is plan_frames (the scan's
// summaries and table as frame_jobs.h's frames) and plan_pass (jobs, descriptors, checksum lists).
// lzf_frame_decompress_stream_device: the stream scan lists the frames of every stream, which go through decode_frames; per
// pass, behind the decode launches, the count-only delivery finds every frame's length, lzf_stream_place_kernel gives every
// frame its place and the room left in its stream's output, and at the end lzf_stream_fold_kernel folds the frames' results into
// the streams'.
// lzf_frame_decompressed_size_device: size_frames, the same plan run once with sizes_only — lengths in the place of bytes.
#include "frame_device_common.h"
#include "lzf_chain_step.h"

using namespace lzf_fdev;

namespace {

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

// a call whose streams are all empty: LZF_OK, 0, 0, 0 for every stream
__global__ __launch_bounds__(256) void lzf_stream_empty_kernel(uint32_t n, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= n) return;
    d_status[s] = LZF_OK; d_out_len[s] = 0; d_consumed[s] = 0;
    if (d_n_frames) d_n_frames[s] = 0;
}

// ---- host side
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
        for (uint32_t f = 0; f < n; ++f) full[f] = sc.full(f);
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
        RC_TRY(enqueue_blocks(P, meta, false, st));
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
        RC_TRY(fold_streams(sx->n_streams, meta.img<const uint64_t>(i_first), d_status, d_out_len, d_consumed, meta.img<const uint64_t>(i_full),
                            sx->s_status, sx->s_out_len, sx->s_consumed, sx->s_n_frames, st));
    // the image left host memory long ago (it was first in the stream behind the table read-back); the kernels run on
    return meta.wait();
}

}  // namespace

namespace lzf_fdev __attribute__((visibility("hidden"))) {

// The block checksums and the decode steps of a planned pass, enqueued: the decode itself, or with sizes_only its twin that
// carries lengths in the place of bytes (lzf_decompressed_size_batch, and lzf_chain_size_step_kernel between the steps).
int enqueue_blocks(const Pass& P, const Meta& meta, bool sizes_only, hipStream_t st) {
    lzf_decompress_job* const d_jobs = meta.img<lzf_decompress_job>(P.i_jobs);
    lzf_job_result* const d_res = meta.scr<lzf_job_result>(P.s_res);
    const lzf_frame_jobs::Plan& pl = P.plan;
    if (P.n_sums) RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_sptr), meta.img<const uint64_t>(P.i_slen), meta.scr<uint32_t>(P.s_sums), P.n_sums, st));
    for (size_t k = 0; k < pl.n_steps; ++k) {
        const lzf_chain_step* const steps = meta.img<const lzf_chain_step>(P.i_steps) + k * pl.n_chain;
        lzf_chain_state* const state = meta.scr<lzf_chain_state>(P.s_state);
        if (pl.n_chain && sizes_only) KERNEL(lzf_chain_size_step_kernel, dim3(pl.n_chain), dim3(256), 0, st, steps, state, pl.n_chain, d_jobs, (const lzf_job_result*)d_res);
        else if (pl.n_chain) RC_TRY(lzf_chain_decompress_step_trimmed(steps, state, pl.n_chain, d_jobs, d_res, st));
        const size_t a = pl.step_off[k], c = pl.step_off[k + 1] - a;
        if (c) RC_TRY((sizes_only ? lzf_decompressed_size_batch : lzf_decompress_batch_sized)(d_jobs + a, d_res + a, (uint32_t)c, lzf_frame_jobs::step_max_input(pl, k), st));
    }
    return LZF_OK;
}

int size_frames(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len, uint64_t* d_out_len, uint64_t* d_consumed,
                int32_t* d_status, hipStream_t st, Scan& sc, Meta& meta, Pass& P, const std::function<void(const Scan&)>& more) {
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
    RC_TRY(enqueue_blocks(P, meta, true, st));
    KERNEL(lzf_frame_size_deliver_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const DFrameDesc>(P.i_frames), meta.img<const DBlkDesc>(P.i_blks),
           meta.img<const lzf_decompress_job>(P.i_jobs), meta.scr<const lzf_job_result>(P.s_res), meta.scr<const uint32_t>(P.s_sums), d_status, d_out_len, d_consumed);
    return LZF_OK;
}

int fold_streams(uint32_t n_streams, const uint64_t* first, const int32_t* f_status, const uint64_t* f_len, const uint64_t* f_consumed,
                 const uint64_t* f_full, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames, hipStream_t st) {
    KERNEL(lzf_stream_fold_kernel, dim3(n_streams), dim3(64), 0, st, first, f_status, f_len, f_consumed, f_full, d_status, d_out_len, d_consumed, d_n_frames);
    return LZF_OK;
}

int empty_streams(uint32_t n_streams, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames, hipStream_t st) {
    KERNEL(lzf_stream_empty_kernel, dim3((n_streams + 255u) / 256u), dim3(256), 0, st, n_streams, d_status, d_out_len, d_consumed, d_n_frames);
    return LZF_OK;
}

}  // namespace lzf_fdev

extern "C" {

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
    if (n == 0) return empty_streams(n_streams, d_status, d_out_len, d_consumed, d_n_frames, st);
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

}  // extern "C"
