// frame_device_resume.hip — the resumable decode of the device frame layer (frame_device_common.h has the map):
// lzf_frame_resume_device and lzf_frame_cursor_bytes (include/lzfear_frame.h, "resumable decode of frames in device memory").
//
// A cursor per frame lives in device memory: lzf_frame_resume_rules.h's Head and, behind it, two window buffers of 64 KiB.  One
// call, for every frame:
//   walk     lzf_frame_resume_walk_kernel, one lane per frame: the bounded walk (walk_piece) from the cursor's offset with the
//            room out_cap[f]; a 64-byte Piece per frame comes back (wait 1).  lzf_frame_resume_table_kernel walks the pieces again
//            and lists their blocks, 24 bytes each (wait 2).  The kernels read the cursors; the host never does.
//   plan     the pieces' blocks as frame_jobs.h's frames, in passes of the memory budget: independent blocks behind the dictionary
//            in slots, a linked piece as one stream buffer that the chain step grows, every job's prefix the cursor's window.
//   enqueue  enqueue_blocks (block checksums, chain steps, decode: the whole-frame call's), lzf_frame_resume_deliver_kernel
//            (frame_deliver_body.inc: the reader's stop rules), lzf_copy_ranges into the callers' outputs; then, once per call,
//            lzf_frame_resume_hash_kernel (the cursors' hash states and the delivered ranges into scratch), lzf_xxh32_update_batch,
//            lzf_xxh32_digest_batch and lzf_frame_resume_settle_kernel: the phase transitions (settle), the window update
//            (window_plan) and the call's results.
// The cursors are written by the last kernel alone, so a call that fails on the host leaves them as they were.
#include "frame_device_common.h"
#include "lzf_frame_resume_rules.h"

using namespace lzf_fdev;
using lzf_resume::Head;
using lzf_resume::Piece;

namespace {

// the delivery kernel's status for a frame whose piece it delivered whole: no block stopped it (no status of the ABI)
constexpr int32_t kNoStop = 0x40000000;

__device__ inline Head* cursor_head(uint8_t* cursors, uint32_t f) { return reinterpret_cast<Head*>(cursors + (uint64_t)f * lzf_resume::CURSOR_BYTES); }
__device__ inline uint8_t* cursor_window(uint8_t* cursors, uint32_t f, uint32_t sel) {
    return cursors + (uint64_t)f * lzf_resume::CURSOR_BYTES + lzf_resume::WINDOW_OFF + (uint64_t)(sel & 1u) * lzf_resume::WINDOW;
}

// args: [in | in_len | out_cap | out] of n entries each
__global__ __launch_bounds__(64) void lzf_frame_resume_walk_kernel(const uint64_t* __restrict__ args, uint32_t n, uint8_t* __restrict__ cursors,
                                                                   const uint8_t* __restrict__ dict, uint64_t dict_len, Piece* __restrict__ pieces) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= n) return;
    const Head c = *cursor_head(cursors, f);
    Piece p = lzf_resume::walk_piece(reinterpret_cast<const uint8_t*>(args[f]), args[n + f], c, args[2 * (uint64_t)n + f], [](const lzf_scan::Block&) {});
    if (c.delivered) { p.prefix = reinterpret_cast<uintptr_t>(cursor_window(cursors, f, c.win_sel)); p.prefix_len = c.win_len; }
    else { p.prefix_len = lzf_resume::dict_window(dict_len); p.prefix = reinterpret_cast<uintptr_t>(dict) + (dict_len - p.prefix_len); }
    pieces[f] = p;
}

__global__ __launch_bounds__(64) void lzf_frame_resume_table_kernel(const uint64_t* __restrict__ args, uint32_t n, uint8_t* __restrict__ cursors,
                                                                    const uint64_t* __restrict__ blk0, const uint64_t* __restrict__ cnt,
                                                                    TBlk* __restrict__ table) {
    const uint32_t f = blockIdx.x * 64u + threadIdx.x;
    if (f >= n || blk0[f] == ~0ull) return;
    const Head c = *cursor_head(cursors, f);
    TBlk* const t = table + blk0[f];
    const uint64_t room = cnt[f];       // what the first walk found: never more entries than the host allocated
    uint64_t k = 0;
    lzf_resume::walk_piece(reinterpret_cast<const uint8_t*>(args[f]), args[n + f], c, args[2 * (uint64_t)n + f], [&](const lzf_scan::Block& b) {
        if (k < room) t[k] = TBlk{b.off, b.len | (b.compressed ? 0u : lzf_scan::INCOMPRESSIBLE), b.want_sum, b.end_off};
        ++k;
    });
}

// The reader's delivery loop over the blocks of a piece (frame_deliver_body.inc), one frame per wavefront: out_len, and the
// status and consumed of the first stop in block order — kNoStop where no block stops the piece.
__global__ __launch_bounds__(64) void lzf_frame_resume_deliver_kernel(const DFrameDesc* __restrict__ frames, const DBlkDesc* __restrict__ blks,
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

// Per frame, behind the delivery: the cursor's hash state (a fresh cursor's: lzf_xxh32_reset) and the bytes the call delivered,
// for lzf_xxh32_update_batch.  A frame without a content checksum, or whose piece delivered nothing, hashes nothing.
__global__ __launch_bounds__(256) void lzf_frame_resume_hash_kernel(const uint64_t* __restrict__ args, uint32_t n, uint8_t* __restrict__ cursors,
                                                                    const Piece* __restrict__ pieces, const uint64_t* __restrict__ d_out_len,
                                                                    lzf_xxh32_state* __restrict__ h_state, const uint8_t** __restrict__ h_ptr,
                                                                    uint64_t* __restrict__ h_len) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f >= n) return;
    const Head* const c = cursor_head(cursors, f);
    const Piece p = pieces[f];
    lzf_xxh32_state s;
    if (c->parsed) s = c->hash; else lzf_resume::hash_reset(s);
    h_state[f] = s;
    h_ptr[f] = reinterpret_cast<const uint8_t*>(args[3 * (uint64_t)n + f]);
    h_len[f] = lzf_resume::delivers(p) && (p.flags & lzf_scan::FL_CSUM) ? d_out_len[f] : 0ull;
}

// The end of a call, one workgroup per frame: thread 0 settles the cursor (lzf_resume::settle) from the piece, the delivery's
// results and the digest; for a linked frame that goes on, all threads then write the new window into the cursor's other
// buffer (window_plan): the tail of the old window (the dictionary's tail in front of the first delivery) and the tail of the
// call's output.  Thread 0 writes the cursor and the call's results last.
__global__ __launch_bounds__(256) void lzf_frame_resume_settle_kernel(const uint64_t* __restrict__ args, uint32_t n, uint8_t* __restrict__ cursors,
                                                                      const Piece* __restrict__ pieces, const lzf_xxh32_state* __restrict__ h_state,
                                                                      const uint32_t* __restrict__ h_digest,
                                                                      int32_t* __restrict__ d_status, uint64_t* __restrict__ d_out_len,
                                                                      uint64_t* __restrict__ d_consumed, uint32_t* __restrict__ d_phase) {
    __shared__ Head c;
    __shared__ lzf_resume::Report rep;
    __shared__ lzf_resume::WindowPlan wp;
    const uint32_t f = blockIdx.x;
    Head* const cur = cursor_head(cursors, f);
    const Piece p = pieces[f];
    if (threadIdx.x == 0) {
        c = *cur;
        const bool had = c.delivered != 0;
        bool stopped = false;
        int32_t st = 0;
        uint64_t consumed = 0, w = 0;
        if (lzf_resume::delivers(p)) { st = d_status[f]; stopped = st != kNoStop; consumed = d_consumed[f]; w = d_out_len[f]; }
        rep = lzf_resume::settle(c, p, stopped, st, consumed, w, h_state[f], h_digest[f]);
        wp = lzf_resume::WindowPlan{0u, 0u, 0u};
        const bool linked = c.parsed && !(c.flags & lzf_scan::FL_INDEP);
        if (linked && rep.out_len && rep.phase != lzf_resume::DONE) {
            wp = lzf_resume::window_plan(p.prefix_len, rep.out_len);       // (p.prefix: the window the call's jobs decoded behind)
            c.win_sel = had ? (c.win_sel ^ 1u) & 1u : 0u;
            c.win_len = wp.new_len;
        }
    }
    __syncthreads();
    if (wp.new_len) {
        uint8_t* const dst = cursor_window(cursors, f, c.win_sel);
        const uint8_t* const old_end = reinterpret_cast<const uint8_t*>(p.prefix) + p.prefix_len;
        const uint8_t* const out_end = reinterpret_cast<const uint8_t*>(args[3 * (uint64_t)n + f]) + rep.out_len;
        for (uint32_t i = threadIdx.x; i < wp.keep; i += 256u) dst[i] = old_end[(int64_t)i - (int64_t)wp.keep];
        for (uint32_t i = threadIdx.x; i < wp.take; i += 256u) dst[wp.keep + i] = out_end[(int64_t)i - (int64_t)wp.take];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *cur = c;
        d_status[f] = rep.status; d_out_len[f] = rep.out_len; d_consumed[f] = rep.consumed; d_phase[f] = rep.phase;
    }
}

// ---- host side
// The plan of one pass: the pieces of frames [P.f0, P.f1) that deliver, as frame_jobs.h's frames (plan_frames' twin over the
// pieces' table), then jobs, chain steps, descriptors and checksum lists into the call's image (plan_pass' twin: every linked
// job decodes behind its cursor's window, no frame hashes its output from seed 0).
void plan_pieces(Pass& P, const uint8_t* const* d_in, const std::vector<Piece>& pc, const std::vector<uint64_t>& blk0, const std::vector<TBlk>& table) {
    for (uint32_t f = P.f0; f < P.f1; ++f) {
        if (!lzf_resume::delivers(pc[f])) continue;
        P.jf.emplace_back();
        lzf_frame_jobs::Frame& J = P.jf.back();
        J.linked = !(pc[f].flags & lzf_scan::FL_INDEP); J.bmax = (size_t)pc[f].block_maxsize; J.consumed = (size_t)(pc[f].stop - pc[f].start);
        for (uint64_t k = 0; k < pc[f].n_blocks; ++k) {
            const TBlk& t = table[blk0[f] + k];
            J.blocks.push_back({d_in[f] + t.off, t.len & ~lzf_scan::INCOMPRESSIBLE, (t.len & lzf_scan::INCOMPRESSIBLE) == 0});
        }
        P.jf_frame.push_back(f);
    }
    lzf_frame_jobs::layout(P.frames(), P.plan);
}

int plan_piece_pass(Pass& P, const std::vector<Piece>& pc, const std::vector<uint64_t>& blk0, const std::vector<TBlk>& table,
                    uint8_t* dslots, const uint8_t* d_dict, size_t dict_len, uint8_t* const* d_out, const size_t* out_cap, Meta& meta) {
    lzf_frame_jobs::build(P.frames(), P.plan, dslots, d_dict, dict_len, false);
    if (P.plan.jobs.size() > 0x7FFFFFFFull) return LZF_E_INVALID;
    std::vector<DFrameDesc> fd; std::vector<DBlkDesc> bd;
    std::vector<const uint8_t*> sptr; std::vector<uint64_t> slen;
    for (size_t q = 0; q < P.jf.size(); ++q) {
        const lzf_frame_jobs::Frame& J = P.jf[q];
        const uint32_t f = P.jf_frame[q];
        const Piece& S = pc[f];
        DFrameDesc d;
        memset(&d, 0, sizeof d);
        d.out_cap = out_cap[f]; d.scan_consumed = S.stop; d.bmax = J.bmax;
        d.blk0 = (uint32_t)bd.size(); d.nb = (uint32_t)J.blocks.size(); d.scan_err = kNoStop;
        d.flags = (J.linked ? kLinked : 0u);
        d.frame = f; d.hash_idx = kNone; d.link_idx = kNone;
        d.dst = d_out[f]; d.stream = J.linked ? dslots + J.out_off : nullptr;
        uint64_t bound = 0;
        for (const lzf_frame_jobs::BlockRef& b : J.blocks) bound += lzf_resume::block_bound(J.bmax, b.len, b.compressed);
        if (J.linked) {
            d.link_idx = P.n_link++;
            if (bound > P.link_max) P.link_max = bound;
            // decompress.rs:253-269: a linked block decodes behind the reader's window, here the cursor's (the dictionary's tail in front of the first delivery)
            for (size_t i = 0; i < J.blocks.size(); ++i)
                if (J.job[i] != SIZE_MAX) { P.plan.jobs[J.job[i]].prefix = reinterpret_cast<const uint8_t*>(S.prefix); P.plan.jobs[J.job[i]].prefix_len = S.prefix_len; }
        } else if (J.bmax > P.ind_max) P.ind_max = J.bmax;
        const bool bsum = (S.flags & lzf_scan::FL_BLOCKSUM) != 0;
        for (size_t i = 0; i < J.blocks.size(); ++i) {
            const TBlk& t = table[blk0[f] + i];
            DBlkDesc b;
            b.src = J.blocks[i].compressed ? (J.linked ? nullptr : dslots + J.slot[i]) : J.blocks[i].src;
            b.end_off = t.end_off; b.job = J.job[i] == SIZE_MAX ? kNone : (uint32_t)J.job[i];
            b.sum_idx = kNone; b.want_sum = t.want_sum; b.len = J.blocks[i].len;
            if (bsum) { b.sum_idx = (uint32_t)sptr.size(); sptr.push_back(J.blocks[i].src); slen.push_back(J.blocks[i].len); }
            bd.push_back(b);
        }
        fd.push_back(d);
    }
    P.n_frames = (uint32_t)fd.size(); P.n_blks = (uint32_t)bd.size(); P.n_sums = (uint32_t)sptr.size();
    P.i_jobs = meta.add(P.plan.jobs); P.i_steps = meta.add(P.plan.csteps);
    P.i_sptr = meta.add(sptr); P.i_slen = meta.add(slen);
    P.i_frames = meta.add(fd); P.i_blks = meta.add(bd);
    P.s_res = meta.room(sizeof(lzf_job_result) * P.plan.jobs.size()); P.s_state = meta.room(sizeof(lzf_chain_state) * P.plan.n_chain);
    P.s_sums = meta.room(4 * (size_t)P.n_sums);
    P.s_rsrc = meta.room(8 * (size_t)P.n_blks); P.s_rdst = meta.room(8 * (size_t)P.n_blks); P.s_rlen = meta.room(8 * (size_t)P.n_blks);
    P.s_lsrc = meta.room(8 * (size_t)P.n_link); P.s_ldst = meta.room(8 * (size_t)P.n_link); P.s_llen = meta.room(8 * (size_t)P.n_link);
    return LZF_OK;
}

int resume_frames(const uint32_t n, const uint8_t* const* d_in, const size_t* in_len, const uint8_t* d_dict, size_t dict_len, uint8_t* cursors,
                  uint8_t* const* d_out, const size_t* out_cap, uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint32_t* d_phase,
                  hipStream_t st) {
    // ---- the bounded walk: a Piece per frame (wait 1), the block table of the pieces (wait 2)
    const size_t o_pieces = up256(32 * (size_t)n), o_blk = o_pieces + up256(sizeof(Piece) * (size_t)n);
    PoolAlloc args(st);
    if (!args.get(o_blk + 16 * (size_t)n)) return LZF_E_HIP;
    std::vector<uint64_t> h(4 * (size_t)n);
    for (uint32_t f = 0; f < n; ++f) {
        h[f] = reinterpret_cast<uintptr_t>(d_in[f]); h[n + f] = in_len[f];
        h[2 * (size_t)n + f] = out_cap[f]; h[3 * (size_t)n + f] = reinterpret_cast<uintptr_t>(d_out[f]);
    }
    DEV_TRY(hipMemcpyAsync(args.p, h.data(), 32 * (size_t)n, hipMemcpyHostToDevice, st));
    const uint64_t* const d_args = args.at<const uint64_t>(0);
    Piece* const d_pieces = args.at<Piece>(o_pieces);
    KERNEL(lzf_frame_resume_walk_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, d_args, n, cursors, d_dict, (uint64_t)dict_len, d_pieces);
    std::vector<Piece> pc(n);
    DEV_TRY(hipMemcpyAsync(pc.data(), d_pieces, sizeof(Piece) * (size_t)n, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> blk0(n, ~0ull), cnt(n, 0);
    uint64_t n_table = 0;
    for (uint32_t f = 0; f < n; ++f) if (lzf_resume::delivers(pc[f])) { blk0[f] = n_table; cnt[f] = pc[f].n_blocks; n_table += pc[f].n_blocks; }
    if (n_table > 0x7FFFFFFFull) return LZF_E_INVALID;
    std::vector<TBlk> table((size_t)n_table);
    if (n_table) {
        std::vector<uint64_t> hb(2 * (size_t)n);
        memcpy(hb.data(), blk0.data(), 8 * (size_t)n); memcpy(hb.data() + n, cnt.data(), 8 * (size_t)n);
        DEV_TRY(hipMemcpyAsync(args.at<uint64_t>(o_blk), hb.data(), 16 * (size_t)n, hipMemcpyHostToDevice, st));
        PoolAlloc tab(st);
        if (!tab.get(sizeof(TBlk) * (size_t)n_table)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
        KERNEL(lzf_frame_resume_table_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, d_args, n, cursors, args.at<const uint64_t>(o_blk),
               args.at<const uint64_t>(o_blk + 8 * (size_t)n), tab.at<TBlk>(0));
        DEV_TRY(hipMemcpyAsync(table.data(), tab.p, sizeof(TBlk) * (size_t)n_table, hipMemcpyDeviceToHost, st));
        DEV_TRY(hipStreamSynchronize(st));
    }
    // ---- passes of the memory budget with the whole-frame call's accounting, counted over the piece; a piece that is over the
    //      budget alone is a pass of its own (its scratch follows out_cap, which the caller chose)
    std::vector<size_t> need(n, 0);
    for (uint32_t f = 0; f < n; ++f) {
        if (!lzf_resume::delivers(pc[f])) continue;
        size_t sum = 0;
        for (uint64_t k = 0; k < pc[f].n_blocks; ++k) {
            const TBlk& t = table[blk0[f] + k];
            const uint32_t len = t.len & ~lzf_scan::INCOMPRESSIBLE;
            sum += (size_t)len + 256u + ((t.len & lzf_scan::INCOMPRESSIBLE) ? 0u : (size_t)lzf_scan::block_out_bound(pc[f].block_maxsize, len));
        }
        need[f] = (size_t)(pc[f].stop - pc[f].start) + 2 * sum + 4096;
    }
    size_t budget = 0;
    RC_TRY(pass_budget(st, &budget));
    std::vector<std::pair<uint32_t, uint32_t>> cuts;
    lzf_frame_jobs::split_passes(need.data(), n, budget, nullptr, cuts);
    std::vector<Pass> passes(cuts.size());
    size_t slots_bytes = 0;
    for (size_t p = 0; p < cuts.size(); ++p) {
        Pass& P = passes[p];
        P.f0 = cuts[p].first; P.f1 = cuts[p].second;
        plan_pieces(P, d_in, pc, blk0, table);
        if (P.plan.out_total > slots_bytes) slots_bytes = P.plan.out_total;
    }
    PoolAlloc slots(st);                // one allocation for all passes (stream order: pass p + 1 decodes after pass p's copy)
    if (slots_bytes && !slots.get(slots_bytes)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
    Meta meta(st);
    for (Pass& P : passes) if (!P.jf.empty()) RC_TRY(plan_piece_pass(P, pc, blk0, table, slots.at<uint8_t>(0), d_dict, dict_len, d_out, out_cap, meta));
    const size_t s_hstate = meta.room(sizeof(lzf_xxh32_state) * (size_t)n), s_hptr = meta.room(8 * (size_t)n), s_hlen = meta.room(8 * (size_t)n),
                 s_hdig = meta.room(4 * (size_t)n);
    // ---- one upload, then the kernels of every pass and the call's last four
    RC_TRY(meta.upload(true));
    for (Pass& P : passes) {
        if (!P.n_frames) continue;
        RC_TRY(enqueue_blocks(P, meta, false, st));
        KERNEL(lzf_frame_resume_deliver_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const DFrameDesc>(P.i_frames), meta.img<const DBlkDesc>(P.i_blks),
               meta.img<const lzf_decompress_job>(P.i_jobs), meta.scr<const lzf_job_result>(P.s_res), meta.scr<const uint32_t>(P.s_sums),
               meta.scr<const uint8_t*>(P.s_rsrc), meta.scr<uint8_t*>(P.s_rdst), meta.scr<uint64_t>(P.s_rlen),
               meta.scr<const uint8_t*>(P.s_lsrc), meta.scr<uint8_t*>(P.s_ldst), meta.scr<uint64_t>(P.s_llen),
               (uint64_t*)nullptr, (uint32_t*)nullptr, d_status, d_out_len, d_consumed);
        if (P.n_blks && P.ind_max)
            RC_TRY(lzf_copy_ranges(meta.scr<const uint8_t* const>(P.s_rsrc), meta.scr<uint8_t* const>(P.s_rdst), meta.scr<const uint64_t>(P.s_rlen), P.n_blks, P.ind_max, st));
        if (P.n_link && P.link_max)
            RC_TRY(lzf_copy_ranges(meta.scr<const uint8_t* const>(P.s_lsrc), meta.scr<uint8_t* const>(P.s_ldst), meta.scr<const uint64_t>(P.s_llen), P.n_link, P.link_max, st));
    }
    lzf_xxh32_state* const h_state = meta.scr<lzf_xxh32_state>(s_hstate);
    KERNEL(lzf_frame_resume_hash_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, d_args, n, cursors, (const Piece*)d_pieces, (const uint64_t*)d_out_len,
           h_state, meta.scr<const uint8_t*>(s_hptr), meta.scr<uint64_t>(s_hlen));
    RC_TRY(lzf_xxh32_update_batch(h_state, meta.scr<const uint8_t* const>(s_hptr), meta.scr<const uint64_t>(s_hlen), n, st));
    RC_TRY(lzf_xxh32_digest_batch(h_state, meta.scr<uint32_t>(s_hdig), n, st));
    KERNEL(lzf_frame_resume_settle_kernel, dim3(n), dim3(256), 0, st, d_args, n, cursors, (const Piece*)d_pieces, (const lzf_xxh32_state*)h_state,
           meta.scr<const uint32_t>(s_hdig), d_status, d_out_len, d_consumed, d_phase);
    // the image left host memory long ago (it was first in the stream behind the table read-back); the kernels run on
    return meta.wait();
}

}  // namespace

extern "C" {

size_t lzf_frame_cursor_bytes(void) { return (size_t)lzf_resume::CURSOR_BYTES; }

int lzf_frame_resume_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                            const uint8_t* d_dict, size_t dict_len, void* d_cursors,
                            uint8_t* const* d_out, const size_t* out_cap,
                            uint64_t* d_out_len, uint64_t* d_consumed, int32_t* d_status, uint32_t* d_phase, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_cursors || !d_out || !out_cap || !d_out_len || !d_consumed || !d_status || !d_phase)) return LZF_E_INVALID;
    if (reinterpret_cast<uintptr_t>(d_cursors) & 15u) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    return resume_frames(n_frames, d_in, in_len, d_dict, dict_len, static_cast<uint8_t*>(d_cursors), d_out, out_cap, d_out_len, d_consumed,
                         d_status, d_phase, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
