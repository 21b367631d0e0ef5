// frame_device_append.hip — the streaming frame writer of the device frame layer (frame_device_common.h has the map):
// lzf_frame_append_device and lzf_frame_wcursor_bytes (include/lzfear_frame.h, "streaming frame writer in device memory").
//
// A write cursor per frame lives in device memory: lzf_frame_append_rules.h's Head and, behind it, the writer's window (64 KiB)
// and the stream's lzf_u32_table.  The host plans a call from in_len, flags, out_cap and the settings alone (cut_offer): it never
// reads a cursor and reads nothing back.  What depends on the cursor is settled by kernels.  Per pass of the memory budget:
//   prepare   lzf_frame_append_prepare_kernel, one wavefront per linked frame that takes blocks: block 0's history (the whole
//             dictionary in front of the first block of the frame, the cursor's window otherwise) as a copy into the scratch in
//             front of the block, block 0's job (input, length, cursor), the table.offset due before block 0 and block 1, and on a
//             cursor without a header the stream's table = template.clone()
//   compress  the whole call's stages over frame_jobs.h's plan: lzf_copy_ranges (dict ++ block, history ++ block 0),
//             lzf_compress_batch (linked streams in lock-step with lzf_table_offset_batch in front of EVERY step: step 0's is what
//             the cursor carried across the call boundary)
//   assemble  lzf_frame_append_assemble_kernel, one wavefront per frame, 64 blocks per round (lzf_frame_layout.h's rule): the
//             header only when it is not out, length words, EndMark only when finishing; the call's out_len, taken, status, phase;
//             the payload and checksum lists of the launches behind it; the frame's hash state for the update
//   then lzf_copy_ranges (payloads), lzf_xxh32_batch and the patch launch (block checksums).
// Once per call: lzf_xxh32_update_batch over the taken bytes, lzf_xxh32_digest_batch, the patch launch (content checksums of the
// frames that finish) and lzf_frame_append_commit_kernel, which alone writes the cursors' heads and windows.
//
// A DONE cursor costs the compression of its offer (the host cannot know) and writes nothing.
#include "frame_device_common.h"
#include "lzf_frame_layout.h"
#include "lzf_frame_append_rules.h"

using namespace lzf_fdev;
using lzf_append::Head;
using lzf_append::Offer;

namespace {

struct __attribute__((packed, aligned(1))) Bytes16 { uint32_t v[4]; };     // 16 bytes at any address (unaligned global access)

// per frame of the call
struct AFrame {
    uint8_t* dst;               // the caller's output
    const uint8_t* in;          // the caller's input
    Offer o;                    // the host's half of the rule
    uint64_t n_last;            // the last taken block's length
    uint32_t blk0, pad;         // the frame's blocks: CBlkDesc [blk0, blk0 + o.n_blocks) of its pass, where it takes blocks
};
static_assert(sizeof(AFrame) == 56, "append frame descriptor");
// per linked frame of a pass that takes blocks
struct APrep {
    uint8_t* block;             // where block 0 stands in the scratch; its history goes right in front of it
    uint64_t n0;                // block 0's length
    uint32_t frame, job0, job1; // job1: kNone where the call takes one block
    uint32_t copy;              // the history's entry in the pass's copy list
};
static_assert(sizeof(APrep) == 32, "append prepare descriptor");

__device__ inline Head* cursor_head(uint8_t* cursors, uint32_t f) { return reinterpret_cast<Head*>(cursors + (uint64_t)f * lzf_append::CURSOR_BYTES); }
__device__ inline uint8_t* cursor_window(uint8_t* cursors, uint32_t f) { return cursors + (uint64_t)f * lzf_append::CURSOR_BYTES + lzf_append::WINDOW_OFF; }
__device__ inline uint8_t* cursor_table(uint8_t* cursors, uint32_t f) { return cursors + (uint64_t)f * lzf_append::CURSOR_BYTES + lzf_append::TABLE_OFF; }

// What block 0 of a linked call stands behind is the cursor's to say (lzf_append::first_window).  One wavefront per frame: lane 0
// writes the job, the copy and the two offsets into the call's image; all lanes clone the template into the table of a cursor
// whose header is not out (compress.rs:213-214; without a template the zeroed cursor's table is U32Table::default()).
__global__ __launch_bounds__(64) void lzf_frame_append_prepare_kernel(const APrep* __restrict__ preps, uint8_t* __restrict__ cursors,
                                                                      const uint8_t* __restrict__ dict, uint64_t dict_len,
                                                                      const lzf_u32_table* __restrict__ tmpl,
                                                                      lzf_compress_job* __restrict__ jobs, uint64_t* __restrict__ adds,
                                                                      const uint8_t** __restrict__ cp_src, uint8_t** __restrict__ cp_dst,
                                                                      uint64_t* __restrict__ cp_len) {
    const APrep p = preps[blockIdx.x];
    const Head c = *cursor_head(cursors, p.frame);
    const lzf_append::FirstWindow w = lzf_append::first_window(c, dict_len, p.n0);
    if (threadIdx.x == 0) {
        lzf_compress_job j = jobs[p.job0];
        j.input = p.block - w.hist; j.input_len = w.hist + p.n0; j.cursor = w.hist;
        jobs[p.job0] = j;
        adds[p.job0] = w.add0;
        if (p.job1 != kNone) adds[p.job1] = w.add1;
        cp_src[p.copy] = c.header_out ? cursor_window(cursors, p.frame) : (w.hist ? dict : p.block);
        cp_dst[p.copy] = p.block - w.hist;
        cp_len[p.copy] = w.hist;
    }
    if (tmpl && c.phase != lzf_append::DONE && !c.header_out) {
        const uint64_t* const s = reinterpret_cast<const uint64_t*>(tmpl);
        uint64_t* const d = reinterpret_cast<uint64_t*>(cursor_table(cursors, p.frame));
        for (uint32_t i = threadIdx.x; i < sizeof(lzf_u32_table) / 8u; i += 64u) d[i] = s[i];
    }
}

// lzf_frame_assemble_kernel's rule for one call of a cursor: round one finds the first block status, in block order, that is
// neither LZF_OK nor LZF_OUTPUT_FULL; round two is the wave-wide exclusive scan of block_span from the header's length, or from 0
// where the header is out.  lzf_append::settle says what the call reports and whether it writes at all: a DONE cursor, a failed
// block or an offer that takes nothing leaves every range empty and every checksum place NULL.  Every word is written bytewise.
__global__ __launch_bounds__(64) void lzf_frame_append_assemble_kernel(const AFrame* __restrict__ frames, uint32_t f0, const CBlkDesc* __restrict__ blks,
                                                                       const lzf_job_result* __restrict__ res, uint8_t* __restrict__ cursors,
                                                                       const uint8_t* __restrict__ hdr, uint32_t hdr_len, uint32_t flags, uint32_t linked,
                                                                       uint64_t dict_len, uint64_t bs,
                                                                       const uint8_t** __restrict__ r_src, uint8_t** __restrict__ r_dst, uint64_t* __restrict__ r_len,
                                                                       uint8_t** __restrict__ s_at, uint8_t** __restrict__ c_at,
                                                                       lzf_xxh32_state* __restrict__ h_state, const uint8_t** __restrict__ h_ptr, uint64_t* __restrict__ h_len,
                                                                       uint64_t* __restrict__ d_out_len, uint64_t* __restrict__ d_taken,
                                                                       int32_t* __restrict__ d_status, uint32_t* __restrict__ d_phase) {
    const uint32_t f = f0 + blockIdx.x;
    const AFrame F = frames[f];
    const uint32_t lane = threadIdx.x;
    const bool bsum = (flags & kBlockSums) != 0, csum = (flags & kContentSum) != 0;
    const Head c = *cursor_head(cursors, f);
    const uint32_t nb = lzf_append::takes(F.o) ? F.o.n_blocks : 0u;
    int st = LZF_OK;
    for (uint32_t base = 0; st == LZF_OK && base < nb; base += 64u) {
        const uint32_t i = base + lane;
        lzf_layout::Block b{0u, false, false, LZF_OK};
        if (i < nb) { const CBlkDesc k = blks[F.blk0 + i]; const lzf_job_result r = res[k.job]; b = lzf_layout::block_of(r.status, r.out_len, k.raw_len); }
        const uint64_t bad = __ballot(b.bad);
        if (bad) st = __shfl(b.status, (int)__builtin_ctzll(bad), 64);
    }
    const bool ok = st == LZF_OK && c.phase != lzf_append::DONE;
    const uint64_t w0 = c.header_out ? 0u : hdr_len;
    uint64_t w = w0;
    for (uint32_t base = 0; base < nb; base += 64u) {
        const uint32_t i = base + lane;
        const bool act = i < nb;
        CBlkDesc k{nullptr, nullptr, 0u, 0u};
        lzf_layout::Block b{0u, false, false, LZF_OK};
        if (act) { k = blks[F.blk0 + i]; const lzf_job_result r = res[k.job]; b = lzf_layout::block_of(r.status, r.out_len, k.raw_len); }
        const uint64_t span = act ? lzf_layout::block_span(b.len, bsum) : 0ull;
        const uint64_t incl = wave_incl_scan(span, lane);
        if (act) {
            const uint32_t g = F.blk0 + i;
            uint8_t* const at = F.dst + (w + incl - span);      // the block's length word
            if (ok) {
                lzf_layout::wr32(at, lzf_layout::size_word(b));
                r_src[g] = b.stored ? k.raw : k.slot; r_dst[g] = at + 4; r_len[g] = b.len;
            } else { r_src[g] = k.raw; r_dst[g] = F.dst; r_len[g] = 0; }
            if (bsum) s_at[g] = ok ? at + 4 + b.len : nullptr;
        }
        w += __shfl(incl, 63, 64);
    }
    Head after = c;
    const lzf_append::Report r = lzf_append::settle(after, F.o, st, w - w0, hdr_len, (uint32_t)lzf_layout::tail_len(csum), linked != 0, dict_len, bs, F.n_last);
    const bool ends = r.writes && F.o.end == lzf_append::END_FINISH;
    if (r.header && lane < hdr_len) F.dst[lane] = hdr[lane];
    if (ends && lane < 4u) F.dst[w + lane] = 0;                 // EndMark (:277)
    if (lane != 0) return;
    d_status[f] = r.status; d_out_len[f] = r.out_len; d_taken[f] = r.taken; d_phase[f] = r.phase;
    if (!csum) return;
    c_at[f] = ends ? F.dst + w + 4 : nullptr;                   // (:279-281)
    lzf_xxh32_state h;
    if (c.header_out) h = c.hash; else lzf_append::hash_reset(h);
    h_state[f] = h; h_ptr[f] = F.in; h_len[f] = r.writes ? F.o.taken : 0ull;
}

// The end of a call, one workgroup per frame: thread 0 settles the cursor from the offer and the status the assembly reported;
// for a linked frame that goes on, all threads copy the last 64 KiB of the taken bytes into the cursor's window, 16 bytes a
// thread (the window is 16-byte aligned, the caller's input stands at any residue); thread 0 writes the head last.  A call that
// leaves the cursor untouched (rules 1, 4, 5) stores nothing.
__global__ __launch_bounds__(256) void lzf_frame_append_commit_kernel(const AFrame* __restrict__ frames, uint8_t* __restrict__ cursors,
                                                                      const lzf_xxh32_state* __restrict__ h_state, const int32_t* __restrict__ d_status,
                                                                      uint32_t hdr_len, uint32_t flags, uint32_t linked, uint64_t dict_len, uint64_t bs) {
    __shared__ Head c;
    __shared__ uint32_t moved, window;
    const uint32_t f = blockIdx.x;
    const AFrame F = frames[f];
    Head* const cur = cursor_head(cursors, f);
    if (threadIdx.x == 0) {
        c = *cur;
        const bool was_done = c.phase == lzf_append::DONE;
        const int32_t bad = lzf_append::takes(F.o) && !was_done ? d_status[f] : LZF_OK;
        const lzf_append::Report r = lzf_append::settle(c, F.o, bad, 0, hdr_len, 0, linked != 0, dict_len, bs, F.n_last);
        if (r.writes && (flags & kContentSum)) c.hash = h_state[f];
        moved = !was_done && (r.writes || r.phase == lzf_append::DONE);
        window = r.writes && linked && r.phase != lzf_append::DONE && F.o.taken >= lzf_append::WINDOW;
    }
    __syncthreads();
    if (window) {
        const uint8_t* const src = F.in + (F.o.taken - lzf_append::WINDOW);
        uint8_t* const dst = cursor_window(cursors, f);
        for (uint32_t i = threadIdx.x * 16u; i < lzf_append::WINDOW; i += 256u * 16u)
            *reinterpret_cast<Bytes16*>(dst + i) = *reinterpret_cast<const Bytes16*>(src + i);
    }
    __syncthreads();
    if (threadIdx.x == 0 && moved) *cur = c;
}

// ---- host side
// one pass: frames [f0, f1), everything in the image (i_*) and the scratch (s_*)
struct APass {
    uint32_t f0 = 0, f1 = 0;
    lzf_frame_jobs::CPlan plan;
    uint32_t n_jobs = 0, n_copies = 0, n_preps = 0;
    size_t slots = 0, copies = 0;
    size_t i_jobs = 0, i_tabptr = 0, i_adds = 0, i_cps = 0, i_cpd = 0, i_cpl = 0, i_blks = 0, i_preps = 0;
    size_t s_res = 0, s_rsrc = 0, s_rdst = 0, s_rlen = 0, s_at = 0, s_val = 0;
};

int append_frames(const lzf_settings* s, const uint32_t n, const uint8_t* const* d_in, const size_t* in_len, const uint32_t* flags_in,
                  const uint8_t* d_dict, size_t dict_len, uint8_t* cursors, uint8_t* const* d_out, const size_t* out_cap,
                  uint64_t* d_out_len, uint64_t* d_taken, int32_t* d_status, uint32_t* d_phase, hipStream_t st) {
    uint8_t bd = 0;
    const int bd_rc = lzf_layout::bd_new(s->block_size, &bd);  // compress.rs:183
    const size_t bs = bd_rc == LZF_OK ? (size_t)s->block_size : 1;
    const bool indep = s->independent_blocks != 0, bsum = s->block_checksums != 0, csum = s->content_checksum != 0;
    const bool per_block_prefix = indep && dict_len > 0;       // :218,:268 in_buffer = dict ++ block, for every block
    const size_t hist_room = dict_len > lzf_append::WINDOW ? dict_len : lzf_append::WINDOW;      // linked: in front of block 0 in the scratch
    uint8_t hdr[lzf_layout::kMaxHeader] = {0};
    const uint32_t hdr_len = bd_rc == LZF_OK ? (uint32_t)lzf_layout::write_header(s, bd, hdr) : 0u;
    // ---- per frame: what is taken (the host's half of the rule), and the scratch that follows the offer
    std::vector<AFrame> fr(n);
    std::vector<int> status0(n);
    std::vector<size_t> taken(n), need(n, 0);
    auto copies_of = [&](uint32_t f) -> size_t {
        const Offer& o = fr[f].o;
        if (!o.n_blocks) return 0;
        return per_block_prefix ? o.n_blocks * dict_len + (size_t)o.taken : !indep ? hist_room + (o.taken < bs ? (size_t)o.taken : bs) : 0;
    };
    for (uint32_t f = 0; f < n; ++f) {
        AFrame& F = fr[f];
        memset(&F, 0, sizeof F);
        F.dst = d_out[f]; F.in = d_in[f];
        F.o = lzf_append::cut_offer(bd_rc, bs, in_len[f], flags_in[f], out_cap[f]);
        const bool work = lzf_append::takes(F.o) && F.o.n_blocks;
        status0[f] = work ? LZF_OK : LZF_OUT_CAPACITY;          // (compress_plan: anything but LZF_OK takes no part)
        taken[f] = work ? (size_t)F.o.taken : 0;
        if (!work) continue;
        F.n_last = F.o.taken - (uint64_t)(F.o.n_blocks - 1u) * bs;
        need[f] = taken[f] + copies_of(f) + 256 * (size_t)F.o.n_blocks + 4096;
    }
    size_t budget = 0;
    RC_TRY(pass_budget(st, &budget));
    std::vector<std::pair<uint32_t, uint32_t>> cuts;
    lzf_frame_jobs::split_passes(need.data(), n, budget, nullptr, cuts);
    std::vector<APass> passes(cuts.size());
    size_t work_bytes = 0;
    bool any_jobs = false;
    for (size_t p = 0; p < cuts.size(); ++p) {
        APass& P = passes[p];
        P.f0 = cuts[p].first; P.f1 = cuts[p].second;
        if (!lzf_frame_jobs::compress_plan(P.f1 - P.f0, taken.data() + P.f0, status0.data() + P.f0, bs, dict_len, indep, P.plan)) return LZF_E_INVALID;
        P.n_jobs = (uint32_t)P.plan.jobs.size(); P.slots = P.plan.slots;
        for (uint32_t f = P.f0; f < P.f1; ++f) P.copies += copies_of(f);
        const size_t b = up256(P.slots) + up256(P.copies);
        if (b > work_bytes) work_bytes = b;
        any_jobs = any_jobs || P.n_jobs;
    }
    PoolAlloc work(st), tmpl(st);
    if (work_bytes && !work.get(work_bytes)) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
    lzf_u32_table* d_tmpl = nullptr;
    if (dict_len >= 8 && any_jobs) {                            // compress.rs:202-211, on the caller's stream
        if (!tmpl.get(sizeof(lzf_u32_table))) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
        d_tmpl = tmpl.at<lzf_u32_table>(0);
        RC_TRY(lzf_table_seed_from_dictionary(d_tmpl, d_dict, dict_len, st));
    }
    // ---- jobs, copies and descriptors of every pass into one image
    Meta meta(st);
    const size_t i_hdr = meta.add(hdr, sizeof hdr);
    for (APass& P : passes) {
        const lzf_frame_jobs::CPlan& pl = P.plan;
        uint8_t* const dslots = work_bytes ? work.at<uint8_t>(0) : nullptr;
        uint8_t* const dcopies = work_bytes ? work.at<uint8_t>(up256(P.slots)) : nullptr;
        std::vector<lzf_compress_job> jobs(P.n_jobs);
        std::vector<void*> tabptr(indep ? 0 : P.n_jobs); std::vector<uint64_t> adds(indep ? 0 : P.n_jobs);
        std::vector<const uint8_t*> cps; std::vector<uint8_t*> cpd; std::vector<uint64_t> cpl;
        std::vector<APrep> preps; std::vector<uint32_t> prep_of(P.f1 - P.f0, kNone);
        std::vector<CBlkDesc> blks;
        size_t copy = 0;
        for (uint32_t q = 0; q < P.n_jobs; ++q) {
            const lzf_frame_jobs::CJob& r = pl.jobs[q];
            const lzf_frame_jobs::CWindow& W = r.W;
            const uint32_t f = P.f0 + r.frame;
            const uint8_t* const data = d_in[f];
            const uint8_t* input;
            void* table;
            if (indep) {
                if (per_block_prefix) {                             // S = dict ++ this block
                    uint8_t* const sc = dcopies + copy;
                    cps.push_back(d_dict); cpd.push_back(sc); cpl.push_back(dict_len);
                    cps.push_back(data + W.off); cpd.push_back(sc + dict_len); cpl.push_back(W.n);
                    input = sc; copy += dict_len + W.n;
                } else input = data + W.lo;
                table = d_tmpl;                                     // :220,:270 template.clone()
                lzf_frame_jobs::fill_compress_job(jobs[q], r, input, dslots + r.slot, table, d_tmpl != nullptr);
                continue;
            }
            table = cursors + (size_t)f * lzf_append::CURSOR_BYTES + lzf_append::TABLE_OFF;     // the stream's own, carried by the cursor
            if (r.block == 0) {                                     // history ++ block 0: the history is the prepare kernel's to say
                uint8_t* const sc = dcopies + copy + hist_room;
                APrep pr{sc, W.n, f, q, kNone, (uint32_t)cps.size()};
                cps.push_back(data); cpd.push_back(sc); cpl.push_back(0);               // (the history: patched)
                cps.push_back(data); cpd.push_back(sc); cpl.push_back(W.n);
                prep_of[r.frame] = (uint32_t)preps.size(); preps.push_back(pr);
                copy += hist_room + W.n;
                lzf_frame_jobs::fill_compress_job(jobs[q], r, sc, dslots + r.slot, table, false);
                jobs[q].input_len = W.n; jobs[q].cursor = 0;                            // (patched with the history's length)
                adds[q] = 0;
            } else {                                                // the last 64 KiB of the caller's input in front of the block
                lzf_frame_jobs::fill_compress_job(jobs[q], r, data + (W.off - lzf_append::WINDOW), dslots + r.slot, table, false);
                jobs[q].input_len = lzf_append::WINDOW + W.n; jobs[q].cursor = lzf_append::WINDOW;
                adds[q] = bs;                                       // (block 1's: patched)
                if (r.block == 1) preps[prep_of[r.frame]].job1 = q;
            }
            tabptr[q] = table;
        }
        for (uint32_t f = P.f0; f < P.f1; ++f) {
            const uint32_t nbf = (uint32_t)pl.nb[f - P.f0];
            fr[f].blk0 = (uint32_t)blks.size();
            for (uint32_t k = 0; k < nbf; ++k) {
                const uint32_t q = (uint32_t)pl.job_of[pl.first[f - P.f0] + k];
                blks.push_back(CBlkDesc{d_in[f] + pl.jobs[q].W.off, jobs[q].out, q, (uint32_t)pl.jobs[q].W.n});
            }
        }
        P.n_copies = (uint32_t)cps.size(); P.n_preps = (uint32_t)preps.size();
        P.i_jobs = meta.add(jobs); P.i_tabptr = meta.add(tabptr); P.i_adds = meta.add(adds);
        P.i_cps = meta.add(cps); P.i_cpd = meta.add(cpd); P.i_cpl = meta.add(cpl);
        P.i_blks = meta.add(blks); P.i_preps = meta.add(preps);
        P.s_res = meta.room(sizeof(lzf_job_result) * (size_t)P.n_jobs);
        P.s_rsrc = meta.room(8 * (size_t)P.n_jobs); P.s_rdst = meta.room(8 * (size_t)P.n_jobs); P.s_rlen = meta.room(8 * (size_t)P.n_jobs);
        P.s_at = meta.room(bsum ? 8 * (size_t)P.n_jobs : 0); P.s_val = meta.room(bsum ? 4 * (size_t)P.n_jobs : 0);
    }
    const size_t i_frames = meta.add(fr);
    const size_t s_cat = meta.room(8 * (size_t)n), s_hstate = meta.room(sizeof(lzf_xxh32_state) * (size_t)n), s_hptr = meta.room(8 * (size_t)n),
                 s_hlen = meta.room(8 * (size_t)n), s_hdig = meta.room(4 * (size_t)n);
    // ---- one upload, then the launches of every pass and the call's last four (the kernels write every scratch entry they read)
    RC_TRY(meta.upload(false));
    const uint32_t flags = (bsum ? kBlockSums : 0u) | (csum ? kContentSum : 0u);
    const AFrame* const d_frames = meta.img<const AFrame>(i_frames);
    lzf_xxh32_state* const h_state = meta.scr<lzf_xxh32_state>(s_hstate);
    for (APass& P : passes) {
        lzf_compress_job* const jobs = meta.img<lzf_compress_job>(P.i_jobs);
        lzf_job_result* const res = meta.scr<lzf_job_result>(P.s_res);
        if (P.n_preps)
            KERNEL(lzf_frame_append_prepare_kernel, dim3(P.n_preps), dim3(64), 0, st, meta.img<const APrep>(P.i_preps), cursors, d_dict, (uint64_t)dict_len,
                   (const lzf_u32_table*)d_tmpl, jobs, meta.img<uint64_t>(P.i_adds), meta.img<const uint8_t*>(P.i_cps), meta.img<uint8_t*>(P.i_cpd),
                   meta.img<uint64_t>(P.i_cpl));
        if (P.n_copies)
            RC_TRY(lzf_copy_ranges(meta.img<const uint8_t* const>(P.i_cps), meta.img<uint8_t* const>(P.i_cpd), meta.img<const uint64_t>(P.i_cpl), P.n_copies,
                                   dict_len > bs ? dict_len : bs, st));
        if (P.n_jobs && indep) RC_TRY(lzf_compress_batch(jobs, res, P.n_jobs, LZF_KINDS_U32 | LZF_KINDS_U32_FRESH_ONLY, st));
        else if (P.n_jobs) {
            const std::vector<size_t>& step_off = P.plan.step_off;
            for (size_t k = 0; k + 1 < step_off.size(); ++k) {      // no host round trip between the steps
                const size_t a = step_off[k], c = step_off[k + 1] - a;
                if (!c) continue;
                RC_TRY(lzf_table_offset_batch(meta.img<void* const>(P.i_tabptr) + a, meta.img<const uint64_t>(P.i_adds) + a, (uint32_t)c, LZF_TABLE_U32, st));
                RC_TRY(lzf_compress_batch(jobs + a, res + a, (uint32_t)c, LZF_KINDS_U32, st));
            }
        }
        uint8_t** const at = meta.scr<uint8_t*>(P.s_at);
        uint32_t* const val = meta.scr<uint32_t>(P.s_val);
        KERNEL(lzf_frame_append_assemble_kernel, dim3(P.f1 - P.f0), dim3(64), 0, st, d_frames, P.f0, meta.img<const CBlkDesc>(P.i_blks), (const lzf_job_result*)res,
               cursors, meta.img<const uint8_t>(i_hdr), hdr_len, flags, indep ? 0u : 1u, (uint64_t)dict_len, (uint64_t)bs,
               meta.scr<const uint8_t*>(P.s_rsrc), meta.scr<uint8_t*>(P.s_rdst), meta.scr<uint64_t>(P.s_rlen), at, meta.scr<uint8_t*>(s_cat),
               h_state, meta.scr<const uint8_t*>(s_hptr), meta.scr<uint64_t>(s_hlen), d_out_len, d_taken, d_status, d_phase);
        if (P.n_jobs) RC_TRY(lzf_copy_ranges(meta.scr<const uint8_t* const>(P.s_rsrc), meta.scr<uint8_t* const>(P.s_rdst), meta.scr<const uint64_t>(P.s_rlen), P.n_jobs, bs, st));
        if (bsum && P.n_jobs) {
            RC_TRY(lzf_xxh32_batch(meta.scr<const uint8_t* const>(P.s_rsrc), meta.scr<const uint64_t>(P.s_rlen), val, P.n_jobs, st));
            RC_TRY(patch_words(at, val, P.n_jobs, st));
        }
    }
    if (csum) {
        RC_TRY(lzf_xxh32_update_batch(h_state, meta.scr<const uint8_t* const>(s_hptr), meta.scr<const uint64_t>(s_hlen), n, st));
        RC_TRY(lzf_xxh32_digest_batch(h_state, meta.scr<uint32_t>(s_hdig), n, st));
        RC_TRY(patch_words(meta.scr<uint8_t*>(s_cat), meta.scr<const uint32_t>(s_hdig), n, st));
    }
    KERNEL(lzf_frame_append_commit_kernel, dim3(n), dim3(256), 0, st, d_frames, cursors, (const lzf_xxh32_state*)h_state, (const int32_t*)d_status,
           hdr_len, flags, indep ? 0u : 1u, (uint64_t)dict_len, (uint64_t)bs);
    return meta.wait();                                         // the image has left host memory; the launches run on
}

}  // namespace

extern "C" {

size_t lzf_frame_wcursor_bytes(void) { return (size_t)lzf_append::CURSOR_BYTES; }

int lzf_frame_append_device(const lzf_settings* s, uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len, const uint32_t* flags,
                            const uint8_t* d_dict, size_t dict_len, void* d_cursors, uint8_t* const* d_out, const size_t* out_cap,
                            uint64_t* d_out_len, uint64_t* d_taken, int32_t* d_status, uint32_t* d_phase, void* hip_stream) {
    if (!s || (n_frames && (!d_in || !in_len || !flags || !d_cursors || !d_out || !out_cap || !d_out_len || !d_taken || !d_status || !d_phase))) return LZF_E_INVALID;
    if (s->dictionary) return LZF_E_INVALID;                    // the dictionary is d_dict: no host pointer may reach a kernel
    if (reinterpret_cast<uintptr_t>(d_cursors) & 15u) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    if (n_frames == 0) return LZF_OK;
    return append_frames(s, n_frames, d_in, in_len, flags, d_dict, dict_len, static_cast<uint8_t*>(d_cursors), d_out, out_cap,
                         d_out_len, d_taken, d_status, d_phase, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
