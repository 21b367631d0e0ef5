// frame_device_compress.hip — the compress drivers of the device frame layer (frame_device_common.h has the map).
//
// lzf_frame_compress_device_many is lzf_frame_compress_many's work on inputs in device memory.  The host plans the whole call
// from in_len[] and the settings (frame_jobs.h's compress_plan, the same as the host driver's) and reads nothing back; per pass
// of the memory budget it enqueues: the dict ++ block copies (lzf_copy_ranges), the tables (lzf_table_seed_from_dictionary once,
// copied into every linked stream's table), the compression (lzf_compress_batch; linked streams in lock-step with
// lzf_table_offset_batch between the steps), assembly (lzf_frame_assemble_kernel: header, length words, EndMark, status and
// out_len, and the lists of the steps behind it, by lzf_frame_layout.h's rule), the payload copy (lzf_copy_ranges), block and
// content checksums (lzf_xxh32_batch) and the checksum words (lzf_frame_patch_kernel).
// lzf_frame_compress_stream_device: the pieces of every input are frames of that call (compress_streams); lzf_stream_pack_kernel,
// in front of the assembly, puts each frame behind the one before.
// lzf_frame_compressed_size_device / lzf_frame_compress_stream_size_device: the same plan with `sizes_only` — no output slots, jobs
// without `out` through lzf_compressed_size_batch, then lzf_frame_size_fold_kernel (per frame) or lzf_stream_pack_kernel (per
// stream) over the job results alone: the (status, out_len) of the compress calls, nothing written, no checksum computed.
#include <map>
#include "frame_device_common.h"
#include "lzf_frame_layout.h"

using namespace lzf_fdev;

namespace {

// ---- compress: per frame and per block of a pass, for the assembly kernel
struct CFrameDesc {
    uint8_t* dst;               // the caller's output
    uint32_t blk0, nb;          // the frame's blocks: CBlkDesc [blk0, blk0 + nb) of the pass, in block order
    int32_t status0;            // what the host decided: LZF_OK, LZF_OUT_CAPACITY or the block size's error (then nb = 0)
    uint32_t frame, hash_idx;   // hash_idx: the frame's content checksum in the pass, kNone: none
    uint32_t hdr_idx;           // the frame's header image (streams with a content size: one per piece length), 0: the call's one
};
static_assert(sizeof(CFrameDesc) == 32, "compress frame descriptor");

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

// one pass of lzf_frame_compress_device_many: frames [f0, f1), everything in the image (i_*) and the scratch (s_*)
struct CPass {
    uint32_t f0 = 0, f1 = 0;
    lzf_frame_jobs::CPlan plan;                                 // the pass's jobs, frames counted from f0
    uint32_t n_jobs = 0, n_copies = 0, n_linked = 0, n_hash = 0, n_frames = 0;
    size_t slots = 0, copies = 0, tables = 0;                   // bytes of the pass's part of the work allocation
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

// What a compress call fixes for all of its passes.  sizes_only: d_out is NULL and no job has an `out`.
struct CCall {
    const uint8_t* const* d_in; const size_t* in_len; const uint8_t* d_dict; size_t dict_len; uint8_t* const* d_out;
    bool indep, bsum, csum, sizes_only;
    const int32_t* status0;             // per frame, what the host decided up front
    uint8_t* work;                      // the work allocation: [output slots | copies | linked tables] of a pass
    lzf_u32_table* d_tmpl;              // the template table of a dictionary of >= 8 bytes, or NULL
    const uint32_t* stream_of; const uint32_t* hdr_idx;         // streams: the stream of every frame, and its header image if each has its own
};

// The plan of one pass: the jobs from frame_jobs.h's records (where S[lo, ..) stands: the caller's input, or a scratch copy of
// dict ++ block), the copy lists, the descriptors of the assembly kernels and the checksum lists, into the call's image; room for
// what the kernels write, in its scratch.
void plan_cpass(CPass& P, const CCall& c, Meta& meta) {
    const lzf_frame_jobs::CPlan& pl = P.plan;
    const bool per_block_prefix = c.indep && c.dict_len > 0;   // :218,:268 in_buffer = dict ++ block, for every block
    uint8_t* const dslots = c.work;
    uint8_t* const dcopies = c.work + up256(P.slots);
    lzf_u32_table* const dtabs = reinterpret_cast<lzf_u32_table*>(c.work + up256(P.slots) + up256(P.copies));
    std::vector<lzf_compress_job> jobs(P.n_jobs);
    std::vector<void*> tabptr; std::vector<uint64_t> adds;
    std::vector<const uint8_t*> cps, tps, hptr; std::vector<uint8_t*> cpd, tpd; std::vector<uint64_t> cpl, tpl, hlen;
    std::vector<CFrameDesc> fd; std::vector<CBlkDesc> blks;
    std::vector<CSeg> segs;
    if (c.d_tmpl) for (uint32_t i = 0; i < pl.n_linked; ++i) {  // :213-214 table = template.clone()
        tps.push_back(reinterpret_cast<const uint8_t*>(c.d_tmpl)); tpd.push_back(reinterpret_cast<uint8_t*>(dtabs + i)); tpl.push_back(sizeof(lzf_u32_table));
    }
    size_t copy = 0;
    for (uint32_t q = 0; q < P.n_jobs; ++q) {
        const lzf_frame_jobs::CJob& r = pl.jobs[q];
        const lzf_frame_jobs::CWindow& W = r.W;
        const uint8_t* const data = c.d_in[P.f0 + r.frame];
        const uint8_t* input;
        if (per_block_prefix || (!c.indep && W.lo < c.dict_len)) {                    // linked: block 0 behind the whole dictionary
            uint8_t* const s = dcopies + copy;                                        // S[lo, lo + hist + n) = dict[lo, ..) ++ data[0, ..)
            const size_t from_dict = per_block_prefix ? c.dict_len : c.dict_len - W.lo;
            cps.push_back(c.d_dict + (per_block_prefix ? 0 : W.lo)); cpd.push_back(s); cpl.push_back(from_dict);
            cps.push_back(data + W.off + W.n - (W.hist + W.n - from_dict)); cpd.push_back(s + from_dict); cpl.push_back(W.hist + W.n - from_dict);
            input = s; copy += W.hist + W.n;
        } else input = data + (W.lo - (c.indep ? 0 : c.dict_len));
        void* const table = c.indep ? static_cast<void*>(c.d_tmpl) : dtabs + r.table;     // :220,:270 template.clone(), or the stream's own
        lzf_frame_jobs::fill_compress_job(jobs[q], r, input, c.sizes_only ? nullptr : dslots + r.slot, table, c.indep && c.d_tmpl);
        if (!c.indep) { tabptr.push_back(table); adds.push_back(W.add); }
    }
    // the frames: their blocks in block order, content checksums over the caller's input
    blks.reserve(P.n_jobs);
    for (uint32_t f = P.f0; f < P.f1; ++f) {
        const uint32_t nb = (uint32_t)pl.nb[f - P.f0];
        CFrameDesc d;
        memset(&d, 0, sizeof d);
        d.dst = c.sizes_only ? nullptr : c.d_out[f]; d.blk0 = (uint32_t)blks.size(); d.nb = nb; d.status0 = c.status0[f]; d.frame = f; d.hash_idx = kNone;
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t q = (uint32_t)pl.job_of[pl.first[f - P.f0] + k];
            blks.push_back(CBlkDesc{c.d_in[f] + pl.jobs[q].W.off, jobs[q].out, q, (uint32_t)pl.jobs[q].W.n});
        }
        if (c.csum && !c.sizes_only && c.status0[f] == LZF_OK) {               // (an empty input: no bytes to read, any valid address)
            d.hash_idx = (uint32_t)hptr.size(); hptr.push_back(c.in_len[f] ? c.d_in[f] : c.d_out[f]); hlen.push_back(c.in_len[f]);
        }
        if (c.stream_of) {                                      // (dst: lzf_stream_pack_kernel puts the frame behind the one before it)
            if (c.hdr_idx) d.hdr_idx = c.hdr_idx[f];
            if (segs.empty() || segs.back().stream != c.stream_of[f]) segs.push_back(CSeg{d.dst, (uint32_t)fd.size(), 0u, c.stream_of[f], c.status0[f]});
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
    const size_t n_at = c.sizes_only ? 0 : (c.bsum ? (size_t)P.n_jobs : 0) + P.n_hash;
    const size_t n_ranges = c.sizes_only ? 0 : (size_t)P.n_jobs;
    P.s_res = meta.room(sizeof(lzf_job_result) * (size_t)P.n_jobs);
    P.s_rsrc = meta.room(8 * n_ranges); P.s_rdst = meta.room(8 * n_ranges); P.s_rlen = meta.room(8 * n_ranges);
    P.s_at = meta.room(8 * n_at); P.s_val = meta.room(4 * n_at);
}

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
        if (!lzf_frame_jobs::compress_plan(P.f1 - P.f0, in_len + P.f0, status0.data() + P.f0, bs, dict_len, indep, P.plan)) return LZF_E_INVALID;
        P.n_jobs = (uint32_t)P.plan.jobs.size(); P.n_linked = P.plan.n_linked; P.slots = sizes_only ? 0 : P.plan.slots;
        for (uint32_t f = P.f0; f < P.f1; ++f) if (nb[f]) P.copies += copies_of(f);
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
    const CCall call{d_in, in_len, d_dict, dict_len, d_out, indep, bsum, csum, sizes_only, status0.data(), work.at<uint8_t>(0), d_tmpl,
                     cx ? stream_of.data() : nullptr, hdr_idx.empty() ? nullptr : hdr_idx.data()};
    for (CPass& P : passes) plan_cpass(P, call, meta);
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
            const std::vector<size_t>& step_off = P.plan.step_off;
            for (size_t k = 0; k + 1 < step_off.size(); ++k) {      // no host round trip between the steps
                const size_t a = step_off[k], c = step_off[k + 1] - a;
                if (!c) continue;
                if (k > 0) RC_TRY(lzf_table_offset_batch(meta.img<void* const>(P.i_tabptr) + a, meta.img<const uint64_t>(P.i_adds) + a, (uint32_t)c, LZF_TABLE_U32, st));
                RC_TRY(batch_call(jobs + a, res + a, (uint32_t)c, LZF_KINDS_U32, st));
            }
        }
        if (cx)                                                 // every frame's place in its stream; sizes_only: the streams' lengths are all there is
            KERNEL(lzf_stream_pack_kernel, dim3(P.n_segs), dim3(64), 0, st, meta.img<const CSeg>(P.i_segs), meta.img<CFrameDesc>(P.i_frames),
                   meta.img<const CBlkDesc>(P.i_blks), (const lzf_job_result*)res, hdr_len, flags, cx->s_status, cx->s_out_len);
        if (sizes_only) {                                       // the lengths from the results: nothing is assembled, copied or hashed
            if (!cx)
                KERNEL(lzf_frame_size_fold_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const CFrameDesc>(P.i_frames), meta.img<const CBlkDesc>(P.i_blks),
                       (const lzf_job_result*)res, hdr_len, flags, d_status, d_out_len);
            continue;
        }
        const size_t n_sums = bsum ? (size_t)P.n_jobs : 0;
        uint8_t** const at = meta.scr<uint8_t*>(P.s_at);
        uint32_t* const val = meta.scr<uint32_t>(P.s_val);
        KERNEL(lzf_frame_assemble_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const CFrameDesc>(P.i_frames), meta.img<const CBlkDesc>(P.i_blks),
               (const lzf_job_result*)res, meta.img<const uint8_t>(i_hdr), hdr_len, flags,
               meta.scr<const uint8_t*>(P.s_rsrc), meta.scr<uint8_t*>(P.s_rdst), meta.scr<uint64_t>(P.s_rlen), at, at + n_sums, d_status, d_out_len);
        if (P.n_jobs) RC_TRY(lzf_copy_ranges(r_src, r_dst, r_len, P.n_jobs, bs, st));
        if (n_sums) RC_TRY(lzf_xxh32_batch(r_src, r_len, val, (uint32_t)n_sums, st));
        if (P.n_hash)                                           // (on the caller's stream: a forked checksum stream did not pay)
            RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(P.i_hptr), meta.img<const uint64_t>(P.i_hlen), val + n_sums, P.n_hash, st));
        const size_t n_at = n_sums + P.n_hash;
        RC_TRY(patch_words(at, val, n_at, st));
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

namespace lzf_fdev {
int patch_words(uint8_t* const* d_at, const uint32_t* d_val, size_t n, hipStream_t st) {
    if (n) KERNEL(lzf_frame_patch_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, st, d_at, d_val, (uint32_t)n);
    return LZF_OK;
}
}  // namespace lzf_fdev

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
