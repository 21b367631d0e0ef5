// frame_device_verify.hip — lzf_frame_verify_device: does every frame deliver exactly the expected bytes?  No output memory, no
// decode (frame_device_common.h has the map).
//
// The size query's own work first (size_frames: scan, block checksums, lzf_decompressed_size_batch, the stop rules), with the
// frame's out_len written straight to d_at; then the delivery body in its index mode (index_blocks) into scratch entries, which
// say where every delivered block's output lies.  With those, no block depends on another: block k's history is simply the
// expected bytes in front of it.  lzf_verify_jobs_kernel, one thread per block, turns an entry into
//   a verify job     a compressed independent block: out = expected + out_off, no existing output, out_cap = out_len;
//                    a compressed linked block: out = expected, existing = out_off, out_cap = out_off + out_len, trimmed past 1 GiB
//                    as lzf_history_trim.h does it; the dictionary is the prefix of both;
//   a stored range   the payload against expected + out_off, for lzf_first_diff_kernel, one wavefront per range,
// either one cut where the expected bytes end.  ALL jobs of all frames, linked ones included, go to lzf_decompress_verify_batch in
// one call; lzf_xxh32_batch hashes the expected bytes of the frames that carry a content checksum; lzf_frame_verify_fold_kernel,
// one wavefront per frame, takes the first failing block in block order.  No output slots, no passes of the memory budget, no
// chain step behind the size query's own.
#include "frame_device_common.h"
#include "lzf_device.h"
#include "lzf_history_trim.h"

namespace {

// per frame of the call, for the two kernels below
struct VFrame {
    const uint8_t* in; const uint8_t* expected;
    uint64_t expected_len, blk0, nb;    // the frame's entries: [blk0, blk0 + nb) of the call's
    uint64_t scan_consumed;             // what the walk consumed: the reader reached the EndMark iff the size query consumed as much
    uint32_t want_content, check;       // check: EndMark read, content checksum present, walk without error
};
constexpr uint64_t kNoDiff = ~0ull;

// One thread per block of the call: the entry into a verify job (input_len 0 and nothing to compare where the block is stored or
// not delivered), a stored range (length 0 where it is compressed or not delivered) and the shift of a trimmed linked job.
__global__ __launch_bounds__(256) void lzf_verify_jobs_kernel(const VFrame* __restrict__ frames, const uint32_t* __restrict__ blk_frame,
                                                              const lzf_frame_block* __restrict__ ent, uint64_t n_blks,
                                                              const uint8_t* dict, uint64_t dict_len, lzf_decompress_job* __restrict__ jobs,
                                                              uint64_t* __restrict__ shift, const uint8_t** __restrict__ r_a,
                                                              const uint8_t** __restrict__ r_b, uint64_t* __restrict__ r_len) {
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= n_blks) return;
    const VFrame F = frames[blk_frame[b]];
    const lzf_frame_block e = ent[b];
    lzf_decompress_job j{};
    uint64_t s = 0, rl = 0;
    const uint8_t *ra = nullptr, *rb = nullptr;
    if (e.flags & LZF_FBLOCK_DELIVERED) {
        // what of the block's output the expected bytes cover (out_off <= the frame's out_len)
        const uint64_t end = e.out_off + e.out_len < F.expected_len ? e.out_off + e.out_len : F.expected_len;
        if (e.flags & LZF_FBLOCK_STORED) {
            ra = F.in + e.in_off; rb = F.expected + e.out_off; rl = end > e.out_off ? end - e.out_off : 0ull;
        } else {
            j.input = F.in + e.in_off; j.input_len = e.in_len; j.prefix = dict; j.prefix_len = dict_len;
            if (e.flags & LZF_FBLOCK_LINKED) {
                j.out = const_cast<uint8_t*>(F.expected); j.out_existing_len = e.out_off; j.out_cap = end > e.out_off ? end : e.out_off;
                j.output_limit = e.out_off + e.block_maxsize;
                j = lzf_trim::trim(j, &s);
            } else {
                j.out = const_cast<uint8_t*>(F.expected) + e.out_off; j.out_cap = end > e.out_off ? end - e.out_off : 0ull;
                j.output_limit = e.block_maxsize;
            }
        }
    }
    jobs[b] = j; shift[b] = s; r_a[b] = ra; r_b[b] = rb; r_len[b] = rl;
}

// One wavefront per range: first[r] = the first i < len[r] with a[r][i] != b[r][i], or kNoDiff.  16 bytes a lane and 1 KiB a step
// where 16 bytes remain, the tail bytewise: nothing outside the ranges is read.
__global__ __launch_bounds__(64) void lzf_first_diff_kernel(const uint8_t* const* __restrict__ a_, const uint8_t* const* __restrict__ b_,
                                                            const uint64_t* __restrict__ len, uint64_t* __restrict__ first) {
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const uint64_t n = len[r];
    lzf::cgu8* a = lzf::as_global(a_[r]);
    lzf::cgu8* b = lzf::as_global(b_[r]);
    uint64_t found = kNoDiff;
    for (uint64_t base = 0; base < n && found == kNoDiff; base += 1024u) {
        const uint64_t i = base + lane * 16u;
        uint32_t d = 16u;
        if (n - base >= 16u * (lane + 1u)) {
            const lzf::u32x4 x = lzf::ld16(a + i) ^ lzf::ld16(b + i);
            for (int k = 3; k >= 0; --k) if (x[k]) d = 4u * (uint32_t)k + ((uint32_t)__builtin_ctz(x[k]) >> 3);
        } else if (i < n) {
            for (uint32_t t = (uint32_t)(n - i); t-- > 0u;) if (a[i + t] != b[i + t]) d = t;
        }
        const unsigned long long bal = __ballot(d < 16u);
        if (bal) { const uint32_t l = lzf::first_lane(bal); found = base + l * 16u + (uint32_t)__shfl((int)d, (int)l, 64); }
    }
    if (lane == 0) first[r] = found;
}

// One wavefront per frame, 64 blocks per round.  A frame the size query did not answer LZF_OK keeps that status, with the size
// query's out_len in d_at.  Otherwise the first delivered block, in block order, whose bytes differ fixes LZF_MISMATCH and the
// position: the verify job's (absolute in a linked frame once the trim's shift is added, behind out_off in an independent one), or
// the stored range's; then the lengths; then XXH32 of the expected bytes against the frame's content checksum.
__global__ __launch_bounds__(64) void lzf_frame_verify_fold_kernel(const VFrame* __restrict__ frames, const lzf_frame_block* __restrict__ ent,
                                                                   const lzf_job_result* __restrict__ res, const uint64_t* __restrict__ shift,
                                                                   const uint64_t* __restrict__ r_len, const uint64_t* __restrict__ r_first,
                                                                   const uint32_t* __restrict__ hashes, const uint64_t* __restrict__ d_consumed,
                                                                   int32_t* __restrict__ d_status, uint64_t* __restrict__ d_at) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x;
    if (d_status[f] != LZF_OK) return;
    const VFrame F = frames[f];
    const uint64_t total = d_at[f];
    int st = LZF_OK;
    uint64_t at = total;
    for (uint64_t base = 0; base < F.nb; base += 64u) {
        const uint64_t b = F.blk0 + base + lane;
        int code = LZF_OK;
        uint64_t pos = 0;
        if (base + lane < F.nb) {
            const lzf_frame_block e = ent[b];
            if (!(e.flags & LZF_FBLOCK_DELIVERED)) {
            } else if (e.flags & LZF_FBLOCK_STORED) {
                if (r_first[b] != kNoDiff) { code = LZF_MISMATCH; pos = e.out_off + r_first[b]; }
                else if (r_len[b] < e.out_len) { code = LZF_MISMATCH; pos = e.out_off + r_len[b]; }
            } else {
                const lzf_job_result r = res[b];
                if (r.status != LZF_OK) { code = r.status; pos = (e.flags & LZF_FBLOCK_LINKED) ? r.out_len + shift[b] : e.out_off + r.out_len; }
            }
        }
        const uint64_t fails = __ballot(code != LZF_OK);
        if (fails) {
            const int first = (int)__builtin_ctzll(fails);
            st = __shfl(code, first, 64);
            at = __shfl(pos, first, 64);
            break;
        }
    }
    if (lane != 0) return;
    if (st == LZF_OK && total != F.expected_len) { st = LZF_MISMATCH; at = total < F.expected_len ? total : F.expected_len; }
    if (st == LZF_OK && F.check && d_consumed[f] == F.scan_consumed && hashes[f] != F.want_content) st = LZF_F_FRAME_CHECKSUM_FAIL;
    d_status[f] = st; d_at[f] = at;
}

}  // namespace

using namespace lzf_fdev;

extern "C" {

int lzf_frame_verify_device(uint32_t n_frames, const uint8_t* const* d_in, const size_t* in_len,
                            const uint8_t* d_dict, size_t dict_len,
                            const uint8_t* const* d_expected, const size_t* expected_len,
                            uint64_t* d_at, uint64_t* d_consumed, int32_t* d_status, void* hip_stream) {
    if (n_frames && (!d_in || !in_len || !d_expected || !expected_len || !d_at || !d_status)) return LZF_E_INVALID;
    for (uint32_t f = 0; f < n_frames; ++f) if (expected_len[f] && !d_expected[f]) return LZF_E_INVALID;
    if (!d_dict) dict_len = 0;
    if (n_frames == 0) return LZF_OK;
    if (usable_device() != LZF_OK) return LZF_E_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    PoolAlloc own_consumed(st);                      // (as the size query: the kernels write `consumed` of every frame)
    if (!d_consumed) { if (!own_consumed.get(8 * (size_t)n_frames)) return LZF_E_HIP; d_consumed = own_consumed.at<uint64_t>(0); }
    Scan sc(st);
    Meta meta(st);
    Pass P;
    PoolAlloc ent_mem(st);                           // the entries: an allocation of their own, so that their addresses travel in the image
    bool ent_ok = true;
    uint64_t n_blks = 0, max_in = 0, max_stored = 0;
    size_t i_frames = 0, i_bframe = 0, i_index = 0, i_cap = 0, i_hptr = 0, i_hlen = 0;
    size_t s_jobs = 0, s_res = 0, s_shift = 0, s_ra = 0, s_rb = 0, s_rlen = 0, s_rfirst = 0, s_hash = 0;
    bool any_check = false;
    const auto more = [&](const Scan& got) {         // what the kernels behind the size query read, and room for what they write
        std::vector<VFrame> vf(n_frames);
        std::vector<uint32_t> bframe;
        std::vector<uint64_t> cap(n_frames), hlen(n_frames);
        for (uint32_t f = 0; f < n_frames; ++f) {
            const FSum& S = got.sum[f];
            const uint64_t nb = got.live(f) ? got.cnt[f] : 0;
            const bool check = got.live(f) && (S.flags & kEndmark) && (S.flags & lzf_scan::FL_CSUM) && S.status == LZF_OK;
            vf[f] = VFrame{d_in[f], d_expected[f], expected_len[f], n_blks, nb, S.consumed, S.want_content, check ? 1u : 0u};
            cap[f] = nb; hlen[f] = check ? expected_len[f] : 0;
            any_check = any_check || check;
            for (uint64_t k = 0; k < nb; ++k) {
                const TBlk& t = got.table[got.blk0[f] + k];
                const uint64_t len = t.len & ~lzf_scan::INCOMPRESSIBLE;
                if (t.len & lzf_scan::INCOMPRESSIBLE) { if (len > max_stored) max_stored = len; } else if (len > max_in) max_in = len;
                bframe.push_back(f);
            }
            n_blks += nb;
        }
        ent_ok = ent_mem.get(sizeof(lzf_frame_block) * n_blks);
        std::vector<lzf_frame_block*> index(n_frames);       // every frame's entries behind each other
        if (ent_ok) for (uint32_t f = 0; f < n_frames; ++f) index[f] = ent_mem.at<lzf_frame_block>(0) + vf[f].blk0;
        i_frames = meta.add(vf); i_bframe = meta.add(bframe); i_cap = meta.add(cap); i_hlen = meta.add(hlen);
        i_hptr = meta.add(d_expected, sizeof(void*) * (size_t)n_frames);
        i_index = meta.add(index);
        s_jobs = meta.room(sizeof(lzf_decompress_job) * n_blks); s_res = meta.room(sizeof(lzf_job_result) * n_blks);
        s_shift = meta.room(8 * n_blks); s_ra = meta.room(8 * n_blks); s_rb = meta.room(8 * n_blks); s_rlen = meta.room(8 * n_blks);
        s_rfirst = meta.room(8 * n_blks); s_hash = meta.room(4 * (size_t)n_frames);
    };
    RC_TRY(size_frames(n_frames, d_in, in_len, dict_len, d_at, d_consumed, d_status, st, sc, meta, P, more));
    if (!ent_ok) { (void)hipStreamSynchronize(st); return LZF_E_HIP; }
    const VFrame* const frames = meta.img<const VFrame>(i_frames);
    lzf_frame_block* const ent = ent_mem.at<lzf_frame_block>(0);
    if (n_blks) {
        if (n_blks > 0x7FFFFFFFull) { (void)hipStreamSynchronize(st); return LZF_E_INVALID; }
        RC_TRY(index_blocks(P, meta, meta.img<lzf_frame_block* const>(i_index), meta.img<const uint64_t>(i_cap), nullptr, st));
        lzf_decompress_job* const jobs = meta.scr<lzf_decompress_job>(s_jobs);
        lzf_job_result* const res = meta.scr<lzf_job_result>(s_res);
        KERNEL(lzf_verify_jobs_kernel, dim3((uint32_t)((n_blks + 255u) / 256u)), dim3(256), 0, st, frames, meta.img<const uint32_t>(i_bframe),
               (const lzf_frame_block*)ent, n_blks, d_dict, (uint64_t)dict_len, jobs, meta.scr<uint64_t>(s_shift), meta.scr<const uint8_t*>(s_ra),
               meta.scr<const uint8_t*>(s_rb), meta.scr<uint64_t>(s_rlen));
        // (res and r_first are zeroed scratch where a launch below is skipped.  The fold reads res[b] only for a DELIVERED compressed block
        //  and r_first[b] only for a DELIVERED stored block; an empty block stops the frame and is never DELIVERED, so either implies
        //  max_in > 0 / max_stored > 0 and the launch that writes the word.)
        if (max_in) RC_TRY(lzf_decompress_verify_batch(jobs, res, (uint32_t)n_blks, max_in, st));
        if (max_stored)
            KERNEL(lzf_first_diff_kernel, dim3((uint32_t)n_blks), dim3(64), 0, st, meta.scr<const uint8_t* const>(s_ra), meta.scr<const uint8_t* const>(s_rb),
                   meta.scr<const uint64_t>(s_rlen), meta.scr<uint64_t>(s_rfirst));
    }
    if (any_check)
        RC_TRY(lzf_xxh32_batch(meta.img<const uint8_t* const>(i_hptr), meta.img<const uint64_t>(i_hlen), meta.scr<uint32_t>(s_hash), n_frames, st));
    KERNEL(lzf_frame_verify_fold_kernel, dim3(n_frames), dim3(64), 0, st, frames, (const lzf_frame_block*)ent, meta.scr<const lzf_job_result>(s_res),
           meta.scr<const uint64_t>(s_shift), meta.scr<const uint64_t>(s_rlen), meta.scr<const uint64_t>(s_rfirst), meta.scr<const uint32_t>(s_hash),
           (const uint64_t*)d_consumed, d_status, d_at);
    return meta.wait();                              // the image has left host memory; the kernels run on
}

}  // extern "C"
