// frame_device_index.hip — the indexes of the device frame layer (frame_device_common.h has the map).
//
// lzf_frame_stream_decompressed_size_device: the stream scan, the size query over every frame it lists (size_frames), the decode's
// fold (fold_streams), and lzf_stream_index_kernel (lzf_stream_index.h's rules, one wavefront per stream) for the frame index;
// lzf_stream_index_locate is that header's locate on the host.
// lzf_frame_block_index_device: the size query over the caller's frames, then lzf_frame_block_index_kernel — the delivery body
// in its index mode, over the size query's descriptors, job results and block checksums — for the block index of every frame
// (lzf_block_index.h's rules); lzf_block_index_locate is that header's locate.
// lzf_frame_decompress_blocks_device: runs of consecutive blocks, planned from the caller's copies of the entries alone (no scan,
// no read-back): checksums, the decode of every block at its final place with its exact length as capacity, the stored copies,
// and lzf_block_run_fold_kernel, one wavefront per run, for status and out_len.
#include "frame_device_common.h"
#include "lzf_stream_index.h"
#include "lzf_block_index.h"

namespace {

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

}  // namespace

namespace lzf_fdev __attribute__((visibility("hidden"))) {

int index_blocks(const Pass& P, const Meta& meta, lzf_frame_block* const* x_index, const uint64_t* x_cap, uint64_t* d_n_listed, hipStream_t st) {
    KERNEL(lzf_frame_block_index_kernel, dim3(P.n_frames), dim3(64), 0, st, meta.img<const DFrameDesc>(P.i_frames), meta.img<const DBlkDesc>(P.i_blks),
           meta.img<const lzf_decompress_job>(P.i_jobs), meta.scr<const lzf_job_result>(P.s_res), meta.scr<const uint32_t>(P.s_sums), x_index, x_cap, d_n_listed);
    return LZF_OK;
}

}  // namespace lzf_fdev

using namespace lzf_fdev;

extern "C" {

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
        RC_TRY(empty_streams(n_streams, d_status, d_out_len, d_consumed, d_n_frames, st));
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
        for (uint32_t f = 0; f < n; ++f) { full[f] = got.full(f); flags[f] = got.sum[f].flags; }
        i_in = meta.add(d_in, sizeof(void*) * (size_t)n_streams); i_first = meta.add(first);
        i_off = meta.add(off); i_flags = meta.add(flags); i_full = meta.add(full);
        if (d_index) {
            const std::vector<uint64_t> cap(index_cap, index_cap + n_streams);
            i_index = meta.add(d_index, sizeof(void*) * (size_t)n_streams); i_cap = meta.add(cap);
        }
    };
    Pass P;
    RC_TRY(size_frames((uint32_t)n, f_in.data(), f_len.data(), dict_len, f_out_len, f_consumed, f_status, st, sc, meta, P, more));
    RC_TRY(fold_streams(n_streams, meta.img<const uint64_t>(i_first), f_status, f_out_len, f_consumed, meta.img<const uint64_t>(i_full),
                        d_status, d_out_len, d_consumed, d_n_frames, st));
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
        RC_TRY(index_blocks(P, meta, d_index ? meta.img<lzf_frame_block* const>(i_index) : (lzf_frame_block* const*)nullptr,
                            d_index ? meta.img<const uint64_t>(i_cap) : (const uint64_t*)nullptr, d_n_listed, st));
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
