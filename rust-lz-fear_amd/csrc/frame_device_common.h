// frame_device_common.h — what the sources of the frame layer for frames in device memory share (include/lzfear_frame.h,
// "frames in device memory").  The map:
//   frame_device_scan.hip      the frame scan (summaries, block table) and the stream scan, with the calls that only scan:
//                              lzf_frame_decompress_bound_device, lzf_frame_stream_bound_device, lzf_frame_stream_count_device,
//                              lzf_frame_block_count_device
//   frame_device_decode.hip    plan_frames / plan_pass / decode_frames / size_frames and the delivery, placement and fold kernels:
//                              lzf_frame_decompress_device_many, lzf_frame_decompress_stream_device, lzf_frame_decompressed_size_device
//   frame_device_index.hip     the stream index, the block index and runs of blocks: lzf_frame_stream_decompressed_size_device,
//                              lzf_frame_block_index_device, lzf_frame_decompress_blocks_device, the two *_locate calls
//   frame_device_verify.hip    size_frames, the block index into scratch, a verify job or a stored range per delivered block and
//                              the fold: lzf_frame_verify_device
//   frame_device_head.hip      one wavefront per frame, the frame walk and the block's head walk together, nothing read back:
//                              lzf_frame_head_device
//   frame_device_resume.hip    a cursor per frame in device memory, the bounded walk from it (lzf_frame_resume_rules.h), the pieces'
//                              blocks through enqueue_blocks and the delivery body, the hash update and the kernel that moves the
//                              cursors: lzf_frame_resume_device, lzf_frame_cursor_bytes
//   frame_device_append.hip    a write cursor per frame in device memory (lzf_frame_append_rules.h): the offer's blocks through the
//                              compress plan and launches, the prepare, append-assembly and commit kernels:
//                              lzf_frame_append_device, lzf_frame_wcursor_bytes
//   frame_device_compress.hip  plan_cpass / compress_frames / compress_streams and the assembly kernels: lzf_frame_compress_device_many,
//                              lzf_frame_compressed_size_device, lzf_frame_compress_stream_device, lzf_frame_compress_stream_size_device,
//                              lzf_frame_compress_stream_bound
// One copy of each rule.  The walk is lzf_frame_scan.h's (the host driver runs the same header).  The passes of the memory budget
// are frame_jobs.h's split_passes, and the jobs of a pass frame_jobs.h's plans (Plan / build, CPlan / compress_plan), for the device
// drivers as for the host drivers.  The small arrays of a call travel in one Meta: one image, one upload, one event, typed
// accessors.  The one-wavefront-per-frame / per-stream / per-run kernels share wave_incl_scan.
//
// Every kernel stands in its source's unnamed namespace, and so do the records below that kernels take as arguments: they are
// part of the kernels' symbols.  A kernel has one source; where another source needs its launch, the source that has the kernel
// offers a host function (fold_streams, empty_streams).  Host code that crosses sources is lzf_fdev's, hidden from the library's
// surface.
#ifndef LZF_FRAME_DEVICE_COMMON_H
#define LZF_FRAME_DEVICE_COMMON_H

#include <hip/hip_runtime.h>
#include <cstring>
#include <functional>
#include <vector>
#include "../../include/lzfear_frame.h"
#include "lzf_frame_scan.h"
#include "frame_jobs.h"

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

// per frame and per block of a pass, for the delivery kernels
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

// per block of a compress pass, for the assembly kernels (frame_device_compress.hip, frame_device_append.hip)
struct CBlkDesc {
    const uint8_t* raw;         // the block in the caller's input: a stored block's payload
    const uint8_t* slot;        // its job's output: a compressed block's payload
    uint32_t job, raw_len;      // job of the pass (its result), the block's length
};
constexpr uint32_t kBlockSums = 1u, kContentSum = 2u;

// ---- the wave-wide sums of the one-wavefront-per-frame / per-stream kernels
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

}  // namespace

namespace lzf_fdev __attribute__((visibility("hidden"))) {

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

inline int usable_device() {
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
inline int pass_budget(hipStream_t st, size_t* budget) {
    *budget = lzf_frame_jobs::memory_budget();
    if (!*budget) { size_t free_b = 0, total_b = 0; DEV_TRY(hipMemGetInfo(&free_b, &total_b)); *budget = free_b / 2; }
    return LZF_OK;
}
// frames [first[s], first[s + 1]) are stream s: the stream of every frame
inline std::vector<uint32_t> streams_of(uint32_t n_streams, const uint64_t* first) {
    std::vector<uint32_t> of((size_t)first[n_streams]);
    for (uint32_t s = 0; s < n_streams; ++s) for (uint64_t f = first[s]; f < first[s + 1]; ++f) of[(size_t)f] = s;
    return of;
}
// ---- frame_device_scan.hip
// What the scan of n frames brings back to the host: the summaries (pass 1) and, with scan_table, the block table (pass 2):
// frame f's blocks are table[blk0[f], blk0[f] + cnt[f]).  `args` keeps [ptrs | lens | blk0 | cnt] on the device between the two.
struct Scan {
    PoolAlloc args;
    std::vector<FSum> sum;
    std::vector<uint64_t> blk0, cnt;
    std::vector<TBlk> table;
    explicit Scan(hipStream_t st) : args(st) {}
    bool live(uint32_t f) const { return (sum[f].flags & kLive) != 0; }
    // the stream fold's f_full: what the frame consumes where its walk reached the EndMark, ~0 where the scan already failed
    uint64_t full(uint32_t f) const { return live(f) && sum[f].status == LZF_OK ? sum[f].consumed : ~0ull; }
};
// Scan pass 1 of n frames: summaries back on the host (the call's first wait).
int scan_summaries(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, Scan& sc,
                   int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed);
// Scan pass 2: the block table of every frame whose header parses, back on the host (the call's second wait).
int scan_table(uint32_t n, hipStream_t st, Scan& sc);
// The stream scan's first launch: the frame count of every stream back on the host (one wait).  `args` keeps
// [ptrs | lens | counts | first] on the device for the second launch.
int count_streams(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, PoolAlloc& args, std::vector<uint64_t>& counts);
// The stream scan of n streams: the frames of every stream back on the host (two waits: the counts, then the starts).  Stream s
// is frames [first[s], first[s + 1]); frame f is f_in[f][0, f_len[f]): everything from its start to the end of its stream, as the
// reader of the frame sees it.
int scan_streams(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, std::vector<uint64_t>& first,
                 std::vector<const uint8_t*>& f_in, std::vector<size_t>& f_len);

// ---- frame_device_decode.hip
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
// The block checksums (lzf_xxh32_batch) and the decode steps (the chain step, then lzf_decompress_batch_sized; with sizes_only their
// twins that carry lengths in the place of bytes) of a planned pass, enqueued.  Reads of P: plan, n_sums, i_jobs, i_steps, i_sptr,
// i_slen, s_res, s_state, s_sums.  The whole-frame decode, the size query and the resumable decode (frame_device_resume.hip) run
// their blocks through it.
int enqueue_blocks(const Pass& P, const Meta& meta, bool sizes_only, hipStream_t st);
// The size query of n frames (lzf_frame_decompressed_size_device's body, and the per-frame half of the stream size query): the
// decode call's scan (two waits), its plan with sizes_only (plan_frames, plan_pass: jobs' lengths and descriptors, no addresses),
// block checksums (they decide where delivery stops), lzf_decompressed_size_batch for the decode (linked frames in lock-step,
// lzf_chain_size_step_kernel between the steps), lzf_frame_size_deliver_kernel for the delivery.  No output slots, hence one pass
// whatever the memory budget is.  `more(sc)` puts what the caller's own kernels behind this need into the call's image before
// its one upload; the caller ends with meta.wait().  Where every header failed and `more` added nothing, nothing is uploaded:
// the scan kernel wrote the results.  `P` is the call's one pass: a caller whose kernels read the descriptors, the job results
// or the block checksums (the block index) finds them there once the call has returned; P.n_frames == 0: nothing was planned.
int size_frames(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, size_t dict_len, uint64_t* d_out_len, uint64_t* d_consumed,
                int32_t* d_status, hipStream_t st, Scan& sc, Meta& meta, Pass& P, const std::function<void(const Scan&)>& more);
// lzf_stream_fold_kernel's launch: the frames' final results (f_*, with f_full = Scan::full) folded into the results of the
// streams, stream s being frames [first[s], first[s + 1]).  Every array is a device address.
int fold_streams(uint32_t n_streams, const uint64_t* first, const int32_t* f_status, const uint64_t* f_len, const uint64_t* f_consumed,
                 const uint64_t* f_full, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames, hipStream_t st);
// lzf_stream_empty_kernel's launch, for a call whose streams are all empty: LZF_OK, 0, 0, 0 for every stream
int empty_streams(uint32_t n_streams, int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed, uint64_t* d_n_frames, hipStream_t st);

// ---- frame_device_index.hip
// lzf_frame_block_index_kernel's launch over the pass size_frames planned (after it has returned): the delivery body in its index
// mode, frame q of the pass into x_index[frame] (x_cap[frame] entries at most; device arrays of the call's n frames).
int index_blocks(const Pass& P, const Meta& meta, lzf_frame_block* const* x_index, const uint64_t* x_cap, uint64_t* d_n_listed, hipStream_t st);

// ---- frame_device_compress.hip
// lzf_frame_patch_kernel's launch: the checksum words d_val[k] at their unaligned places d_at[k] (NULL: skipped), k < n; n == 0: no launch
int patch_words(uint8_t* const* d_at, const uint32_t* d_val, size_t n, hipStream_t st);

}  // namespace lzf_fdev

#endif  // LZF_FRAME_DEVICE_COMMON_H
