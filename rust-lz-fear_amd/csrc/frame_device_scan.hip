// frame_device_scan.hip — the scans of the device frame layer (frame_device_common.h has the map), and the calls that only scan.
//
// Frame scan, one lane per frame, lzf_frame_scan.h's header parse (decompress.rs:102-161) and block walk (:198-235):
//   pass 1 (lzf_frame_scan_kernel, scan_summaries): a 64-byte summary per frame comes back (one wait);
//   pass 2 (lzf_frame_table_kernel, scan_table): the block table, 24 bytes per block, comes back (one more wait).
// Stream scan, one lane per stream, lzf_stream_walk.h's walk over back-to-back frames (lzf_stream_scan_kernel): launch one counts
// the frames of every stream (count_streams), launch two lists where they begin (scan_streams); a wait each.
// lzf_frame_decompress_bound_device and lzf_frame_block_count_device read the summaries, lzf_frame_stream_count_device the
// counts, lzf_frame_stream_bound_device the summaries of the frames the stream scan lists.
#include "frame_device_common.h"
#include "lzf_stream_walk.h"

namespace {

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
}  // namespace

namespace lzf_fdev __attribute__((visibility("hidden"))) {

// [ptrs | lens] of a scan's n inputs at the head of its device arguments
static int upload_inputs(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, PoolAlloc& args) {
    std::vector<uint64_t> h(2 * (size_t)n);
    for (uint32_t f = 0; f < n; ++f) { h[f] = reinterpret_cast<uintptr_t>(d_in[f]); h[n + f] = in_len[f]; }
    DEV_TRY(hipMemcpyAsync(args.p, h.data(), 16 * (size_t)n, hipMemcpyHostToDevice, st));
    return LZF_OK;
}

int scan_summaries(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, Scan& sc,
                   int32_t* d_status, uint64_t* d_out_len, uint64_t* d_consumed) {
    PoolAlloc& args = sc.args;
    const size_t o_sum = up256(32 * (size_t)n);
    if (!args.get(o_sum + sizeof(FSum) * (size_t)n)) return LZF_E_HIP;
    RC_TRY(upload_inputs(n, d_in, in_len, st, args));
    KERNEL(lzf_frame_scan_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, args.at<const uint8_t* const>(0), args.at<const uint64_t>(8 * (size_t)n), n,
           args.at<FSum>(o_sum), d_status, d_out_len, d_consumed);
    sc.sum.resize(n);
    DEV_TRY(hipMemcpyAsync(sc.sum.data(), args.at<FSum>(o_sum), sizeof(FSum) * (size_t)n, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    return LZF_OK;
}

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

int count_streams(uint32_t n, const uint8_t* const* d_in, const size_t* in_len, hipStream_t st, PoolAlloc& args, std::vector<uint64_t>& counts) {
    if (!args.get(32 * (size_t)n)) return LZF_E_HIP;
    counts.resize(n);
    RC_TRY(upload_inputs(n, d_in, in_len, st, args));
    KERNEL(lzf_stream_scan_kernel, dim3((n + 63u) / 64u), dim3(64), 0, st, args.at<const uint8_t* const>(0), args.at<const uint64_t>(8 * (size_t)n), n,
           args.at<uint64_t>(16 * (size_t)n), (const uint64_t*)nullptr, (uint64_t*)nullptr);
    DEV_TRY(hipMemcpyAsync(counts.data(), args.at<uint64_t>(16 * (size_t)n), 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    DEV_TRY(hipStreamSynchronize(st));
    return LZF_OK;
}

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

}  // namespace lzf_fdev

using namespace lzf_fdev;

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

}  // extern "C"
