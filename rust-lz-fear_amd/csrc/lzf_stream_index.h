// lzf_stream_index.h — the rules of the frame index of a stream of back-to-back frames (include/lzfear_frame.h,
// lzf_frame_stream_decompressed_size_device / lzf_stream_index_locate) as __host__ __device__ code, like lzf_stream_walk.h.
//
//   ends_stream   the stream rule's stop: a frame that does not end at its EndMark with LZF_OK ends its stream (the predicate
//                 of lzf_stream_fold_kernel: status != LZF_OK, or `consumed` short of where the structural walk ended)
//   fill_entry    one lzf_stream_frame from a frame's size results: flags, and the content size from a parsed header
//   locate        the frames of an index whose output meets [a, b): two binary searches over the frames' ends (locate_units,
//                 generic over the entry type: lzf_block_index.h runs it over the blocks of a frame)
//
// lzf_stream_index_kernel (frame_device_index.hip) runs ends_stream and fill_entry one lane per frame; lzf_stream_index_locate is
// locate.  The CPU tests compile this header with g++ (tests/emu/emu_stream_index.cpp).
#ifndef LZF_STREAM_INDEX_H
#define LZF_STREAM_INDEX_H

#include "../../include/lzfear_frame.h"
#include "lzf_frame_scan.h"

namespace lzf_sindex {

// `full`: where the frame's structural walk ended if it reached the EndMark without error, ~0 otherwise
LZF_SCAN_HD inline bool ends_stream(int status, uint64_t consumed, uint64_t full) { return status != lzf_scan::OK || consumed != full; }

// The header's content size field: 8 bytes behind magic, FLG and BD (decompress.rs:111-118), read bytewise.  `frame` is only
// looked at when the header parsed and FLG has FL_CSIZE: the header parse has then read these bytes.
LZF_SCAN_HD inline uint64_t content_size(const uint8_t* frame, bool header_parsed, uint32_t flg) {
    if (!header_parsed || !(flg & lzf_scan::FL_CSIZE)) return LZF_STREAM_NO_CONTENT_SIZE;
    return (uint64_t)lzf_scan::rd32(frame + 6) | ((uint64_t)lzf_scan::rd32(frame + 10) << 32);
}

// Entry of the frame at in[in_off, len): its own size results, its place, and what the stream rule says about it.  `behind`: an
// earlier frame ended the stream (out_off is then the stream's out_len).
LZF_SCAN_HD inline lzf_stream_frame fill_entry(const uint8_t* frame, bool header_parsed, uint32_t flg, uint64_t in_off, int status,
                                               uint64_t out_len, uint64_t consumed, uint64_t full, uint64_t out_off, bool behind) {
    lzf_stream_frame e;
    e.in_off = in_off; e.consumed = consumed; e.out_off = out_off; e.out_len = out_len;
    e.content_size = content_size(frame, header_parsed, flg);
    e.status = status;
    e.flags = (ends_stream(status, consumed, full) ? 0u : LZF_SFRAME_COMPLETE) | (behind ? LZF_SFRAME_BEHIND_STOP : 0u);
    return e;
}

// first k in [0, n) with pred(k), n if none; pred is false up to some k and true from there on
template <class Pred>
LZF_SCAN_HD inline uint64_t partition_point(uint64_t n, Pred&& pred) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (pred(mid)) hi = mid; else lo = mid + 1; }
    return lo;
}

// Units [*first, *first + *count) of index[0, n) whose output meets [a, b): unit k with out_off < b && out_off + out_len > a,
// among the entries in front of the first one for which outside(entry) holds (a prefix of the index: the frames without
// LZF_SFRAME_BEHIND_STOP of a stream's index, the delivered blocks of a frame's, lzf_block_index.h).  A unit's end, out_off +
// out_len, is the next unit's out_off: the ends never decrease, so the first unit is the first whose end is beyond a, and the
// last one is the first whose end reaches b, or the total where b is beyond it.  Both have bytes of their own: units of zero
// length are never at either edge of the result (inside it they add nothing).  Nothing meets the range: *count = 0, *first = 0.
template <class Entry, class Outside>
LZF_SCAN_HD inline void locate_units(const Entry* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count, Outside&& outside) {
    *first = 0; *count = 0;
    const uint64_t m = partition_point(n, [&](uint64_t k) { return outside(index[k]); });
    if (m == 0 || a >= b) return;
    const uint64_t total = index[m - 1].out_off + index[m - 1].out_len;
    const uint64_t bb = b < total ? b : total;
    if (bb <= a) return;
    const uint64_t lo = partition_point(m, [&](uint64_t k) { return index[k].out_off + index[k].out_len > a; });
    const uint64_t hi = partition_point(m, [&](uint64_t k) { return index[k].out_off + index[k].out_len >= bb; });
    *first = lo; *count = hi - lo + 1;      // (a < bb <= total: both exist, and lo <= hi)
}

// the frames of a stream's index: everything in front of the first entry with LZF_SFRAME_BEHIND_STOP
LZF_SCAN_HD inline void locate(const lzf_stream_frame* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count) {
    locate_units(index, n, a, b, first, count, [](const lzf_stream_frame& e) { return (e.flags & LZF_SFRAME_BEHIND_STOP) != 0; });
}

}  // namespace lzf_sindex

#endif  // LZF_STREAM_INDEX_H
