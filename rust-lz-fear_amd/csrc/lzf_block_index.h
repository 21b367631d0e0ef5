// lzf_block_index.h — the rules of the block index of a frame (include/lzfear_frame.h, lzf_frame_block_index_device /
// lzf_block_index_locate / lzf_frame_decompress_blocks_device) as __host__ __device__ code, next to lzf_stream_index.h.
//
//   place_of      where a block stands to the frame's stop: delivered, the stopping block, behind it
//   fill_entry    one lzf_frame_block from what the walk found of a block and what the delivery's stop rules
//                 (frame_deliver_body.inc) decided about it: the flags, the status, out_off on either side of the stop
//   locate        the delivered blocks of an index whose output meets [a, b): lzf_stream_index.h's search over another entry
//   check_run     what lzf_frame_decompress_blocks_device asks of a run of entries before it enqueues anything
//   run_total     the bytes a run decodes to
//
// lzf_frame_block_index_kernel (frame_device_index.hip) is the delivery body in its index mode and runs fill_entry one lane per block;
// the host runs check_run and locate.  The CPU tests compile this header with g++ (tests/emu/emu_block_index.cpp).
#ifndef LZF_BLOCK_INDEX_H
#define LZF_BLOCK_INDEX_H

#include "../../include/lzfear_frame.h"
#include "lzf_stream_index.h"

namespace lzf_bindex {

// What the stop rules say about a block, as the delivery body has it per lane: `code` the block's own status (0: none), `n` its
// decoded length (0 where code is a checksum or codec error), `at` the sum of n over the blocks before it in its frame.
//   place   DELIVERED: in front of the first stop.  STOP: the first block that stops the reader.  BEHIND: every block after it;
//           `frame_len` is then the frame's out_len (the stopping block's `at`).
enum Place : uint32_t { DELIVERED = 0, STOP = 1, BEHIND = 2 };
// block k of a round of blocks whose first stopping block is `first_stop` (any value beyond the round: none stops), in a frame
// that an earlier round has stopped or not
LZF_SCAN_HD inline Place place_of(bool stopped_before, uint32_t k, uint32_t first_stop) {
    return stopped_before || k > first_stop ? BEHIND : k == first_stop ? STOP : DELIVERED;
}

LZF_SCAN_HD inline lzf_frame_block fill_entry(uint64_t in_off, uint32_t in_len, bool stored, bool has_sum, uint32_t want_sum, bool linked,
                                              uint64_t block_maxsize, int code, uint64_t n, uint64_t at, uint64_t frame_len, Place place) {
    lzf_frame_block e;
    e.in_off = in_off; e.out_off = place == BEHIND ? frame_len : at; e.out_len = n;
    e.in_len = in_len; e.want_sum = has_sum ? want_sum : 0u; e.block_maxsize = (uint32_t)block_maxsize;
    e.status = code;
    e.flags = (stored ? LZF_FBLOCK_STORED : 0u) | (has_sum ? LZF_FBLOCK_HAS_SUM : 0u) | (linked ? LZF_FBLOCK_LINKED : 0u)
            | (place == DELIVERED ? LZF_FBLOCK_DELIVERED : 0u) | (place == BEHIND ? LZF_FBLOCK_BEHIND_STOP : 0u);
    e.reserved = 0u;
    return e;
}

// the delivered blocks are a prefix of the index: everything in front of the first entry without LZF_FBLOCK_DELIVERED
LZF_SCAN_HD inline void locate(const lzf_frame_block* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count) {
    lzf_sindex::locate_units(index, n, a, b, first, count, [](const lzf_frame_block& e) { return (e.flags & LZF_FBLOCK_DELIVERED) == 0; });
}

// Why a run is refused (LZF_E_INVALID), RUN_OK otherwise.  e[0, count) are consecutive entries of the index of a frame of
// frame_len bytes.  What holds for an accepted run: every payload (and checksum word) lies inside the frame, every block's
// place [out_off - e[0].out_off, + out_len) lies inside [0, run_total), the places do not overlap, and a stored block is
// copied to a place of its own length.
enum RunCheck : int { RUN_OK = 0, RUN_NOT_DELIVERED = 1, RUN_LINKED = 2, RUN_INPUT_RANGE = 3, RUN_IN_LEN = 4, RUN_OUT_LEN = 5,
                      RUN_STORED_LEN = 6, RUN_NOT_CONTIGUOUS = 7 };
LZF_SCAN_HD inline RunCheck check_run(const lzf_frame_block* e, uint64_t count, uint64_t frame_len) {
    for (uint64_t k = 0; k < count; ++k) {
        const lzf_frame_block& b = e[k];
        if (!(b.flags & LZF_FBLOCK_DELIVERED)) return RUN_NOT_DELIVERED;
        if (b.flags & LZF_FBLOCK_LINKED) return RUN_LINKED;
        const uint64_t span = (uint64_t)b.in_len + ((b.flags & LZF_FBLOCK_HAS_SUM) ? 4u : 0u);
        if (b.in_off > frame_len || frame_len - b.in_off < span) return RUN_INPUT_RANGE;
        if (b.in_len > b.block_maxsize) return RUN_IN_LEN;
        if (b.out_len > b.block_maxsize) return RUN_OUT_LEN;
        if ((b.flags & LZF_FBLOCK_STORED) && b.out_len != b.in_len) return RUN_STORED_LEN;
        if (k + 1 < count && e[k + 1].out_off - b.out_off != b.out_len) return RUN_NOT_CONTIGUOUS;
    }
    return RUN_OK;
}

// the bytes of an accepted run (out_len <= block_maxsize < 2^32 each: no overflow below 2^32 blocks)
LZF_SCAN_HD inline uint64_t run_total(const lzf_frame_block* e, uint64_t count) {
    uint64_t t = 0;
    for (uint64_t k = 0; k < count; ++k) t += e[k].out_len;
    return t;
}

}  // namespace lzf_bindex

#endif  // LZF_BLOCK_INDEX_H
