// lzf_frame_head_rules.h — "the first bytes of this frame": LZ4FrameReader (src/framed/decompress.rs:102-288) with one added
// rule, as __host__ __device__ code on top of lzf_frame_scan.h (the header parse, the walk's step) and lzf_head_rules.h (the head
// of one block).
//
// `target` is the number of bytes asked for; `pos` is the number of bytes delivered when decode_block (:198) is entered.
//   header    read_header runs always, also for target 0; its status and nothing else decides a frame whose header fails
//             (out_len 0);
//   stop      the reader ends with LZF_OK in front of the first block entered at pos >= target: that block's length word and
//             everything behind it is never looked at, malformed or not;
//   walk      a block entered at pos < target is read as the reader reads it — lzf_scan::walk_blocks' step: the EndMark (its
//             content checksum word must be there, else LZF_F_INPUT_ERROR, but it is NOT compared) ends the frame with LZF_OK
//             and out_len = pos, below the target: the frame ended first; LZF_F_BLOCK_SIZE_OVERFLOW for a length word above
//             block_maxsize; LZF_F_INPUT_ERROR where the payload or its checksum word is cut off (the reader's read_exact
//             comes before the decode);
//   checksums block checksums are stepped over, NOT verified: hashing a 4 MiB block to read 64 bytes of it would cost more
//             than everything else the call does.  The size, verify and decode calls verify them; this call is for reading a
//             preamble;
//   stored    the bytes at positions below the target are copied, n = the block's length;
//   compressed  lzf_head::head_block on the job frame_jobs.h states for the decode (block_job below).  A codec status 1..4 ends
//             the frame with that status and out_len = pos, the length in front of the failing block (bytes below the target
//             may have been written);
//   behind a block that ended in front of the target (pos + n < target) the reader's remaining stops, in the delivery's order
//             (frame_deliver_body.inc): n > block_maxsize is LZF_F_BLOCK_SIZE_OVERFLOW, n == 0 is LZF_OK (the io::Read adapter
//             stops at an empty block), both with out_len = pos; otherwise pos += n.  A block that reaches the target is asked
//             neither question: an error at or behind the target is not seen, as in the raw call;
//   result    LZF_OK with out_len = min(pos reached, target).  out_len < target: the frame ended first; out_len == target does
//             not say whether more follows.  No byte at or beyond out + target is written;
//   contract  a target of 2 GiB - 256 (lzf_head::kMaxLen) or more is LZF_CONTRACT with nothing read: a head is short, and with
//             that bound no position the walk holds leaves the decoder's 31-bit contract.  The lengths head_block itself
//             refuses (the dictionary's) stay LZF_CONTRACT, reported when a compressed block is entered.
// head_frame below is the one definition of the result: the CPU tests run it (tests/emu/emu_frame_head.cpp) against the oracle's
// decode cut at the target, and the kernel (frame_device_head.hip) is held to it and takes its steps from the same functions.
#ifndef LZF_FRAME_HEAD_RULES_H
#define LZF_FRAME_HEAD_RULES_H

#include "lzf_frame_scan.h"
#include "lzf_head_rules.h"

namespace lzf_frame_head {

struct Result { int status; uint64_t out_len; };

LZF_SIZE_HD bool contract(uint64_t target) { return target >= lzf_head::kMaxLen; }

// The walk's step from input offset r: the block entered there (found; off and end_off are offsets into the frame), or what ends
// the walk instead — the EndMark (status OK) or a structural error.
struct Next { int status; bool found; lzf_scan::Block b; };
LZF_SCAN_HD inline Next next_block(const uint8_t* in, uint64_t in_len, uint64_t r, const lzf_scan::Header& h) {
    const lzf_scan::Header from{lzf_scan::OK, 0, 0, h.flags, h.bd, h.block_maxsize};       // (the walk starts at header_len: 0 of in + r)
    Next x{lzf_scan::OK, false, lzf_scan::Block{0, 0, 0, 0, 0}};
    const lzf_scan::Walk w = lzf_scan::walk_blocks(in + r, in_len - r, from, [&](const lzf_scan::Block& b) { x.b = b; x.found = true; return false; });
    x.status = w.status;
    x.b.off += r; x.b.end_off += r;
    return x;
}

// The head job of a compressed block entered at pos (frame_jobs.h: build): the job's `out` is the frame's output + shift.
struct BlockJob { uint64_t shift, existing, limit, target; };
LZF_SIZE_HD BlockJob block_job(bool linked, uint64_t pos, uint64_t bmax, uint64_t target) {
    return linked ? BlockJob{0ull, pos, pos + bmax, target} : BlockJob{pos, 0ull, bmax, target - pos};
}

// Does a block of n bytes entered at pos reach the target?  (Then nothing more is asked of it.)
LZF_SIZE_HD bool reaches(uint64_t pos, uint64_t n, uint64_t target) { return n >= target - pos; }       // (pos < target)

// Behind a block that ended in front of the target: the stop it raises (ends: out_len = pos), or none.
struct Behind { int status; bool ends; };
LZF_SIZE_HD Behind behind_block(uint64_t n, uint64_t bmax) {
    if (n > bmax) return Behind{lzf_scan::BLOCK_SIZE_OVERFLOW, true};
    return Behind{lzf_scan::OK, n == 0};
}

// The serial reference.  out1(r) = out[r] for r below the position being written; put1(r, byte) writes out[r], r < target.
template <class RO, class WO>
LZF_SCAN_HD inline Result head_frame(const uint8_t* in, uint64_t in_len, const uint8_t* dict, uint64_t dict_len, RO out1, WO put1, uint64_t target) {
    if (contract(target)) return Result{lzf_head::CONTRACT, 0};
    const lzf_scan::Header h = lzf_scan::read_header(in, in_len);
    if (h.status != lzf_scan::OK) return Result{h.status, 0};
    const bool linked = (h.flags & lzf_scan::FL_INDEP) == 0;
    uint64_t pos = 0, r = h.header_len;
    while (!lzf_head::stops(pos, target)) {
        const Next x = next_block(in, in_len, r, h);
        if (!x.found) return Result{x.status, pos};                  // the EndMark (OK), or the walk's error
        r = x.b.end_off;
        uint64_t n = x.b.len;
        if (!x.b.compressed) {
            const uint64_t k = lzf_head::below(pos, n, target);
            for (uint64_t i = 0; i < k; ++i) put1(pos + i, in[x.b.off + i]);
        } else {
            const BlockJob j = block_job(linked, pos, h.block_maxsize, target);
            const uint8_t* const p = in + x.b.off;
            const uint32_t len = x.b.len;
            auto rd1 = [&](uint32_t q) -> uint32_t { return p[q]; };
            auto rd4 = [&](uint32_t q) -> uint32_t {
                uint32_t v = 0;
                for (uint32_t i = 0; i < 4u && q + i < len; ++i) v |= (uint32_t)p[q + i] << (8u * i);
                return v;
            };
            auto ffrun = [&](uint32_t q) -> uint32_t { uint32_t c = 0; while (q + c < len && p[q + c] == 255u) ++c; return c; };
            auto pre1 = [&](uint64_t k) -> uint32_t { return dict[k]; };
            const lzf_head::Result v = lzf_head::head_block(len, rd4, rd1, ffrun, pre1, dict_len, [&](uint64_t q) -> uint32_t { return out1(j.shift + q); },
                                                            [&](uint64_t q, uint32_t b) { put1(j.shift + q, b); }, j.existing, j.target, j.limit);
            if (v.status != lzf_size::OK) return Result{v.status, pos};
            n = v.out_len - j.existing;                              // (min(the block's length, what was asked of it))
        }
        if (reaches(pos, n, target)) break;
        const Behind s = behind_block(n, h.block_maxsize);
        if (s.ends) return Result{s.status, pos};
        pos += n;
    }
    return Result{lzf_scan::OK, target};
}

}  // namespace lzf_frame_head

#endif  // LZF_FRAME_HEAD_RULES_H
