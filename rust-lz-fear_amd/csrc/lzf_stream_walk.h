// lzf_stream_walk.h — the frame-to-frame walk of a stream of back-to-back LZ4 frames ("This also allows LZ4 frames to be
// concatenated back to back", src/framed/mod.rs:6) as __host__ __device__ code, on top of lzf_frame_scan.h.
//
//   walk_frames   the loop a caller of lzf_frame_decompress writes with `consumed`: read_header and walk_blocks once per frame,
//                 hop to where the frame's reader stopped, go on while input is left
//
// The walk stops behind the first frame whose header or block walk fails; that frame is still reported (it is the stream's
// last frame: its status and `consumed` end the stream).  1-3 trailing bytes are a frame whose header is cut short
// (INPUT_ERROR, consumed = everything); 4 or more trailing bytes that are not the magic — skippable and legacy frames
// included, the reference knows neither — are a frame that fails with WRONG_MAGIC after 4 bytes.
// What only the decode finds (a block checksum, a codec error, a block beyond block_maxsize, an empty block, the output
// capacity, the content checksum) ends the stream earlier: the stream kernels of frame_device_decode.hip apply those stops to the
// frames this walk lists.  The stream scan kernel runs walk_frames one lane per stream; the CPU tests compile this header
// with g++ (tests/emu/emu_stream_walk.cpp).
#ifndef LZF_STREAM_WALK_H
#define LZF_STREAM_WALK_H

#include "lzf_frame_scan.h"

namespace lzf_scan {

struct StreamWalk {
    int status;                 // OK, or the header / walk error of the last frame
    uint64_t consumed;          // bytes read when the walk ends
    uint64_t n_frames;          // frames found, the failing one included
    uint64_t n_complete;        // frames whose walk reached the EndMark
};

// on_frame(uint64_t start) is called for every frame found, the failing one included: it is in[start, len).
template <class OnFrame>
LZF_SCAN_HD inline StreamWalk walk_frames(const uint8_t* in, uint64_t len, OnFrame&& on_frame) {
    StreamWalk s{OK, 0, 0, 0};
    uint64_t pos = 0;
    while (pos < len) {
        on_frame(pos);
        ++s.n_frames;
        const Header h = read_header(in + pos, len - pos);
        if (h.status != OK) { s.status = h.status; pos += h.consumed; break; }
        const Walk w = walk_blocks(in + pos, len - pos, h, [](const Block&) {});
        pos += w.consumed;
        if (w.status != OK) { s.status = w.status; break; }
        ++s.n_complete;
    }
    s.consumed = pos;
    return s;
}

}  // namespace lzf_scan

#endif  // LZF_STREAM_WALK_H
