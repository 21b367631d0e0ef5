// lzf_frame_layout.h — how a compressed frame is laid out (src/framed/compress.rs:160-282), shared by the frame compressors.
//
//   bd_new         BlockDescriptor::new, src/framed/header.rs:53-62
//   write_header   compress.rs:163-200: magic, FLG, BD, [content size], [dictionary id], HC
//   block_of / block_span / size_word / tail_len
//                  the block loop (:221-276) and the end (:277-281) once the blocks are compressed: a block whose writer
//                  refused (LZF_OUTPUT_FULL) is stored raw (:250-255), any other status but LZF_OK fails the frame; block i
//                  takes 4 + payload + [4] bytes, the EndMark and the optional content checksum follow the last one.
//
// lzf_frame_compress_many (frame.cpp) places frames on the host with block_of and lay_out; lzf_frame_compress_device_many
// (frame_device_compress.hip) runs the same rule in its assembly kernel, one wavefront per frame (a wave-wide exclusive scan of
// block_span).  The CPU tests compile this header with g++ (tests/emu/emu_frame_layout.cpp) and hold lay_out below to
// lzf_frame_assemble's bytes.
#ifndef LZF_FRAME_LAYOUT_H
#define LZF_FRAME_LAYOUT_H

#include <stddef.h>
#include <stdint.h>
#include "lzf_frame_scan.h"
#include "../../include/lzfear_frame.h"

namespace lzf_layout {

using lzf_scan::FL_INDEP; using lzf_scan::FL_BLOCKSUM; using lzf_scan::FL_CSIZE; using lzf_scan::FL_CSUM; using lzf_scan::FL_DICTID;
using lzf_scan::INCOMPRESSIBLE;
constexpr uint32_t kMaxHeader = 19;                     // 4 magic + FLG + BD + 8 content size + 4 dictionary id + HC

LZF_SCAN_HD inline void wr32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// header.rs:53-62 BlockDescriptor::new
inline int bd_new(uint64_t maxsize, uint8_t* bd) {
    unsigned tz = maxsize ? (unsigned)__builtin_ctzll(maxsize) : 64;
    unsigned maybe = ((tz > 8 ? tz - 8 : 0) / 2) & 0xFF;
    uint8_t b = (uint8_t)(maybe << 4);
    if (b & 0x8F) return LZF_F_PANIC;                           // :55 parse(..).unwrap()
    unsigned size = (b >> 4) & 7;
    if (size < 4 || (1ull << (size * 2 + 8)) != maxsize) return LZF_F_INVALID_BLOCK_SIZE;
    *bd = b;
    return LZF_OK;
}

// compress.rs:163-200: magic, FLG, BD, [content size], [dict id], HC (XXH32 of FLG .. dict id, 14 bytes at most)
inline size_t write_header(const lzf_settings* s, uint8_t bd, uint8_t* out) {
    uint8_t flags = 0;
    if (s->independent_blocks) flags |= FL_INDEP;
    if (s->block_checksums) flags |= FL_BLOCKSUM;
    if (s->content_checksum) flags |= FL_CSUM;
    if (s->has_dictionary_id) flags |= FL_DICTID;
    if (s->has_content_size) flags |= FL_CSIZE;
    size_t w = 0;
    wr32(out, LZF_MAGIC); w += 4;
    out[w++] = (uint8_t)((1 << 6) | flags);
    out[w++] = bd;
    if (s->has_content_size) { wr32(out + w, (uint32_t)s->content_size); wr32(out + w + 4, (uint32_t)(s->content_size >> 32)); w += 8; }
    if (s->has_dictionary_id) { wr32(out + w, s->dictionary_id); w += 4; }
    const uint8_t hc = (uint8_t)(lzf_scan::xxh32_short(out + 4, (uint32_t)(w - 4)) >> 8);
    out[w++] = hc;
    return w;
}

// A compressed block as it goes into the frame: `len` payload bytes, raw (stored) or LZ4; `bad` = the frame fails with `status`.
struct Block { uint32_t len; bool stored; bool bad; int status; };
// compress.rs:244-255 from the block's job result (status, out_len) and its raw length
LZF_SCAN_HD inline Block block_of(int status, uint64_t out_len, uint32_t raw_len) {
    if (status == LZF_OK) return Block{(uint32_t)out_len, false, false, LZF_OK};
    if (status == LZF_OUTPUT_FULL) return Block{raw_len, true, false, LZF_OK};
    return Block{0u, false, true, status};
}
// bytes block i takes in the frame: length word (:247,:253), payload (:258), block checksum (:259-263)
LZF_SCAN_HD inline uint64_t block_span(uint32_t len, bool bsum) { return 4u + (uint64_t)len + (bsum ? 4u : 0u); }
LZF_SCAN_HD inline uint32_t size_word(const Block& b) { return b.stored ? (b.len | INCOMPRESSIBLE) : b.len; }
// EndMark (:277) and content checksum (:279-281)
LZF_SCAN_HD inline uint64_t tail_len(bool csum) { return 4u + (csum ? 4u : 0u); }

// Where everything goes, one block after the other: the serial form of the assembly kernel's rule.  pos[i] = block i's length
// word; sum_at[i] = its checksum word (bsum); *content_at = the content checksum word (csum).  Returns the frame's length, or 0
// with *status set when a block fails the frame (the first bad block in block order).
LZF_SCAN_HD inline uint64_t lay_out(uint32_t header_len, uint32_t nb, const Block* b, bool bsum, bool csum,
                                    uint64_t* pos, uint64_t* sum_at, uint64_t* end_at, uint64_t* content_at, int* status) {
    *status = LZF_OK;
    for (uint32_t i = 0; i < nb; ++i) if (b[i].bad) { *status = b[i].status; return 0; }
    uint64_t w = header_len;
    for (uint32_t i = 0; i < nb; ++i) {
        pos[i] = w;
        if (bsum) sum_at[i] = w + 4u + b[i].len;
        w += block_span(b[i].len, bsum);
    }
    *end_at = w;
    *content_at = csum ? w + 4u : 0u;
    return w + tail_len(csum);
}

}  // namespace lzf_layout

#endif  // LZF_FRAME_LAYOUT_H
