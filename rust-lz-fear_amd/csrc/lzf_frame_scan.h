// lzf_frame_scan.h — the header parse and the block walk of lz-fear's LZ4FrameReader as __host__ __device__ code.
//
//   read_header   LZ4FrameReader::new, src/framed/decompress.rs:102-161 (header.rs:29-81 for FLG / BD)
//   walk_blocks   the u32 length hops of decode_block, src/framed/decompress.rs:198-235
//
// This is the frame layer's only walk.  The device frame layer (frame_device_scan.hip) runs it in its scan kernels, one lane per
// frame; the host driver (frame.cpp) runs it over the caller's bytes: lzf_frame_read_header and lzf_frame_decompress_many through
// both, the block-by-block reader through a walk_blocks that stops behind its one block.  The CPU tests compile this header with g++
// (tests/emu/emu_frame_scan.cpp) and hold it to the reference's statuses and `consumed` on the decode corpus.  No
// alignment is assumed: frames start anywhere, every multi-byte field is read bytewise.  Status codes are those of
// include/lzfear_frame.h.
#ifndef LZF_FRAME_SCAN_H
#define LZF_FRAME_SCAN_H

#include <stdint.h>
#include <type_traits>

#if defined(__HIPCC__) || defined(__HIP__)
#define LZF_SCAN_HD __host__ __device__
#else
#define LZF_SCAN_HD
#endif

namespace lzf_scan {

enum : int {
    OK = 0, INPUT_ERROR = 16, WRONG_MAGIC = 17, HEADER_CHECKSUM_FAIL = 18, BLOCK_SIZE_OVERFLOW = 22,
    UNIMPLEMENTED_BLOCKSIZE = 23, UNSUPPORTED_VERSION = 24, RESERVED_FLAG_BITS = 25, RESERVED_BD_BITS = 26
};
constexpr uint32_t MAGIC = 0x184D2204u;                 // framed/mod.rs:16
constexpr uint32_t INCOMPRESSIBLE = 0x80000000u;        // framed/mod.rs:18
constexpr uint8_t FL_INDEP = 0x20, FL_BLOCKSUM = 0x10, FL_CSIZE = 0x08, FL_CSUM = 0x04, FL_DICTID = 0x01;   // header.rs:8-16

LZF_SCAN_HD inline uint32_t rd32(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
LZF_SCAN_HD inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 (seed 0) of fewer than 16 bytes: the header checksum covers FLG, BD, content size and dictionary id, 14 bytes at most
LZF_SCAN_HD inline uint32_t xxh32_short(const uint8_t* p, uint32_t n) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
    uint32_t h = P5 + n;
    for (; n >= 4; p += 4, n -= 4) h = rotl(h + rd32(p) * P3, 17) * P4;
    for (; n; ++p, --n) h = rotl(h + (uint32_t)(*p) * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

struct Header {
    int status;                 // OK or the header error
    uint64_t consumed;          // bytes read when the reader stops (the whole header when it parses)
    uint32_t header_len;
    uint8_t flags, bd;
    uint64_t block_maxsize;
};

// decompress.rs:102-161: magic, FLG (version, reserved bit), BD (reserved bits), content size, dictionary id, HC, block size.
// On truncation the reader has read everything there was (consumed = in_len).
LZF_SCAN_HD inline Header read_header(const uint8_t* in, uint64_t in_len) {
    Header h{OK, 0, 0, 0, 0, 0};
    uint64_t r = 0;
#define LZF_SCAN_NEED(n) if (in_len - r < (uint64_t)(n)) { h.status = INPUT_ERROR; h.consumed = in_len; return h; }
#define LZF_SCAN_FAIL(c) { h.status = (c); h.consumed = r; return h; }
    LZF_SCAN_NEED(4); r = 4;
    if (rd32(in) != MAGIC) LZF_SCAN_FAIL(WRONG_MAGIC);                // :103-106
    LZF_SCAN_NEED(1); const uint8_t flg = in[r++];
    if ((flg >> 6) != 1) LZF_SCAN_FAIL(UNSUPPORTED_VERSION);          // header.rs:33-36
    if (flg & 0x02) LZF_SCAN_FAIL(RESERVED_FLAG_BITS);                // header.rs:37-39
    LZF_SCAN_NEED(1); const uint8_t bd = in[r++];
    if (bd & 0x8F) LZF_SCAN_FAIL(RESERVED_BD_BITS);                   // header.rs:66-68
    h.flags = flg; h.bd = bd;
    if (flg & FL_CSIZE) { LZF_SCAN_NEED(8); r += 8; }                 // :111-118
    if (flg & FL_DICTID) { LZF_SCAN_NEED(4); r += 4; }                // :119-126
    LZF_SCAN_NEED(1); const uint8_t hc = in[r++];
    if (hc != (uint8_t)(xxh32_short(in + 4, (uint32_t)(r - 5)) >> 8)) LZF_SCAN_FAIL(HEADER_CHECKSUM_FAIL);   // :132-136
    const unsigned size = (bd >> 4) & 7;
    if (size < 4) LZF_SCAN_FAIL(UNIMPLEMENTED_BLOCKSIZE);             // :153, header.rs:73-80
#undef LZF_SCAN_NEED
#undef LZF_SCAN_FAIL
    h.block_maxsize = 1ull << (size * 2 + 8);
    h.header_len = (uint32_t)r;
    h.consumed = r;
    return h;
}

// One block as the walk finds it: its bytes are in[off, off + len); end_off = input read once its checksum word is.
struct Block { uint64_t off; uint32_t len; uint32_t compressed; uint32_t want_sum; uint64_t end_off; };
struct Walk {
    int status;                 // OK, INPUT_ERROR or BLOCK_SIZE_OVERFLOW: the structural error that ends the walk
    uint64_t consumed;          // bytes read when the walk ends
    bool endmark;               // the EndMark (and the content checksum word, if the frame has one) was read
    uint32_t want_content;
};

// decompress.rs:205-235: length word (EndMark and content checksum word :206-215, stored bit :217-218, bl > block_maxsize
// :220-222), payload (:224-226), block checksum word (:228-230).  on_block(const Block&) is called for every block found; one
// that returns bool ends the walk behind the block for which it returns false (status OK, no EndMark, consumed = the block's
// end_off): the block-by-block reader takes its one block so.  The walk starts at h.header_len and reads h.flags and
// h.block_maxsize, nothing else of the header.
template <class OnBlock>
LZF_SCAN_HD inline Walk walk_blocks(const uint8_t* in, uint64_t in_len, const Header& h, OnBlock&& on_block) {
    Walk w{OK, 0, false, 0};
    const bool bsum = (h.flags & FL_BLOCKSUM) != 0, csum = (h.flags & FL_CSUM) != 0;
    uint64_t r = h.header_len;
    for (;;) {
        if (in_len - r < 4) { w.status = INPUT_ERROR; r = in_len; break; }
        uint32_t bl = rd32(in + r); r += 4;
        if (bl == 0) {
            if (csum) { if (in_len - r < 4) { w.status = INPUT_ERROR; r = in_len; break; } w.want_content = rd32(in + r); r += 4; }
            w.endmark = true; break;
        }
        const uint32_t compressed = (bl & INCOMPRESSIBLE) == 0 ? 1u : 0u; bl &= ~INCOMPRESSIBLE;
        if ((uint64_t)bl > h.block_maxsize) { w.status = BLOCK_SIZE_OVERFLOW; break; }
        if (in_len - r < bl) { w.status = INPUT_ERROR; r = in_len; break; }
        Block b{r, bl, compressed, 0u, 0u};
        r += bl;
        if (bsum) {
            if (in_len - r < 4) { w.status = INPUT_ERROR; r = in_len; break; }
            b.want_sum = rd32(in + r); r += 4;
        }
        b.end_off = r;
        if constexpr (std::is_same<decltype(on_block(b)), bool>::value) { if (!on_block(b)) break; }
        else on_block(b);
    }
    w.consumed = r;
    return w;
}

// the most a block of `len` compressed bytes can decode to: every byte a 255-run length byte (raw/decompress.rs:40-56)
LZF_SCAN_HD inline uint64_t block_out_bound(uint64_t bmax, uint64_t len) { const uint64_t e = 255 * len + 16; return e < bmax ? e : bmax; }

}  // namespace lzf_scan

#endif  // LZF_FRAME_SCAN_H
