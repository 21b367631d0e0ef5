// emu_frame_layout.cpp — TEST INFRASTRUCTURE: the frame layout rule of the device compressor (rust-lz-fear_amd/csrc/lzf_frame_layout.h)
// compiled with g++ for the CPU tests of tests/test_device_compress_cpu.py.  The product never loads it.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../rust-lz-fear_amd/csrc/lzf_frame_layout.h"

extern "C" {
// One frame from block results, the way the assembly kernel places it: status[i] / out_len[i] = block i's job result, raw_len[i]
// its length, comp[i] / raw[i] its compressed and raw bytes, sums[i] its checksum, `content` the content checksum.  Writes the
// frame to out, its length to *frame_len and block i's length word position to pos[i]; returns the frame's status.
int lzf_emu_frame_layout(const lzf_settings* s, uint32_t nb, const int32_t* status, const uint64_t* out_len, const uint32_t* raw_len,
                         const uint8_t* const* comp, const uint8_t* const* raw, const uint32_t* sums, uint32_t content,
                         uint8_t* out, uint64_t* frame_len, uint64_t* pos) {
    *frame_len = 0;
    uint8_t bd = 0;
    const int rc = lzf_layout::bd_new(s->block_size, &bd);
    if (rc != LZF_OK) return rc;
    uint8_t hdr[lzf_layout::kMaxHeader];
    const uint32_t hdr_len = (uint32_t)lzf_layout::write_header(s, bd, hdr);
    std::vector<lzf_layout::Block> b(nb);
    for (uint32_t i = 0; i < nb; ++i) b[i] = lzf_layout::block_of(status[i], out_len[i], raw_len[i]);
    std::vector<uint64_t> sum_at(nb, 0);
    uint64_t end_at = 0, content_at = 0;
    int st = LZF_OK;
    const bool bsum = s->block_checksums != 0, csum = s->content_checksum != 0;
    const uint64_t n = lzf_layout::lay_out(hdr_len, nb, b.data(), bsum, csum, pos, sum_at.data(), &end_at, &content_at, &st);
    if (st != LZF_OK) return st;
    memcpy(out, hdr, hdr_len);
    for (uint32_t i = 0; i < nb; ++i) {
        lzf_layout::wr32(out + pos[i], lzf_layout::size_word(b[i]));
        memcpy(out + pos[i] + 4, b[i].stored ? raw[i] : comp[i], b[i].len);
        if (bsum) lzf_layout::wr32(out + sum_at[i], sums[i]);
    }
    lzf_layout::wr32(out + end_at, 0);
    if (csum) lzf_layout::wr32(out + content_at, content);
    *frame_len = n;
    return LZF_OK;
}
}
