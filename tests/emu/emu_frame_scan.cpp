// emu_frame_scan.cpp — TEST INFRASTRUCTURE: the device frame scan (rust-lz-fear_amd/csrc/lzf_frame_scan.h) compiled with g++
// for the CPU tests of tests/test_frame_scan_cpu.py.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_frame_scan.h"

extern "C" {
// out[0..7): header status, header consumed, walk status, walk consumed, endmark, want_content, blocks found;
// then 5 words per block (off, len, compressed, want_sum, end_off), at most max_blocks of them
int lzf_emu_frame_scan(const uint8_t* in, uint64_t in_len, uint64_t* out, uint64_t max_blocks) {
    const lzf_scan::Header h = lzf_scan::read_header(in, in_len);
    out[0] = (uint64_t)h.status; out[1] = h.consumed;
    for (int i = 2; i < 7; ++i) out[i] = 0;
    if (h.status != lzf_scan::OK) return h.status;
    uint64_t k = 0;
    const lzf_scan::Walk w = lzf_scan::walk_blocks(in, in_len, h, [&](const lzf_scan::Block& b) {
        if (k < max_blocks) { uint64_t* e = out + 7 + 5 * k; e[0] = b.off; e[1] = b.len; e[2] = b.compressed; e[3] = b.want_sum; e[4] = b.end_off; }
        ++k;
    });
    out[2] = (uint64_t)w.status; out[3] = w.consumed; out[4] = w.endmark; out[5] = w.want_content; out[6] = k;
    return w.status;
}
}
