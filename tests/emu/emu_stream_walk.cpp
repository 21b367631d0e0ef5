// emu_stream_walk.cpp — TEST INFRASTRUCTURE: the frame-to-frame walk of the device stream scan
// (rust-lz-fear_amd/csrc/lzf_stream_walk.h) compiled with g++ for the CPU tests of tests/test_stream_frames_cpu.py.
// The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_stream_walk.h"

extern "C" {
// out[0..4): status, consumed, frames found, frames that reached their EndMark; then the frames' start offsets, at most
// max_frames of them
int lzf_emu_stream_walk(const uint8_t* in, uint64_t in_len, uint64_t* out, uint64_t max_frames) {
    uint64_t k = 0;
    const lzf_scan::StreamWalk w = lzf_scan::walk_frames(in, in_len, [&](uint64_t at) { if (k < max_frames) out[4 + k] = at; ++k; });
    out[0] = (uint64_t)w.status; out[1] = w.consumed; out[2] = w.n_frames; out[3] = w.n_complete;
    return w.status;
}
}
