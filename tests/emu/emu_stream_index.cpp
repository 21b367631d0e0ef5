// emu_stream_index.cpp — TEST INFRASTRUCTURE: the rules of the stream frame index (rust-lz-fear_amd/csrc/lzf_stream_index.h)
// compiled with g++ for the CPU tests of tests/test_stream_index_cpu.py, applied frame by frame by a serial driver: what
// lzf_stream_index_kernel does 64 frames per round.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_stream_walk.h"
#include "../../rust-lz-fear_amd/csrc/lzf_stream_index.h"

extern "C" {

// The stream as the device's scans see it.  Per frame the walk finds, at most max_frames of them: w[3k] = its start, w[3k + 1] =
// where its structural walk ended if that reached the EndMark without error (~0 otherwise), w[3k + 2] = 0x100 | FLG if its
// header parsed (0 otherwise).  Returns the number of frames found.
uint64_t lzf_emu_index_walk(const uint8_t* in, uint64_t len, uint64_t* w, uint64_t max_frames) {
    uint64_t k = 0;
    lzf_scan::walk_frames(in, len, [&](uint64_t at) {
        if (k < max_frames) {
            const lzf_scan::Header h = lzf_scan::read_header(in + at, len - at);
            uint64_t full = ~0ull, flags = 0;
            if (h.status == lzf_scan::OK) {
                const lzf_scan::Walk wk = lzf_scan::walk_blocks(in + at, len - at, h, [](const lzf_scan::Block&) {});
                flags = 0x100u | h.flags;
                if (wk.status == lzf_scan::OK) full = wk.consumed;
            }
            w[3 * k] = at; w[3 * k + 1] = full; w[3 * k + 2] = flags;
        }
        ++k;
    });
    return k;
}

// fr[6k ..]: in_off, status, out_len, consumed, full, header flags (as above) of frame k.  Writes min(n, cap) entries and the
// stream's results res[0..4): status, out_len, consumed, frames that ended at their EndMark with LZF_OK in front of the stop.
void lzf_emu_stream_index(const uint8_t* in, const uint64_t* fr, uint64_t n, lzf_stream_frame* out, uint64_t cap, uint64_t* res) {
    uint64_t run = 0, pos = 0, good = 0;
    int status = 0;
    bool stopped = false;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t* f = fr + 6 * k;
        const int code = (int)(int64_t)f[1];
        const bool ends = lzf_sindex::ends_stream(code, f[3], f[4]);
        if (k < cap) out[k] = lzf_sindex::fill_entry(in + f[0], (f[5] & 0x100u) != 0, (uint32_t)f[5], f[0], code, f[2], f[3], f[4], run, stopped);
        if (stopped) continue;
        run += f[2]; pos += f[3];
        if (ends) { status = code; stopped = true; } else ++good;
    }
    res[0] = (uint64_t)(int64_t)status; res[1] = run; res[2] = pos; res[3] = good;
}

void lzf_emu_stream_locate(const lzf_stream_frame* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count) {
    lzf_sindex::locate(index, n, a, b, first, count);
}

}
