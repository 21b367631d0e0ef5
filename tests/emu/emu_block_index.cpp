// emu_block_index.cpp — TEST INFRASTRUCTURE: the rules of the block index of a frame (rust-lz-fear_amd/csrc/lzf_block_index.h)
// compiled with g++ for the CPU tests of tests/test_block_index_cpu.py, applied block by block by a serial driver in rounds of
// 64: what lzf_frame_block_index_kernel does with the delivery body's decisions, one lane per block.  The stop rules themselves
// are NOT run here: they are frame_deliver_body.inc's, device code, and which block stops the reader is an input of this driver.
// The body's index-mode control flow (the rounds going on behind the stop, the stopping lane's offset, the carried length) is
// covered by the GPU tests (tests/test_gpu_block_index.py) alone.  The product never loads it.
#include <cstdint>
#include "../../rust-lz-fear_amd/csrc/lzf_block_index.h"
#include "../../rust-lz-fear_amd/csrc/lzf_stream_index.h"

extern "C" {

// blk[8k ..]: in_off, in_len, stored, has_sum, want_sum, the block's own status, its decoded length, whether the delivery's rules
// stop the reader at it if nothing did before (the caller's decision: the rules themselves are the delivery body's) — of block k.
// Writes min(n, cap) entries; res[0..2): the frame's out_len (the sum in front of the first stop), the stopping block or n.
void lzf_emu_block_index(const uint64_t* blk, uint64_t n, uint64_t bmax, int linked, lzf_frame_block* out, uint64_t cap, uint64_t* res) {
    uint64_t w = 0, stop_at = n;
    bool stopped = false;
    for (uint64_t base = 0; base < n; base += 64) {
        // the round as the wavefront sees it: every lane's place behind the running offset, the first lane that stops
        uint64_t at[64], run = w;
        uint32_t first = 64;
        const uint64_t lanes = n - base < 64 ? n - base : 64;
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint64_t* b = blk + 8 * (base + l);
            at[l] = run; run += b[6];
            if (first == 64 && b[7]) first = l;
        }
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint64_t* b = blk + 8 * (base + l);
            const lzf_bindex::Place place = lzf_bindex::place_of(stopped, l, first);
            if (base + l < cap)
                out[base + l] = lzf_bindex::fill_entry(b[0], (uint32_t)b[1], b[2] != 0, b[3] != 0, (uint32_t)b[4], linked != 0, bmax, (int)(int64_t)b[5], b[6],
                                                       at[l], stopped ? w : first < 64 ? at[first] : 0, place);
        }
        if (stopped) continue;
        if (first < 64) { w = at[first]; stopped = true; stop_at = base + first; }
        else w = run;
    }
    res[0] = w; res[1] = stop_at;
}

int lzf_emu_check_run(const lzf_frame_block* e, uint64_t count, uint64_t frame_len) { return (int)lzf_bindex::check_run(e, count, frame_len); }
uint64_t lzf_emu_run_total(const lzf_frame_block* e, uint64_t count) { return lzf_bindex::run_total(e, count); }

void lzf_emu_block_locate(const lzf_frame_block* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count) {
    lzf_bindex::locate(index, n, a, b, first, count);
}
// the stream locate through the header the block locate shares with it
void lzf_emu_stream_locate2(const lzf_stream_frame* index, uint64_t n, uint64_t a, uint64_t b, uint64_t* first, uint64_t* count) {
    lzf_sindex::locate(index, n, a, b, first, count);
}

}
