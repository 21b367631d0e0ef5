// emu_frame_resume.cpp — TEST INFRASTRUCTURE: rust-lz-fear_amd/csrc/lzf_frame_resume_rules.h, the rules of lzf_frame_resume_device that
// the kernels and the host share, compiled with g++ as plain functions over host memory.  tests/test_frame_resume_cases_cpu.py
// drives them call by call and compares them with the Python model of tests/frame_resume_cases.py.  The product never loads it.
#include <cstddef>
#include <cstring>
#include "../../rust-lz-fear_amd/csrc/lzf_frame_resume_rules.h"

using namespace lzf_resume;

extern "C" {

uint64_t lzf_emu_resume_head_bytes(void) { return sizeof(Head); }
uint64_t lzf_emu_resume_cursor_bytes(void) { return CURSOR_BYTES; }
uint64_t lzf_emu_resume_hash_offset(void) { return offsetof(Head, hash); }

// the hash a fresh cursor starts from, for the comparison with lzf_xxh32_reset
void lzf_emu_resume_hash_reset(lzf_xxh32_state* s) { memset(s, 0, sizeof *s); hash_reset(*s); }

// The bounded walk of one call.  blocks: room for `room` entries of {off, len, compressed, want_sum, end_off}; returns the number of
// blocks of the piece.  Reads in[0, in_len) only.
uint64_t lzf_emu_resume_walk(const uint8_t* in, uint64_t in_len, const Head* c, uint64_t out_cap, Piece* piece, uint64_t* blocks, uint64_t room) {
    uint64_t k = 0;
    *piece = walk_piece(in, in_len, *c, out_cap, [&](const lzf_scan::Block& b) {
        if (k < room) { uint64_t* e = blocks + 5 * k; e[0] = b.off; e[1] = b.len; e[2] = b.compressed; e[3] = b.want_sum; e[4] = b.end_off; }
        ++k;
    });
    return k;
}

int lzf_emu_resume_delivers(const Piece* p) { return delivers(*p) ? 1 : 0; }

// The phase transitions: moves the cursor's head, report = {out_len, consumed, status, phase}.
void lzf_emu_resume_settle(Head* c, const Piece* p, int stopped, int32_t stop_status, uint64_t stop_consumed, uint64_t w,
                           const lzf_xxh32_state* hash, uint32_t digest, uint64_t* report) {
    const Report r = settle(*c, *p, stopped != 0, stop_status, stop_consumed, w, *hash, digest);
    report[0] = r.out_len; report[1] = r.consumed; report[2] = (uint64_t)(int64_t)r.status; report[3] = r.phase;
}

// The window update: plan = {keep, take, new_len}.
void lzf_emu_resume_window(uint32_t old_len, uint64_t w, uint32_t* plan) {
    const WindowPlan q = window_plan(old_len, w);
    plan[0] = q.keep; plan[1] = q.take; plan[2] = q.new_len;
}
uint32_t lzf_emu_resume_dict_window(uint64_t dict_len) { return dict_window(dict_len); }

}  // extern "C"
