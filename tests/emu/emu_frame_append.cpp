// emu_frame_append.cpp — TEST INFRASTRUCTURE: rust-lz-fear_amd/csrc/lzf_frame_append_rules.h, the rules of lzf_frame_append_device that
// the host plan and the kernels share, compiled with g++ as plain functions over host memory.  tests/test_frame_append_cases_cpu.py
// drives them call by call and compares them with the Python model of tests/frame_append_cases.py.  The product never loads it.
#include <cstddef>
#include <cstring>
#include "../../rust-lz-fear_amd/csrc/lzf_frame_append_rules.h"

using namespace lzf_append;

extern "C" {

uint64_t lzf_emu_append_head_bytes(void) { return sizeof(Head); }
uint64_t lzf_emu_append_cursor_bytes(void) { return CURSOR_BYTES; }
uint64_t lzf_emu_append_hash_offset(void) { return offsetof(Head, hash); }
uint64_t lzf_emu_append_bound(uint64_t bs, uint64_t t) { return frame_bound(bs, t); }
void lzf_emu_append_hash_reset(lzf_xxh32_state* s) { memset(s, 0, sizeof *s); hash_reset(*s); }

// what is taken: offer = {taken, n_blocks, end, status}
void lzf_emu_append_cut(int32_t bd_status, uint64_t bs, uint64_t in_len, uint32_t flags, uint64_t out_cap, uint64_t* offer) {
    const Offer o = cut_offer(bd_status, bs, in_len, flags, out_cap);
    offer[0] = o.taken; offer[1] = o.n_blocks; offer[2] = o.end; offer[3] = (uint64_t)(int64_t)o.status;
}

// what block 0 and block 1 of a linked call stand behind: w = {hist, add0, add1}
void lzf_emu_append_first_window(const Head* c, uint64_t dict_len, uint64_t n0, uint64_t* w) {
    const FirstWindow f = first_window(*c, dict_len, n0);
    w[0] = f.hist; w[1] = f.add0; w[2] = f.add1;
}

// the cursor after the call: report = {out_len, taken, status, phase, writes, header}
void lzf_emu_append_settle(Head* c, const uint64_t* offer, int32_t block_status, uint64_t body, uint32_t header_len, uint32_t tail_len,
                           int linked, uint64_t dict_len, uint64_t bs, uint64_t n_last, uint64_t* report) {
    const Offer o{offer[0], (uint32_t)offer[1], (uint32_t)offer[2], (int32_t)(int64_t)offer[3], 0};
    const Report r = settle(*c, o, block_status, body, header_len, tail_len, linked != 0, dict_len, bs, n_last);
    report[0] = r.out_len; report[1] = r.taken; report[2] = (uint64_t)(int64_t)r.status; report[3] = r.phase; report[4] = r.writes; report[5] = r.header;
}

}  // extern "C"
