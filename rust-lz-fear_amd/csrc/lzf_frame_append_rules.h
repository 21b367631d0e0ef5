// lzf_frame_append_rules.h — the rules of lzf_frame_append_device (include/lzfear_frame.h, "streaming frame writer in device
// memory") as __host__ __device__ code: one definition for the host plan and the kernels (frame_device_append.hip) and for the
// CPU tests, which compile this header with g++ and hold it to a Python model of the rule on every case
// (tests/test_frame_append_cases_cpu.py).
//
//   Head          the fixed part of a cursor: what a frame carries from call to call beside its window and its table
//   cut_offer     WHAT IS TAKEN: from in_len, flags, out_cap and the block size alone (the host's half of the rule: it never
//                 reads a cursor) — the reference's cut of the input (src/framed/compress.rs:221-231: whole blocks, a shorter
//                 last one only at the end of the stream) and the longest run of those blocks whose frame bound fits out_cap
//   first_window  what block 0 and block 1 of a linked call stand behind and which table.offset is due before them (:271-275
//                 carried across the call boundary): the device's half, it needs the cursor
//   settle        the cursor after the call and what the call reports
#ifndef LZF_FRAME_APPEND_RULES_H
#define LZF_FRAME_APPEND_RULES_H

#include <stdint.h>
#include "../../include/lzfear_hip.h"
#include "lzf_frame_scan.h"

namespace lzf_append {

constexpr uint32_t MORE = 0u, NEED_INPUT = 1u, DONE = 2u;       // LZF_APPEND_* of include/lzfear_frame.h
constexpr uint32_t FINISH = 1u;                                 // LZF_APPEND_FINISH
constexpr uint32_t WINDOW = 65536u;                             // framed/mod.rs:20
constexpr int32_t OK = 0, OUT_CAPACITY = 7;                     // LZF_OK, LZF_OUT_CAPACITY

// The fixed part of a cursor; the window (64 KiB) and the stream's lzf_u32_table stand behind it.  All zero = nothing written
// yet: no header out, phase MORE, an empty window, a table as U32Table::default().
struct Head {
    uint32_t phase;             // MORE / NEED_INPUT / DONE as last stored; DONE is sticky
    uint32_t header_out;        // 1: the frame's header is written, the hash state below is valid
    int32_t  status;            // sticky with DONE
    uint32_t win_len;           // linked frames: the window is the first win_len bytes of the window buffer
    uint64_t taken;             // bytes taken so far
    uint64_t pending;           // linked frames: the table.offset(forget) due before the next block (:271-275)
    lzf_xxh32_state hash;       // the content hash of the bytes taken so far
    uint64_t pad[6];
};
static_assert(sizeof(Head) == 128, "write cursor head");
constexpr uint64_t WINDOW_OFF = 256u;
constexpr uint64_t TABLE_OFF = WINDOW_OFF + WINDOW;
constexpr uint64_t CURSOR_BYTES = TABLE_OFF + ((sizeof(lzf_u32_table) + 255u) & ~(uint64_t)255u);

// lzf_xxh32_reset(st, 0): the hash a cursor starts from
LZF_SCAN_HD inline void hash_reset(lzf_xxh32_state& s) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u;
    s.v[0] = P1 + P2; s.v[1] = P2; s.v[2] = 0u; s.v[3] = 0u - P1;
    for (int i = 0; i < 16; ++i) s.buf[i] = 0;
    s.fill = 0; s.seed = 0; s.total = 0;
}

// lzf_frame_compress_bound(s, t) for a block size bs >= 1: header, EndMark and checksum words always counted
LZF_SCAN_HD inline uint64_t frame_bound(uint64_t bs, uint64_t t) { return 19u + t + (t / bs + 1u) * 8u + 8u; }

// how the host's half of the rule ends
enum : uint32_t {
    END_BAD_BLOCK_SIZE = 0,     // rule 2: the frame becomes DONE with `status`
    END_NO_ROOM = 1,            // rule 4: LZF_OUT_CAPACITY, phase MORE, the cursor untouched
    END_NO_BLOCK = 2,           // rule 5: less than one block offered without FINISH: NEED_INPUT, the cursor untouched
    END_MORE = 3,               // blocks taken, a block was left for lack of room
    END_NEED_INPUT = 4,         // blocks taken, a part-block or nothing is left
    END_FINISH = 5              // FINISH and the whole offer taken (possibly no byte): EndMark and content checksum follow
};
struct Offer { uint64_t taken; uint32_t n_blocks; uint32_t end; int32_t status; uint32_t pad; };
static_assert(sizeof(Offer) == 24, "offer");
LZF_SCAN_HD inline bool takes(const Offer& o) { return o.end >= END_MORE; }       // its blocks are compressed, its bytes written

// What is taken.  bd_status: what BlockDescriptor::new says of the block size (LZF_OK, or rule 2's status).
LZF_SCAN_HD inline Offer cut_offer(int32_t bd_status, uint64_t bs, uint64_t in_len, uint32_t flags, uint64_t out_cap) {
    if (bd_status != OK) return Offer{0, 0, END_BAD_BLOCK_SIZE, bd_status, 0};
    const bool finish = (flags & FINISH) != 0;
    const uint64_t whole = in_len / bs, rest = in_len % bs;
    const uint64_t offered = whole + (finish && rest ? 1u : 0u);
    if (!offered) {
        if (!finish) return Offer{0, 0, END_NO_BLOCK, OK, 0};
        return out_cap < frame_bound(bs, 0) ? Offer{0, 0, END_NO_ROOM, OUT_CAPACITY, 0} : Offer{0, 0, END_FINISH, OK, 0};
    }
    // whole blocks: frame_bound(bs, k * bs) = 27 + k * bs + (k + 1) * 8 <= out_cap
    uint64_t k = out_cap < 35u ? 0u : (out_cap - 35u) / (bs + 8u);
    if (k > whole) k = whole;
    uint64_t t = k * bs;
    if (k == whole && offered > whole && frame_bound(bs, in_len) <= out_cap) { ++k; t = in_len; }
    if (!k) return Offer{0, 0, END_NO_ROOM, OUT_CAPACITY, 0};
    if (k > 0x7FFFFFFFull) { k = 0x7FFFFFFFull; t = k * bs; }     // (more blocks than a launch takes: the rest next time)
    return Offer{t, (uint32_t)k, k < offered ? END_MORE : finish ? END_FINISH : END_NEED_INPUT, OK, 0};
}

// Linked frames: the history block 0 of a call stands behind (a cursor without a header out: the whole dictionary; otherwise the
// cursor's window), the table.offset due before block 0 (what the cursor carried) and before block 1 (what block 0 makes the
// window forget).  From block 1 on the history is the last 64 KiB of the caller's input, from block 2 on the offset is the block
// size: the host knows those.  A DONE cursor's blocks are compressed for nothing: no history, no offset.
struct FirstWindow { uint64_t hist, add0, add1; };
LZF_SCAN_HD inline FirstWindow first_window(const Head& c, uint64_t dict_len, uint64_t n0) {
    if (c.phase == DONE) return FirstWindow{0, 0, 0};
    const uint64_t hist = c.header_out ? (c.win_len < WINDOW ? c.win_len : WINDOW) : dict_len;      // (never more than the scratch in front of block 0)
    return FirstWindow{hist, c.header_out ? c.pending : 0u, hist + n0 > WINDOW ? hist + n0 - WINDOW : 0u};
}
// The table.offset the cursor carries into the next call, behind a call that took n_blocks >= 1 blocks (the last one n_last
// bytes), block 0 behind `hist` bytes: compress.rs:271-275 for the last block of the call.
LZF_SCAN_HD inline uint64_t pending_after(uint64_t hist, uint32_t n_blocks, uint64_t n_last) {
    const uint64_t before = n_blocks == 1 ? hist : WINDOW;      // (bs >= 64 KiB: behind a whole block the window is full)
    return before + n_last > WINDOW ? before + n_last - WINDOW : 0u;
}

// What a call reports for a frame.
struct Report { uint64_t out_len, taken; int32_t status; uint32_t phase; uint32_t writes, header; };
// The cursor after the call, and the report.  block_status: the first status in block order that is neither LZF_OK nor
// LZF_OUTPUT_FULL (LZF_OK: none); body: the bytes of the taken blocks in the frame (length words, payloads, block checksums);
// header_len / tail_len: the header's and the EndMark's (with the content checksum's) bytes; n_last: the last taken block's
// length; linked: the frame's blocks are linked.  `writes`: bytes of this call go out; `header`: the header is among them.
LZF_SCAN_HD inline Report settle(Head& c, const Offer& o, int32_t block_status, uint64_t body, uint32_t header_len, uint32_t tail_len,
                                 bool linked, uint64_t dict_len, uint64_t bs, uint64_t n_last) {
    if (c.phase == DONE) return Report{0, 0, c.status, DONE, 0, 0};                          // rule 1
    if (o.end == END_BAD_BLOCK_SIZE) { c.phase = DONE; c.status = o.status; return Report{0, 0, o.status, DONE, 0, 0}; }   // rule 2
    if (o.end == END_NO_ROOM) return Report{0, 0, OUT_CAPACITY, MORE, 0, 0};                // rule 4
    if (o.end == END_NO_BLOCK) return Report{0, 0, OK, NEED_INPUT, 0, 0};                   // rule 5
    if (block_status != OK) { c.phase = DONE; c.status = block_status; return Report{0, 0, block_status, DONE, 0, 0}; }    // rule 7
    const uint32_t header = c.header_out ? 0u : 1u;
    Report r{(header ? header_len : 0u) + body + (o.end == END_FINISH ? tail_len : 0u), o.taken, OK,
             o.end == END_MORE ? MORE : o.end == END_NEED_INPUT ? NEED_INPUT : DONE, 1u, header};
    if (linked && o.n_blocks) {
        const FirstWindow w = first_window(c, dict_len, o.n_blocks == 1 ? n_last : bs);
        c.pending = pending_after(w.hist, o.n_blocks, n_last);
        c.win_len = o.taken < WINDOW ? (uint32_t)o.taken : WINDOW;     // rule 8 (a frame that goes on took a whole block: a full window)
    }
    c.header_out = 1; c.taken += o.taken; c.phase = r.phase; c.status = OK;
    return r;
}

}  // namespace lzf_append

#endif  // LZF_FRAME_APPEND_RULES_H
