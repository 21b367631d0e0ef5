// lzf_frame_resume_rules.h — the rules of lzf_frame_resume_device (include/lzfear_frame.h, "resumable decode of frames in device
// memory") as __host__ __device__ code: one definition for the kernels (frame_device_resume.hip) and for the CPU tests, which
// compile this header with g++ and hold it to a Python model of the rule on every case (tests/test_frame_resume_cases_cpu.py).
//
//   Head          the fixed part of a cursor: what a frame carries from call to call beside its window
//   walk_piece    the bounded walk: from the cursor's offset, lzf_frame_scan.h's walk_blocks (the frame layer's only walk) with
//                 the FIT RULE as its on_block — whole blocks while their bounds fit the room given
//   settle        the PHASE TRANSITIONS: the cursor after the call and what the call reports, from the piece, what the delivery
//                 found among its blocks and the content hash's digest
//   window_plan   the WINDOW UPDATE: which bytes of the old window and of the call's output make the new one
//
// The order of the questions a block is asked is the reader's (src/framed/decompress.rs:205-235) with the fit rule last: the
// length word (EndMark, overflow), then the payload and its checksum word (cut off: NEED_INPUT), then the bound against the
// room (MORE).  So a block is weighed only once it is whole, and nothing behind the block that ends the piece is read.
#ifndef LZF_FRAME_RESUME_RULES_H
#define LZF_FRAME_RESUME_RULES_H

#include <stdint.h>
#include "../../include/lzfear_hip.h"
#include "lzf_frame_scan.h"

namespace lzf_resume {

constexpr uint32_t MORE = 0u, NEED_INPUT = 1u, DONE = 2u;       // LZF_RESUME_* of include/lzfear_frame.h
constexpr uint32_t WINDOW = 65536u;                             // framed/mod.rs:20
constexpr int32_t OUT_CAPACITY = 7, FRAME_CHECKSUM_FAIL = 20;   // LZF_OUT_CAPACITY, LZF_F_FRAME_CHECKSUM_FAIL

// The fixed part of a cursor (the two window buffers stand behind it).  All zero = the start of a frame: nothing parsed, phase
// MORE, no bytes delivered.  While nothing has been delivered a linked frame's window is the dictionary's tail and is not
// stored: win_len / win_sel count from the first delivery on.
struct Head {
    uint32_t phase;             // MORE / NEED_INPUT / DONE as last reported; DONE is sticky
    uint32_t parsed;            // 1: the header's fields below and the hash state are valid
    int32_t  status;            // sticky with DONE
    uint32_t header_len;
    uint32_t flags;             // FLG byte
    uint32_t win_len, win_sel;  // linked frames: the window is win_len bytes at the start of buffer win_sel
    uint32_t pad0;
    uint64_t block_maxsize;
    uint64_t in_off;            // input offset of the next unread item
    uint64_t delivered;         // bytes delivered so far
    lzf_xxh32_state hash;       // the content hash of the bytes delivered so far
    uint64_t pad1[3];
};
static_assert(sizeof(Head) == 128, "cursor head");
constexpr uint64_t CURSOR_BYTES = 256u + 2u * WINDOW;           // head (128 bytes used) + two window buffers
constexpr uint64_t WINDOW_OFF = 256u;

// lzf_xxh32_reset(st, 0): the hash a fresh cursor starts from
LZF_SCAN_HD inline void hash_reset(lzf_xxh32_state& s) {
    const uint32_t P1 = 2654435761u, P2 = 2246822519u;
    s.v[0] = P1 + P2; s.v[1] = P2; s.v[2] = 0u; s.v[3] = 0u - P1;
    for (int i = 0; i < 16; ++i) s.buf[i] = 0;
    s.fill = 0; s.seed = 0; s.total = 0;
}

// how a call's walk ended
enum : uint32_t {
    END_MORE = 0,               // in front of a whole block whose bound does not fit what is left of the room
    END_NEED_INPUT = 1,         // in front of a length word, a block or a content checksum word that in_len cuts off
    END_ENDMARK = 2,            // behind the EndMark and the content checksum word
    END_ERROR = 3,              // behind a length word above block_maxsize: `status`
    END_HELD = 4,               // the cursor was DONE: nothing read
    END_HEADER_CUT = 5,         // fresh cursor, in_len ends inside the header: the cursor stays fresh
    END_HEADER_ERROR = 6,       // fresh cursor, the header fails: `status`, stop = the reader's consumed
    END_NO_ROOM = 7             // the very first block of the call does not fit: LZF_OUT_CAPACITY, the cursor untouched
};
// The piece of one call: blocks [0, n_blocks) found from `start` on; `stop` is where the cursor stands behind it unless the
// delivery stops at one of its blocks.  64 bytes: the summary the host reads back (prefix / prefix_len are the kernel's: where a
// linked frame's window stands in device memory for this call).
struct Piece {
    uint32_t end; int32_t status;
    uint32_t flags, header_len;
    uint32_t want_content, prefix_len;
    uint64_t block_maxsize;
    uint64_t start, stop, n_blocks;
    uint64_t prefix;
};
static_assert(sizeof(Piece) == 64, "piece summary");
LZF_SCAN_HD inline bool delivers(const Piece& p) { return p.end <= END_ERROR && p.n_blocks != 0; }   // its blocks go through decode and delivery

// The fit rule's term: lzf_frame_decompress_bound_device's per-block bound.
LZF_SCAN_HD inline uint64_t block_bound(uint64_t bmax, uint32_t len, bool compressed) { return compressed ? lzf_scan::block_out_bound(bmax, len) : len; }

// The bounded walk.  on_block(const lzf_scan::Block&) sees every block of the piece, offsets counted from the frame's start.
template <class OnBlock>
LZF_SCAN_HD inline Piece walk_piece(const uint8_t* in, uint64_t in_len, const Head& c, uint64_t out_cap, OnBlock&& on_block) {
    Piece p{};
    if (c.phase == DONE) { p.end = END_HELD; p.status = c.status; p.start = p.stop = c.in_off; return p; }
    lzf_scan::Header h{lzf_scan::OK, 0, 0, 0, 0, 0};
    if (!c.parsed) {
        h = lzf_scan::read_header(in, in_len);
        if (h.status == lzf_scan::INPUT_ERROR) { p.end = END_HEADER_CUT; return p; }
        if (h.status != lzf_scan::OK) { p.end = END_HEADER_ERROR; p.status = h.status; p.stop = h.consumed; return p; }
    } else { h.flags = (uint8_t)c.flags; h.block_maxsize = c.block_maxsize; h.header_len = c.header_len; }
    const uint64_t base = c.parsed ? c.in_off : h.header_len;
    p.flags = h.flags; p.header_len = h.header_len; p.block_maxsize = h.block_maxsize;
    p.start = p.stop = base;
    if (in_len < base) { p.end = END_NEED_INPUT; return p; }        // (an in_len that shrank: nothing to read)
    lzf_scan::Header from = h;
    from.header_len = 0;                                            // the walk starts at in + base
    uint64_t room = out_cap, last_end = 0;
    bool nofit = false;
    const lzf_scan::Walk w = lzf_scan::walk_blocks(in + base, in_len - base, from, [&](const lzf_scan::Block& b) -> bool {
        const uint64_t bound = block_bound(h.block_maxsize, b.len, b.compressed != 0);
        if (bound > room) { nofit = true; return false; }
        room -= bound; last_end = b.end_off; ++p.n_blocks;
        lzf_scan::Block a = b;
        a.off += base; a.end_off += base;
        on_block(a);
        return true;
    });
    if (nofit) { p.end = p.n_blocks ? END_MORE : END_NO_ROOM; p.stop = base + last_end; }
    else if (w.status == lzf_scan::INPUT_ERROR) { p.end = END_NEED_INPUT; p.stop = base + last_end; }
    else if (w.status != lzf_scan::OK) { p.end = END_ERROR; p.status = w.status; p.stop = base + w.consumed; }
    else { p.end = END_ENDMARK; p.want_content = w.want_content; p.stop = base + w.consumed; }
    return p;
}

// What a call reports for a frame.
struct Report { uint64_t out_len, consumed; int32_t status; uint32_t phase; };

// The phase transitions.  `stopped`: the delivery stopped at a block of the piece (block checksum, codec status, more than
// block_maxsize bytes, the empty block) with stop_status and stop_consumed; `w` the bytes it delivered; `hash` the content hash
// after them and `digest` its digest.  Moves the cursor and says what the call reports.
LZF_SCAN_HD inline Report settle(Head& c, const Piece& p, bool stopped, int32_t stop_status, uint64_t stop_consumed, uint64_t w,
                                 const lzf_xxh32_state& hash, uint32_t digest) {
    switch (p.end) {
    case END_HELD: return Report{0, c.in_off, c.status, DONE};
    case END_HEADER_CUT: return Report{0, 0, lzf_scan::OK, NEED_INPUT};
    case END_NO_ROOM: return Report{0, c.in_off, OUT_CAPACITY, MORE};
    case END_HEADER_ERROR:
        c.phase = DONE; c.status = p.status; c.in_off = p.stop;
        return Report{0, p.stop, p.status, DONE};
    default: break;
    }
    if (!c.parsed) { c.parsed = 1; c.flags = p.flags; c.header_len = p.header_len; c.block_maxsize = p.block_maxsize; }
    c.hash = hash;
    if (!delivers(p)) { w = 0; stopped = false; }
    c.delivered += w;
    Report r{w, p.stop, lzf_scan::OK, p.end == END_MORE ? MORE : p.end == END_NEED_INPUT ? NEED_INPUT : DONE};
    if (stopped) { r.consumed = stop_consumed; r.status = stop_status; r.phase = DONE; }
    else if (p.end == END_ERROR) r.status = p.status;
    else if (p.end == END_ENDMARK && (p.flags & lzf_scan::FL_CSUM) && digest != p.want_content) r.status = FRAME_CHECKSUM_FAIL;
    c.phase = r.phase; c.status = r.status; c.in_off = r.consumed;
    return r;
}

// The window update (decompress.rs:253-269): the new window is the last new_len bytes of (old window ++ the call's w bytes):
// the last `keep` bytes of the old one, then the last `take` bytes of the call's output.  It is written to the OTHER buffer, so
// a piece shorter than the window never shifts a buffer onto itself.
struct WindowPlan { uint32_t keep, take, new_len; };
LZF_SCAN_HD inline WindowPlan window_plan(uint32_t old_len, uint64_t w) {
    const uint32_t take = w < WINDOW ? (uint32_t)w : WINDOW;
    const uint32_t keep = old_len < WINDOW - take ? old_len : WINDOW - take;
    return WindowPlan{keep, take, keep + take};
}
// The window in front of the first delivery: the dictionary's last <= 64 KiB.
LZF_SCAN_HD inline uint32_t dict_window(uint64_t dict_len) { return dict_len < WINDOW ? (uint32_t)dict_len : WINDOW; }

}  // namespace lzf_resume

#endif  // LZF_FRAME_RESUME_RULES_H
