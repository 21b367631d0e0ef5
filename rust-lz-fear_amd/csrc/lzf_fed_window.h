// lzf_fed_window.h — the WINDOW RULES of the bitmap-fed decompress kernel (lz4_decompress_fed.hip, lz4_decompress_feed_phase.inc,
// lz4_decompress_batch_phase.inc under LZF_FED_DECODE) as plain functions the kernel, a CPU emulator (tests/emu/emu_fed_window.cpp)
// and the fill model (tools/fed_fill_model.c) all compile: C and C++, host and device.
//
//   lzf_fedw_start   where the window that serves the chain position `expect` begins
//   lzf_fedw_chunk   which chunk of the segmented parse owns the bit-map word of a 32-aligned position
//   lzf_fedw_word    that word's index in the chunk's row of the bit map
//   lzf_fedw_carry   is the short batch at the end of a window's token list left for the next window
//
// A window is kFedwRound compressed bytes from a 32-aligned position: one bit-map word per lane.  The parse writes one row of
// kFedwChunk bits per chunk; chunk h starts at h * kFedwStride, chunk 0 owns its whole row and chunk h >= 1 the positions from
// h * kFedwStride + kFedwOverlap on, up to where chunk h + 1 owns.  Chunk starts, the overlap and the stride are multiples of 32,
// so a 32-aligned word lies inside ONE chunk's share; a window may straddle a boundary between two shares, its words never do.
// (Until the windows followed the chain a window was a kFedwRound-aligned round and the kernel asserted that rounds subdivide the
// 2 KiB tiles of the segmented pipeline, so that a whole round had one owner; the per-word owner below replaces that.)
#ifndef LZF_FED_WINDOW_H
#define LZF_FED_WINDOW_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LZF_FEDW_HD __host__ __device__ static inline
#else
#define LZF_FEDW_HD static inline
#endif

enum {
    kFedwChunk = 16384,                      // = kSegChunk   (kernels.h asserts the three)
    kFedwOverlap = 2048,                     // = kSegOverlap
    kFedwStride = kFedwChunk - kFedwOverlap, // = kSegStride
    kFedwRound = 1024,                       // compressed bytes of a window: 32 bit-map words
    kFedwLanes = 64,                         // sequences of a full batch
    // A batch of at most this many sequences at the end of a window's list waits for the next window, which starts on its first
    // token and fills the batch up (tools/fed_fill_model.c: 245 351 -> 214 678 batches over the Silesia stand-in).
    kFedwCarry = 32
};
#if defined(__cplusplus)
static_assert(kFedwChunk % 32 == 0 && kFedwOverlap % 32 == 0 && kFedwStride % 32 == 0, "a 32-aligned bit-map word has one owner");
#endif

// fixed != 0: the kFedwRound-aligned rounds of the kernel before the windows followed the chain (kept for A/B timing)
LZF_FEDW_HD uint32_t lzf_fedw_start(uint32_t expect, int fixed) {
    return fixed ? expect & ~(uint32_t)(kFedwRound - 1) : expect & ~31u;
}
LZF_FEDW_HD uint32_t lzf_fedw_chunk(uint32_t wpos) {
    return wpos < (uint32_t)kFedwChunk ? 0u : 1u + (wpos - (uint32_t)kFedwChunk) / (uint32_t)kFedwStride;
}
LZF_FEDW_HD uint32_t lzf_fedw_word(uint32_t wpos, uint32_t h) {
    return (wpos - h * (uint32_t)kFedwStride) >> 5;
}
// The batch that would start at token `tidx` of a window's list of `tc` tokens: left for the next window?
//   - it ends at the end of the list, short of a full batch: tc - tidx <= carry (carry < kFedwLanes);
//   - it is not the window's first batch (tidx > 0) — THE PROGRESS GUARANTEE: every window runs at least one batch;
//   - the window does not reach the end of the input (window_end < len): no later window would pick the tail up.
// The decision is taken before the batch's tokens are decoded, so a tail the span limit would cut in two is carried as well (it is
// cut in the next window).  carry = 0: never.
LZF_FEDW_HD int lzf_fedw_carry(uint32_t tc, uint32_t tidx, uint32_t window_end, uint32_t len, uint32_t carry) {
    return tidx > 0u && tc - tidx <= carry && window_end < len;
}

// ---- the PIECE RULES: a launch of more jobs than resident wavefronts cuts every job into `pieces` stretches and deals (job, piece)
// tickets out group by group (lz4_decompress_fed.hip; a group is the jobs of one XCD).
//
//   lzf_fedw_piece_end     where piece p of a job of `len` compressed bytes ends: the tokens that START below it are the piece's
//   lzf_fedw_group_jobs    how many of n jobs (ranks g, g + ng, g + 2 ng, ...) group g of ng serves
//   lzf_fedw_ticket_piece  ticket tk of a group of n_g jobs -> the piece: lap after lap over the group's jobs
//   lzf_fedw_ticket_rank   ... and the job's rank in launch order; piece p - 1 of a job is drawn n_g tickets before its piece p
//
// A job is `rounds` windows' worth of input; every piece but the last is `per` whole rounds, the last ends at len — and so does
// every piece from the one that reaches the last round on (rounds < pieces: the later pieces are empty).
LZF_FEDW_HD uint32_t lzf_fedw_piece_end(uint32_t len, uint32_t pieces, uint32_t p) {
    const uint32_t rounds = (len + (uint32_t)kFedwRound - 1u) / (uint32_t)kFedwRound, per = (rounds + pieces - 1u) / pieces;
    return (p + 1u) * per >= rounds ? len : (p + 1u) * per * (uint32_t)kFedwRound;
}
LZF_FEDW_HD uint32_t lzf_fedw_group_jobs(uint32_t n, uint32_t g, uint32_t ng) {
    return n > g ? (n - g + ng - 1u) / ng : 0u;
}
LZF_FEDW_HD uint32_t lzf_fedw_ticket_piece(uint32_t tk, uint32_t n_g) {
    return tk / n_g;
}
LZF_FEDW_HD uint32_t lzf_fedw_ticket_rank(uint32_t tk, uint32_t piece, uint32_t n_g, uint32_t g, uint32_t ng) {
    return (tk - piece * n_g) * ng + g;
}

#endif  // LZF_FED_WINDOW_H
