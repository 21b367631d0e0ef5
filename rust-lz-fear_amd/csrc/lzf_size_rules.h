// lzf_size_rules.h — the arithmetic of raw::decompress_raw (src/raw/decompress.rs:58-99) without the copies, as
// __host__ __device__ code: what a token adds to output.len() and which DecodeError its sequence raises.
//
// Every DecodeError depends on positions and lengths only, never on an output byte: an offset is compared with
// output.len() + prefix.len() (:83-89), a match end with output_limit (:72-74).  So adding lengths gives the decoder's status and
// its output.len().  The size kernel (lz4_decoded_size.hip) runs decode_token and check per lane, 64 tokens per round, with
// a wave scan of L + M in between; the CPU tests compile this header with g++ (tests/emu/emu_decoded_size.cpp) and hold it
// to the reference on blocks of every error kind.  Status codes are those of include/lzfear_hip.h.
//
// Positions are 64-bit: a block below the decoder's input limit (2 GiB) decodes to up to 255 x that, and callers pass
// 2^63 - 1 as "no limit".
//
// Follow-up (one block over many wavefronts): chunk sums compose.  A chunk's run of sequences is summarised by its length
// sum and, for the two position checks, by the largest M + L-prefix against the limit and the largest "offset minus
// position" — both relative to the chunk's start — so a later pass that knows the start position finishes the checks.
#ifndef LZF_SIZE_RULES_H
#define LZF_SIZE_RULES_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define LZF_SIZE_HD __host__ __device__ __forceinline__
#else
#define LZF_SIZE_HD inline
#endif

namespace lzf_size {

enum : int { OK = 0, UNEXPECTED_END = 1, MEMORY_LIMIT_EXCEEDED = 2, ZERO_DEDUP_OFFSET = 3, INVALID_DEDUP_OFFSET = 4 };

// One sequence (decompress.rs:61-76): L literals, then — when two more bytes follow them (:70 read_u16) — a match of M bytes
// at `off`.  The last sequence of a block has no match: has = false, M = 0.
struct Seq {
    uint64_t M;         // 4 + read_lsic(token & 15): up to 255 per input byte, beyond 32 bits for inputs over 16 MiB
    uint32_t L;         // read_lsic(token >> 4): never more than the input holds (:67 read_exact), else UnexpectedEnd
    uint32_t off;
    bool has;
};

// Decodes the token at `tp` (tp < len) of an input of `len` bytes (len < 2 GiB).  Readers:
//   rd4(p)    the 4 input bytes at p, bytes at or past `len` read as 0
//   rd1(p)    the byte at p < len
//   ffrun(p)  how many bytes from p on are 0xFF, counting no further than `len`
// Returns false on UnexpectedEnd (:63 / :67 / :71: a length byte or a literal is missing); `next` is where the following
// token starts, `len` after the last sequence.  The common token — no 0xFF length byte — takes no loop.
template <class R4, class R1, class RF>
LZF_SIZE_HD bool decode_token(uint32_t tp, uint32_t len, R4 rd4, R1 rd1, RF ffrun, Seq& s, uint32_t& next) {
    const uint32_t w = rd4(tp);
    const uint32_t l0 = (w >> 4) & 15u, b1 = (w >> 8) & 255u, m0 = w & 15u;
    const bool lx = l0 == 15u;
    uint32_t L = l0 + (lx ? b1 : 0u);
    uint32_t q = tp + (lx ? 2u : 1u);                 // the literals
    s.M = 0; s.L = 0; s.off = 0; s.has = false; next = len;
    if (lx && tp + 1u >= len) return false;           // :63 read_lsic: the first length byte is missing
    if (lx && b1 == 255u) {                           // a run of 0xFF length bytes, then the byte that ends it
        const uint32_t n = ffrun(q);
        if (len - q <= n) return false;               // the run reaches the end of the input
        // 255 * (n + 1) + 15 + 254 overflows 32 bits only where the literals cannot be there either
        if (n >= (1u << 23)) return false;            // L > 2^31 > len: :67 read_exact fails
        L += 255u * n + rd1(q + n);
        q += n + 1u;
    }
    if (len - q < L) return false;                    // :67 read_exact
    s.L = L;
    q += L;
    if (len - q < 2u) return true;                    // :70 read_u16 fails: the loop ends at the next read_u8 or here
    s.off = rd1(q) | (rd1(q + 1u) << 8);
    q += 2u;
    uint64_t M = m0;
    if (m0 == 15u) {
        if (q >= len) return false;                   // :71 read_lsic
        const uint32_t b = rd1(q); ++q;
        M += b;
        if (b == 255u) {
            const uint32_t n = ffrun(q);
            if (len - q <= n) return false;
            M += 255ull * n + rd1(q + n);
            q += n + 1u;
        }
    }
    s.M = M + 4u; s.has = true; next = q;
    return true;
}

// The checks of one sequence with a match, in the reference's order (:72-74, then copy_overlapping :83-89).  `mo` is
// output.len() behind the sequence's literals (existing output included); literals are not limit-checked (:63-67).
LZF_SIZE_HD int check(uint64_t mo, uint64_t M, uint32_t off, uint64_t prefix_len, uint64_t output_limit) {
    if (mo + M > output_limit) return MEMORY_LIMIT_EXCEEDED;          // (mo + M < 2^41: no wrap)
    if (off == 0u) return ZERO_DEDUP_OFFSET;
    if ((uint64_t)off > mo && (uint64_t)off - mo > prefix_len) return INVALID_DEDUP_OFFSET;
    return OK;
}

// The carry from sequence to sequence (and from round to round of the kernel): output.len().
LZF_SIZE_HD uint64_t advance(uint64_t pos, const Seq& s) { return pos + s.L + s.M; }

}  // namespace lzf_size

#endif  // LZF_SIZE_RULES_H
