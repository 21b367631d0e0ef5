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
// One block over many wavefronts (lzf_size_tile_kernel / lzf_size_finish_kernel, lz4_decoded_size_seg.hip): sums compose.  The true
// tokens that start in a tile of compressed bytes are summarised RELATIVE to the tile's first token (TileSum, summarise); a second
// pass that knows every tile's base position finishes the three checks (clean).  That path only says "clean, and this long" or
// nothing: which error a job has, and where, stays with the token-by-token walk above.
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

// ---- tiles -----------------------------------------------------------------------------------------------------------------------
// What the sequences of one tile come to, relative to output position 0 at the tile's first token:
//   sum    the position behind the tile's last sequence (the sum of L + M); at most kTileSumMax
//   end    the largest mo_rel + M over the sequences with a match — their ends rise, so the last match's end; 0: no match
//   need   the largest off - mo_rel (0 where the offset stays inside the tile) over the sequences with a match: how much output the
//          tile wants in front of itself; at most 65 535
//   flags  kTileZeroOffset: a match with offset 0;  kTileUnsummarised: a token that could not be decoded, a length beyond kTileLenClamp
//          or a sum beyond kTileSumMax
// Every field only grows, so summaries of parts of a tile that share its origin combine field by field (max, max, max, or): the
// tile kernel summarises 64 sequences at once, one per lane, and reduces with three wave maxima and a ballot.
struct TileSum { uint32_t sum, end, need, flags; };
enum : uint32_t { kTileZeroOffset = 1u, kTileUnsummarised = 2u };
constexpr uint32_t kTileLenClamp = 1u << 26;          // (the segmented pipeline's kLenClamp: longer literals / matches are the one-wave kernel's)
constexpr uint64_t kTileSumMax = 0x7FFFFFFFull;

// One sequence whose first literal sits at tile-relative position `rel` into the running summary; decoded = decode_token's (or the
// tile decoder's) verdict.  Serial use: rel = t.sum.
LZF_SIZE_HD void summarise(TileSum& t, uint64_t rel, const Seq& s, bool decoded) {
    if (!decoded || s.L > kTileLenClamp || s.M > (uint64_t)kTileLenClamp + 4u) { t.flags |= kTileUnsummarised; return; }
    const uint64_t mo = rel + s.L, behind = mo + s.M;
    if (behind > kTileSumMax) { t.flags |= kTileUnsummarised; return; }
    if (behind > t.sum) t.sum = (uint32_t)behind;
    if (!s.has) return;
    if (s.off == 0u) t.flags |= kTileZeroOffset;
    if (behind > t.end) t.end = (uint32_t)behind;
    const uint32_t need = (uint64_t)s.off > mo ? (uint32_t)((uint64_t)s.off - mo) : 0u;
    if (need > t.need) t.need = need;
}
// check()'s three tests over a tile whose first token sits at output position `base` (existing output included; 64 bits).
// Literals are not limit-checked, as in the reference (:63-67).
LZF_SIZE_HD bool clean(const TileSum& t, uint64_t base, uint64_t prefix_len, uint64_t output_limit) {
    if (t.flags) return false;
    if (t.end && base + t.end > output_limit) return false;       // :72-74
    return (uint64_t)t.need <= base + prefix_len;                  // :83-89
}
// The carry from tile to tile, and a job's verdict: clean with out_existing_len + the sums — or not this path's business.
struct Fold { uint64_t base; bool clean; };
LZF_SIZE_HD Fold fold_begin(uint64_t existing) { return Fold{existing, true}; }
LZF_SIZE_HD void fold(Fold& f, const TileSum& t, uint64_t prefix_len, uint64_t output_limit) {
    f.clean = f.clean && clean(t, f.base, prefix_len, output_limit);
    f.base += t.sum;
}
// (a job whose total does not fit 32 bits is left to the one-wave kernel as well)
LZF_SIZE_HD bool fold_end(const Fold& f, uint64_t existing) { return f.clean && f.base - existing <= 0xFFFFFFFFull; }

}  // namespace lzf_size

#endif  // LZF_SIZE_RULES_H
