// lzf_seg_common.h — raw::decompress_raw (src/raw/decompress.rs:58-138) for gfx950 with ONE BLOCK DECODED BY MANY
// WAVEFRONTS: the segmented pipeline of kernels.h (plan, parse, seam, tilesum, scan, records + levels, resolve), one source per
// group of stages, and in this header what two or more of them share:
//   lz4_seg_front.hip          plan, parse, seam — also the front of the fed call (plan, parse: seg_ctx::fed) and of the size call's latency class
//   lz4_seg_tiles.hip          tilesum, scan, records
//   lz4_seg_order.hip          the launch orders (by_len, rank, order) and the pause between two groups
//   lz4_seg_resolve.hip        resolve
//   lz4_decoded_size_seg.hip   the size call's latency class behind the front: lzf_size_tile_kernel, lzf_size_finish_kernel
// A helper with one user stands in that user's source.
//
// Why: a block is a serial chain twice over — the position of a token depends on every token before it
// (decompress.rs:61-71), and a match copies bytes an earlier match produced (:80-138; on text the chain of dependent
// matches is ~1/11 of the sequences long in windows of 64, tools/seg_depth.c).  One workgroup per block therefore needs ~20 ms per 4 MiB
// block whatever the load.  Here everything that is not the second chain is spread over the chip:
//   * the first chain is cut by SPECULATION: a token walk started at an arbitrary byte is on the true chain within 1-2 KB
//     (tools/seq_stats.c), so every 16 KiB chunk is parsed on its own from its first byte and the chains are joined where
//     the true one steps on a token the next chunk's chain has marked;
//   * literals go to their final place in `out` from all tiles at once (they depend on nothing);
//   * the second chain is reduced to what it is: per batch of 64 sequences, one LDS round (read, write) per dependency
//     level, by a wave that does nothing else — the records it consumes carry positions, lengths and levels.
// History (decompress.rs:80-99: a match source lies on the virtual stream prefix ++ output): a job's existing output
// out[0, E) is output that is final before the launch — the tiles' sums start at E, every position is absolute, the
// resolve stage primes its ring with the tail of out[0, E) and stores nothing below out + E; a source in the prefix is
// moved in by the stager from `prefix` (class 13), one that starts there and ends in the output stands alone like a
// sequence larger than a sub-batch (class 8).  So the blocks of a linked frame and of a frame with a dictionary are
// the pipeline's like any other.
// Error behaviour: the pipeline only finishes jobs that decode cleanly.  Anything else (every DecodeError, a buffer that
// is too small, sizes outside the window, history beyond 31-bit positions) is left to the pair kernel, launched last,
// which skips finished jobs — so statuses and partial outputs are exactly the pair kernel's.
#pragma once
#include "lzf_device.h"
#include "kernels.h"
#include "lzf_copy_helpers.h"

namespace lzf {
namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kLenClamp = 1u << 26;           // a literal / match length beyond this sends the job to the pair kernel
constexpr uint32_t kTileStage = kSegTile + 128u;   // staged bytes of a tile
constexpr uint32_t kTileTokMax = kSegTile / 3u + 2u;

// cooperative copy of a long run, 4 KiB per step with four loads in flight per lane (the records stage's long literals, the stager's class 8)
__device__ __forceinline__ void wave_copy_long(gu8* __restrict__ dst, cgu8* __restrict__ src, uint32_t n, uint32_t lane) {
    uint32_t i = 0;
    for (; i + 4096u <= n; i += 4096u) {
        const uint32_t o = i + lane * 16u;
        const u32x4 a0 = ld16(src + o), a1 = ld16(src + o + 1024u), a2 = ld16(src + o + 2048u), a3 = ld16(src + o + 3072u);
        st16(dst + o, a0); st16(dst + o + 1024u, a1); st16(dst + o + 2048u, a2); st16(dst + o + 3072u, a3);
    }
    wave_copy(dst + i, src + i, n - i, lane);
}

// ---- the token readers of parse, seam and tile_decode, over whatever holds the bytes (RD8 / RDB)
// Length of the run of 0xFF bytes that starts at q (stops at len): the body of read_lsic (decompress.rs:30-43) eight bytes
// at a time.  RD8(q) = 8 bytes at q (q + 8 <= len), RDB(q) = one byte.
template <class RD8, class RDB>
__device__ __forceinline__ uint32_t count_ff(uint32_t q, uint32_t len, RD8 rd8, RDB rdb) {
    uint32_t n = 0;
    while (len - q >= 8u) {
        const uint64_t w = rd8(q);
        if (w != ~0ull) return n + ((uint32_t)__builtin_ctzll(~w) >> 3);
        n += 8u; q += 8u;
    }
    while (q < len && rdb(q) == 255u) { ++n; ++q; }
    return n;
}
// LSIC value that continues a nibble of 15 at q: false when the input ends before the terminating byte (UnexpectedEnd).
// v = 15 + 255 * run + last byte, clamped; q moves behind the last byte.
template <class RD8, class RDB>
__device__ __forceinline__ bool read_lsic_tail(uint32_t& q, uint32_t len, uint32_t& v, RD8 rd8, RDB rdb) {
    if (q >= len) return false;
    const uint32_t n = count_ff(q, len, rd8, rdb);
    if (q + n >= len) { q = len; return false; }
    const uint64_t vv = 15ull + 255ull * n + rdb(q + n);
    v = vv > kMaxPosB ? kMaxPosB : (uint32_t)vv;
    q += n + 1u;
    return true;
}
// One token at p (p < len), general form: position of the next token; false on UnexpectedEnd.
// decompress.rs:61-71 without the copies.
template <class RD8, class RDB>
__device__ __forceinline__ bool token_next_gen(uint32_t len, uint32_t p, uint32_t& next, RD8 rd8, RDB rdb) {
    const uint32_t tok = rdb(p);
    uint32_t q = p + 1u;
    uint32_t L = tok >> 4;
    if (L == 15u) { if (!read_lsic_tail(q, len, L, rd8, rdb)) return false; }
    if (len - q < L) return false;                    // :67 read_exact
    q += L;
    if (len - q < 2u) { next = len; return true; }    // :70 read_u16 fails: last literals
    q += 2u;
    if ((tok & 15u) == 15u) { uint32_t M; if (!read_lsic_tail(q, len, M, rd8, rdb)) return false; }
    next = q;
    return true;
}
__device__ __forceinline__ uint64_t lds_ld64u(uint32_t a) {
    uint64_t v; asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory"); return v;
}

// =====================================================================================================================
// tiles: enumerate the true tokens of 2 KiB of compressed bytes and decode them
// =====================================================================================================================
struct TileCtx {
    uint32_t tstart;     // first byte of the tile
    uint32_t stage_a;    // LDS address of the staged bytes
    uint32_t len;
    cgu8* in;
};
__device__ __forceinline__ uint32_t tile_rdb(const TileCtx& t, uint32_t q) {
    const uint32_t r = q - t.tstart;
    if (r < kTileStage) return lds_ld8(t.stage_a + r);
    return (uint32_t)t.in[q];
}
// The tokens of tile t of job j: positions (tile-relative) into list[], count returned.  Also stages the tile's bytes.
__device__ __forceinline__ uint32_t tile_enumerate(const seg_ctx& c, uint32_t j, uint32_t t, uint32_t lane, uint32_t len, cgu8* in,
                                                   uint8_t* stage, uint16_t* list) {
    const uint32_t tstart = t * kSegTile;
    // stage [tstart, tstart + kTileStage)
    {
        const uint32_t avail = len - tstart < kTileStage ? len - tstart : kTileStage;
        cgu8* g = in + tstart;
        for (uint32_t i = lane * 16u; i < kTileStage; i += 1024u) {
            u32x4 v = u32x4{0, 0, 0, 0};
            if (i + 16u <= avail) v = ld16(g + i);
            else if (i < avail) { for (uint32_t b = 0; i + b < avail; ++b) v[(b >> 2) & 3u] |= (uint32_t)g[i + b] << ((b & 3u) * 8u); }
            *reinterpret_cast<u32x4*>(&stage[i]) = v;
        }
    }
    const uint32_t h = t < kSegChunk / kSegTile ? 0u : 1u + (t - kSegChunk / kSegTile) / (kSegStride / kSegTile);
    const uint32_t widx = t * (kSegTile / 32u) - h * (kSegStride / 32u) + lane;
    uint32_t w = c.bits[((size_t)j * c.maxch + h) * kSegChunkWords + widx];
    const uint32_t vf = c.vfrom[(size_t)j * c.maxch + h];
    const uint32_t wpos = tstart + lane * 32u;                 // position of bit 0
    if (vf == kNone || vf >= wpos + 32u) w = 0u;
    else if (vf > wpos) w &= ~((1u << (vf - wpos)) - 1u);
    if (wpos >= len) w = 0u;
    else if (len - wpos < 32u) w &= (1u << (len - wpos)) - 1u;
    const uint32_t cnt = (uint32_t)__popc(w);
    const uint32_t incl = wave_scan_add(cnt);
    uint32_t k = incl - cnt;
    while (w) { const uint32_t b = (uint32_t)__builtin_ctz(w); list[k++] = (uint16_t)(lane * 32u + b); w &= w - 1u; }
    __syncthreads();
    return __builtin_amdgcn_readlane(incl, 63);
}
struct Tok { uint32_t L, M, off, src; bool err; };
// decompress.rs:61-74 for the token at p (p < len): lengths, offset, where its literals are.  M = 0: the last sequence.
// WANT_OFF = false: the lengths alone (the tile sums do not look at the offset).
template <bool WANT_OFF = true>
__device__ __forceinline__ Tok tile_decode(const TileCtx& t, uint32_t p) {
    Tok k; k.err = false; k.M = 0; k.off = 0;
    const uint32_t len = t.len;
    uint32_t w;
    if (p - t.tstart + 4u <= kTileStage) { asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(t.stage_a + (p - t.tstart)) : "memory"); }
    else { w = 0; for (uint32_t i = 0; i < 4u && p + i < len; ++i) w |= tile_rdb(t, p + i) << (8u * i); }
    const uint32_t tok = w & 255u;
    uint32_t q = p + 1u;
    uint32_t L = tok >> 4;
    auto rd8 = [&](uint32_t x) -> uint64_t { const uint32_t r = x - t.tstart; if (r + 8u <= kTileStage) return lds_ld64u(t.stage_a + r); return ld8(t.in + x); };
    auto rdb = [&](uint32_t x) -> uint32_t { return tile_rdb(t, x); };
    if (L == 15u) {
        if (((w >> 8) & 255u) != 255u && q < len) { L += (w >> 8) & 255u; ++q; }
        else if (!read_lsic_tail(q, len, L, rd8, rdb) || L > kLenClamp) k.err = true;
    }
    k.L = L; k.src = q;
    if (k.err) return k;
    if (len - q < L) { k.err = true; return k; }           // :67 read_exact
    q += L;
    if (len - q < 2u) return k;                            // :70 read_u16 fails: last literals, no match
    if (WANT_OFF) k.off = tile_rdb(t, q) | (tile_rdb(t, q + 1u) << 8);
    q += 2u;
    uint32_t M = tok & 15u;
    if (M == 15u) { if (!read_lsic_tail(q, len, M, rd8, rdb) || M > kLenClamp) k.err = true; }
    k.M = M + 4u;
    return k;
}
}  // namespace
}  // namespace lzf
