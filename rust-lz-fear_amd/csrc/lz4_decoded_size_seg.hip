// lz4_decoded_size_seg.hip — the size call's latency class: ONE BLOCK SUMMED UP BY MANY WAVEFRONTS.  The tile helpers
// (tile_enumerate, tile_decode) are lzf_seg_common.h's, shared with the decode pipeline's tile stages (lz4_seg_tiles.hip);
// the rule is lzf_size_rules.h (TileSum, summarise, clean), which the CPU tests compile with g++.
//
// lzf_decoded_size_kernel walks a block's token chain with one wavefront: about 20 ms for a 4 MiB block whatever the batch.  A
// call that leaves the chip mostly empty takes the decode pipeline's front instead — plan, parse, seam: the bit map of the true
// tokens — and then
//   tile     one wavefront per 2 KiB tile of compressed bytes: the tile's true tokens, 64 per round; a wave scan of L + M behind the
//            tile-relative carry gives every lane its sequence's position, the lane summarises it, the wave reduces: 16 bytes per tile
//   finish   one wavefront per job: a 64-bit scan of the tiles' sums gives every tile its base position, every lane runs the three
//            position checks for its tile; a job of clean tiles gets {out_existing_len + total, LZF_OK} and done = 1
// Nothing else is written, and nothing at all for a job that is not clean: lzf_decoded_size_kernel, launched last over the whole
// call, skips the done jobs and gives every other one its status and length as it always did.
#include "lzf_seg_common.h"
#include "lzf_size_rules.h"

namespace lzf {

static_assert(kLenClamp == lzf_size::kTileLenClamp, "lzf_size_rules.h restates the clamp of tile_decode");
static_assert(sizeof(lzf_size::TileSum) == sizeof(u32x4), "one 16-byte store per tile");

__global__ __launch_bounds__(64) void lzf_size_tile_kernel(seg_ctx c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTileStage];
    __shared__ uint16_t list[kTileTokMax + 64u];
    const uint32_t j = seg_job_of(c, blockIdx.y);
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    cgu8* __restrict__ in = as_global(job.input);
    const uint32_t len = (uint32_t)job.input_len;
    LZF_GLOBAL u32x4* const TS = (LZF_GLOBAL u32x4*)c.tile_sum + (size_t)j * c.maxtile;
    for (uint32_t t = blockIdx.x; t < sj.ntile; t += gridDim.x) {
        __syncthreads();
        const uint32_t n = tile_enumerate(c, j, t, lane, len, in, stage, list);
        const TileCtx tc{t * kSegTile, lds_addr(stage), len, in};
        lzf_size::TileSum ts{0u, 0u, 0u, 0u};          // this lane's sequences, one per round
        uint64_t carry = 0;                            // tile-relative position behind the rounds so far
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            const bool act = i0 + lane < n;
            Tok k; k.L = 0; k.M = 0; k.off = 0; k.src = 0; k.err = false;
            if (act) k = tile_decode<true>(tc, tc.tstart + list[i0 + lane]);
            // a token that failed to decode adds nothing: its flag is all that is left of the tile
            const uint32_t tot = k.err ? 0u : k.L + k.M;                         // (each <= 2^26 + 4)
            // one 32-bit scan while 64 lengths cannot carry out of it; else 16-bit halves, added up in 64 bits
            uint64_t incl;
            if (__ballot(tot >= (1u << 24)) == 0ull) incl = wave_scan_add(tot);
            else incl = (uint64_t)wave_scan_add(tot & 0xFFFFu) + ((uint64_t)wave_scan_add(tot >> 16) << 16);
            if (act) {
                lzf_size::Seq s; s.M = k.M; s.L = k.L; s.off = k.off; s.has = k.M != 0u;
                lzf_size::summarise(ts, carry + (incl - tot), s, !k.err);
            }
            carry += (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)incl, 63) + ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(incl >> 32), 63) << 32);
        }
        // the lanes' summaries combined, field by field: max, max, max, or (a tile without a token: all zero)
        const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane(wave_scan_max(ts.sum), 63);
        const uint32_t end = (uint32_t)__builtin_amdgcn_readlane(wave_scan_max(ts.end), 63);
        const uint32_t need = (uint32_t)__builtin_amdgcn_readlane(wave_scan_max(ts.need), 63);
        const uint32_t flags = (__ballot(ts.flags & lzf_size::kTileZeroOffset) ? lzf_size::kTileZeroOffset : 0u) |
                               (__ballot(ts.flags & lzf_size::kTileUnsummarised) ? lzf_size::kTileUnsummarised : 0u);
        if (lane == 0u) TS[t] = u32x4{sum, end, need, flags};
    }
}

__global__ __launch_bounds__(64) void lzf_size_finish_kernel(seg_ctx c) {
    const uint32_t j = blockIdx.x;
    if (j >= c.n_jobs) return;
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    const uint64_t existing = job.out_existing_len, plen = job.prefix_len, limit = job.output_limit;
    const LZF_GLOBAL u32x4* const TS = (const LZF_GLOBAL u32x4*)c.tile_sum + (size_t)j * c.maxtile;
    uint64_t total = 0;                                // the sums of the tiles in front of the round
    bool bad = false;
    // (eight rounds' loads in flight at once, as in lzf_seg_scan_kernel: one round per round trip to HBM makes a 4 MiB block's 33 rounds a chain of 33 loads)
    for (uint32_t t8 = 0; t8 < sj.ntile; t8 += 512u) {
        u32x4 v[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) { const uint32_t t = t8 + 64u * k + lane; v[k] = t < sj.ntile ? TS[t] : u32x4{0u, 0u, 0u, 0u}; }
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const lzf_size::TileSum ts{v[k][0], v[k][1], v[k][2], v[k][3]};      // (lanes behind the last tile: an empty tile, clean anywhere)
            // sums are below 2^31: 16-bit halves, 64 of them stay below 2^22, and a 64-bit carry
            const uint32_t ilo = wave_scan_add(ts.sum & 0xFFFFu), ihi = wave_scan_add(ts.sum >> 16);
            const uint64_t incl = (uint64_t)ilo + ((uint64_t)ihi << 16);
            bad = bad || !lzf_size::clean(ts, existing + total + (incl - ts.sum), plen, limit);
            total += (uint64_t)(uint32_t)__builtin_amdgcn_readlane(ilo, 63) + ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(ihi, 63) << 16);
        }
    }
    if (__ballot(bad) != 0ull || total > 0xFFFFFFFFull) return;                  // not clean: the one-wave kernel's job, nothing written
    if (lane == 0u) {
        c.results[j].out_len = existing + total;
        c.results[j].status = LZF_OK;
        c.results[j].reserved = sj.ntile;              // diagnostic: the tiles the job was summed up in
        c.st[j].done = 1u;
    }
}

}  // namespace lzf
