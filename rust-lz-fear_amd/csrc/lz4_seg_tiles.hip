// lz4_seg_tiles.hip — the tile stages of the segmented pipeline (lzf_seg_common.h, kernels.h): tilesum, scan, records.  They run behind
// the front (lz4_seg_front.hip) on the bit map of the true tokens and leave the records the resolve stage (lz4_seg_resolve.hip) consumes.
#include "lzf_seg_common.h"

namespace lzf {
namespace {

// The records stage's own copies of literals (long runs: wave_copy_long of the common header), with their packed unaligned stores.
struct __attribute__((packed, aligned(1))) S8B { uint64_t v; };
struct __attribute__((packed, aligned(1))) S4B { uint32_t v; };
struct __attribute__((packed, aligned(1))) S2B { uint16_t v; };
__device__ __forceinline__ void st8(gu8* p, uint64_t v) { reinterpret_cast<LZF_GLOBAL S8B*>(p)->v = v; }
__device__ __forceinline__ void st4(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL S4B*>(p)->v = v; }
__device__ __forceinline__ void st2(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL S2B*>(p)->v = (uint16_t)v; }

// exact per-lane copy of n (1..64) bytes, global -> global, ranges not overlapping: two-ended pieces
__device__ __forceinline__ void copy_small_gg(gu8* d, cgu8* g, uint32_t n) {
    if (n > 32u) {
        const uint64_t a0 = ld8(g), a1 = ld8(g + 8u), a2 = ld8(g + 16u), a3 = ld8(g + 24u);
        const uint64_t b0 = ld8(g + n - 32u), b1 = ld8(g + n - 24u), b2 = ld8(g + n - 16u), b3 = ld8(g + n - 8u);
        st8(d, a0); st8(d + 8u, a1); st8(d + 16u, a2); st8(d + 24u, a3);
        st8(d + n - 32u, b0); st8(d + n - 24u, b1); st8(d + n - 16u, b2); st8(d + n - 8u, b3);
    } else if (n >= 16u) {
        const uint64_t a0 = ld8(g), a1 = ld8(g + 8u), b0 = ld8(g + n - 16u), b1 = ld8(g + n - 8u);
        st8(d, a0); st8(d + 8u, a1); st8(d + n - 16u, b0); st8(d + n - 8u, b1);
    } else if (n >= 8u) {
        const uint64_t a0 = ld8(g), b0 = ld8(g + n - 8u);
        st8(d, a0); st8(d + n - 8u, b0);
    } else if (n >= 4u) {
        const uint32_t a0 = ld4(g), b0 = ld4(g + n - 4u);
        st4(d, a0); st4(d + n - 4u, b0);
    } else if (n >= 2u) {
        const uint32_t a0 = ld2(g), b0 = ld2(g + n - 2u);
        st2(d, a0); st2(d + n - 2u, b0);
    } else if (n == 1u) {
        d[0] = g[0];
    }
}

// per-lane copy of n (65..256) bytes, global -> global, ranges not overlapping: 16-byte pieces, the last one two-ended
__device__ __forceinline__ void copy_medium_gg(gu8* d, cgu8* g, uint32_t n) {
    uint32_t t = 0;
    for (; t + 64u <= n; t += 64u) {
        const u32x4 a0 = ld16(g + t), a1 = ld16(g + t + 16u), a2 = ld16(g + t + 32u), a3 = ld16(g + t + 48u);
        st16(d + t, a0); st16(d + t + 16u, a1); st16(d + t + 32u, a2); st16(d + t + 48u, a3);
    }
    for (; t + 16u <= n; t += 16u) st16(d + t, ld16(g + t));
    if (t < n) st16(d + n - 16u, ld16(g + n - 16u));
}
}  // namespace

__global__ __launch_bounds__(64) void lzf_seg_tilesum_kernel(seg_ctx c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTileStage];
    __shared__ uint16_t list[kTileTokMax + 64u];
    const uint32_t j = seg_job_of(c, blockIdx.y);
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    cgu8* __restrict__ in = as_global(job.input);
    const uint32_t len = (uint32_t)job.input_len;
    for (uint32_t t = blockIdx.x; t < sj.ntile; t += gridDim.x) {
        __syncthreads();
        const uint32_t n = tile_enumerate(c, j, t, lane, len, in, stage, list);
        TileCtx tc{t * kSegTile, lds_addr(stage), len, in};
        uint32_t sum = 0; bool err = false;
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            if (i0 + lane < n) {
                const Tok k = tile_decode<false>(tc, tc.tstart + list[i0 + lane]);
                err = err || k.err;
                sum += k.L + k.M;                          // (each <= 2^26 + 4, at most 11 per lane)
            }
        }
        const uint64_t tot = (uint64_t)__builtin_amdgcn_readlane(wave_scan_add(sum & 0xFFFFu), 63) +
                             ((uint64_t)__builtin_amdgcn_readlane(wave_scan_add(sum >> 16), 63) << 16);
        if (tot > 0x7FFFFFFFull) err = true;
        // (records are kept in batches of 64 that never span tiles: a tile's tokens take ceil(n / 64) batches, the last one padded)
        if (lane == 0u) { c.tile_tok[(size_t)j * c.maxtile + t] = (n + 63u) / 64u; c.tile_out[(size_t)j * c.maxtile + t] = (uint32_t)tot; }
        if (__ballot(err) && lane == 0u) c.st[j].failed = 1u;
    }
}

__global__ __launch_bounds__(64) void lzf_seg_scan_kernel(seg_ctx c) {
    if (blockIdx.x >= c.g_n) return;
    const uint32_t j = c.grouped ? seg_job_of(c, blockIdx.x) : blockIdx.x;
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    LZF_GLOBAL uint32_t* const TT = (LZF_GLOBAL uint32_t*)c.tile_tok + (size_t)j * c.maxtile;
    LZF_GLOBAL uint32_t* const TO = (LZF_GLOBAL uint32_t*)c.tile_out + (size_t)j * c.maxtile;
    uint64_t ctok = 0, cout = job.out_existing_len;            // the job's first output byte: positions are absolute from here on (the plan stage: below kMaxPosB)
    // (eight steps' loads in flight at once: with one step per round trip to HBM the kernel was 33 dependent loads long, 75 us)
    for (uint32_t t8 = 0; t8 < sj.ntile; t8 += 512u) {
        uint32_t av[8], bv[8];
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) { const uint32_t t = t8 + 64u * k + lane; av[k] = t < sj.ntile ? TT[t] : 0u; bv[k] = t < sj.ntile ? TO[t] : 0u; }
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t t = t8 + 64u * k + lane;
            const uint32_t a = av[k], b = bv[k];
            // 64-bit running sums (a job whose output does not fit 31 bits is not ours)
            const uint32_t ia = wave_scan_add(a);
            uint32_t blo = b & 0xFFFFu, bhi = b >> 16;
            const uint32_t ilo = wave_scan_add(blo), ihi = wave_scan_add(bhi);
            const uint64_t ib = (uint64_t)ilo + ((uint64_t)ihi << 16);
            const uint64_t eo = cout + ib - b;
            if (t < sj.ntile) { TT[t] = (uint32_t)(ctok + ia - a); TO[t] = eo > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)eo; }
            ctok += __builtin_amdgcn_readlane(ia, 63);
            cout += (uint64_t)__builtin_amdgcn_readlane(ilo, 63) + ((uint64_t)__builtin_amdgcn_readlane(ihi, 63) << 16);
        }
    }
    if (lane == 0u) {
        const uint64_t cap = LZF_DECODE_JOB_VIEW(job).cap;                       // (64 bits here: it is set against 64-bit sums)
        ctok *= 64ull;                                                           // batches -> records (padded)
        bool ok = cout <= cap && ctok < 0x7FFFFFFFull;
        uint64_t off = 0;
        if (ok) {
            const uint64_t need = ctok + 64ull;
            off = atomicAdd(c.rec_top, (unsigned long long)need);
            if (off + need > c.rec_cap) ok = false;
        }
        if (!ok) c.st[j].failed = 1u;
        else { c.st[j].ntok = (uint32_t)ctok; c.st[j].outb = (uint32_t)cout; c.st[j].rec_off = off; }
    }
}

// =====================================================================================================================
// records + literals + levels: everything the resolve stage needs to know about a sequence, so that its two wavefronts
// compute nothing of it themselves
// =====================================================================================================================
// Per batch of 64 tokens of a tile (batches never span tiles; the last one of a tile is padded with empty sequences):
// decode (decompress.rs:61-74), absolute positions, the checks of :72-74,:83-89, LITERALS -> out, then
// level(j) = 1 + max level of the matches (of the same batch) whose destination overlaps j's source bytes; 1 when there
// are none (everything in front of the batch is final when the batch starts).  Destinations are disjoint and in stream
// order, so the matches j depends on are a range of lanes [i_lo, i_hi], found by two binary searches; ranges wider than
// two lanes use the running maximum up to i_hi (never too small: a larger level is only later, not wrong).
// Record:  w0 = M,  w1 = biased destination (mo + rb, rb = out & 15),  w2 = sub-batch (0..63) | level << 16 | class << 24,  w3 = off.
// Sub-batches: consecutive sequences of the batch whose output spans at most ring / 8 bytes (greedy).
// Classes: 0 no match | 1: 4..7 bytes | 2: 8..16 | 3: 17..32 | 4: 33..64 (all not overlapping, source inside the ring) |
//   5 overlapping, <= 64 | 6 whole wave (longer, or wrapping around the ring) | 7 source (partly) older than what the ring
//   is guaranteed to hold when the sub-batch is resolved: moved by the stager | 8 a sequence that stands alone in its sub-batch:
//   one larger than a sub-batch, or a match whose source starts in the prefix and ends in the output | 9..12 run-length (offset 1, 2,
//   4) of the sizes of 1..4 | 13 source wholly in the prefix: moved by the stager from `prefix`.
// History: positions are absolute (the tiles' sums start at out_existing_len), so a source in the existing output is classed like any
// other: inside the ring (the stager primes it) or older (class 7).  A job without a prefix gets the records it always got — from the
// instruction stream it always had: the tiles' loop is compiled twice, HIST = false without a word about prefixes, and the kernel takes a
// job to one or the other (with one body and a uniform `if (P)` around the additions the 980-block call took 16.3 ms instead of 16.0:
// profiles/seg_history.txt).
namespace {
template <bool HIST>
__device__ __forceinline__ void seg_records_tiles(const seg_ctx& c, const uint32_t j, const seg_job& sj, const lzf_decompress_job& job, const uint32_t lane,
                                                  uint8_t* const stage, uint16_t* const list) {
    // (as DecodeJob of lzf_copy_helpers.h has them; the view itself moved three instructions here: profiles/copy_stage_one_ring.txt)
    cgu8* __restrict__ in = as_global(job.input);
    gu8* out = as_global(job.out);
    const uint32_t len = (uint32_t)job.input_len;
    const uint32_t cap = job.out_cap > kMaxPosB ? kMaxPosB : (uint32_t)job.out_cap;
    const uint64_t limit = job.output_limit;
    LZF_GLOBAL u32x4* const recs = (LZF_GLOBAL u32x4*)c.recs + sj.rec_off;
    const uint32_t R = c.ring_bytes, kSpan = R / 8u, kAheadB = 3u * kSpan + 64u;
    const uint32_t rb = (uint32_t)(reinterpret_cast<uintptr_t>(job.out) & 15u);
    // the prefix an offset can still reach (decompress.rs:80-99: a source in front of the output continues in the prefix's tail)
    const uint32_t P = HIST ? __builtin_amdgcn_readfirstlane((uint32_t)job.prefix_len) : 0u;
    for (uint32_t t = blockIdx.x; t < sj.ntile; t += gridDim.x) {
        __syncthreads();
        const uint32_t n = tile_enumerate(c, j, t, lane, len, in, stage, list);
        TileCtx tc{t * kSegTile, lds_addr(stage), len, in};
        const uint32_t tbase = c.tile_tok[(size_t)j * c.maxtile + t] * 64u;         // first record of the tile (its batches are padded to 64)
        uint32_t obase = c.tile_out[(size_t)j * c.maxtile + t];
        bool bad = false;
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            const uint32_t nb = n - i0 < 64u ? n - i0 : 64u;
            const bool act = lane < nb;
            Tok k; k.L = 0; k.M = 0; k.off = 0; k.src = 0; k.err = false;
            if (act) k = tile_decode(tc, tc.tstart + list[i0 + lane]);
            const uint32_t tot = k.L + k.M;
            const uint32_t incl = wave_scan_add(tot);
            const uint32_t ob = obase;
            const uint32_t lo = obase + (incl - tot), mo = lo + k.L;
            obase += __builtin_amdgcn_readlane(incl, 63);
            bool ok = act && !k.err;
            if (ok) {
                if (lo > cap || cap - lo < k.L) ok = false;                                   // our buffer (literals)
                else if (k.M && ((uint64_t)mo + k.M > limit || k.off == 0u || (k.off > mo && k.off - mo > P) || cap - mo < k.M)) ok = false;   // :72-74, :83, :84-89, our buffer
            }
            bad = bad || (act && !ok);
            if (ok) {
                if (k.L > 0u && k.L <= 64u) copy_small_gg(out + lo, in + k.src, k.L);       // literals :65-67
                else if (k.L > 64u && k.L <= 256u) copy_medium_gg(out + lo, in + k.src, k.L);
            }
            for (unsigned long long m = __ballot(ok && k.L > 256u); m; m &= m - 1ull) {       // long runs: all lanes
                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                wave_copy_long(out + __builtin_amdgcn_readlane(lo, q), in + __builtin_amdgcn_readlane(k.src, q), __builtin_amdgcn_readlane(k.L, q), lane);
            }
            if (__ballot(bad)) continue;                                                      // (the job is not ours any more: no records needed)
            // ---- levels: which matches of the batch copy from which (see the head of this section)
            const uint32_t M = k.M, off = k.off;
            const bool has = act && M != 0u;
            const uint32_t span = M < off ? M : off;
            const uint32_t s0 = mo - off, e0 = s0 + span;
            uint32_t lvl = has ? 1u : 0u;
            // a source that starts in the prefix (s0 is negative: wrapped) is moved by the stager, which waits for what it needs of the
            // output: it depends on nothing here.  A source in the existing output is a source like any other, only final already.
            bool pre = false;
            if (HIST) pre = has && off > mo;
            const bool dep = has && !pre && e0 > ob;     // the source reaches into the batch
            // (lane values are exchanged by ds_bpermute: no LDS memory, no address arithmetic — every lane is active here)
            auto from_lane = [](uint32_t l, uint32_t v) -> uint32_t { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((l & 63u) << 2), (int)v); };
            if (__any(dep)) {
                const uint32_t endv = act ? mo + M : 0xFFFFFFFFu, mov = act ? mo : 0xFFFFFFFFu;
                uint32_t a = 0, bb = 0;                   // a = #lanes with end <= s0; bb = #lanes with mo < e0
#pragma unroll
                for (uint32_t step = 32u; step; step >>= 1) {
                    if (from_lane(a + step - 1u, endv) <= s0) a += step;
                    if (from_lane(bb + step - 1u, mov) < e0) bb += step;
                }
                const uint32_t ilo = a, ihi = bb - 1u;
                const bool any_dep = dep && bb >= 1u && ilo <= ihi && ihi < lane;
                if (__any(any_dep)) {
                    const bool wide = any_dep && ihi - ilo > 1u;
                    const bool any_wide = __any(wide);
                    for (uint32_t it = 0; it < 64u; ++it) {
                        const uint32_t la = from_lane(ilo, lvl), lb = from_lane(ihi, lvl);
                        uint32_t m = la > lb ? la : lb;
                        if (any_wide) { const uint32_t pm = from_lane(ihi, wave_scan_max(lvl)); if (wide) m = pm; }
                        const uint32_t nl = any_dep ? 1u + m : lvl;
                        const bool ch = nl != lvl;
                        lvl = nl;
                        if (!__any(ch)) break;
                    }
                }
            }
            // ---- sub-batches and classes
            const uint32_t endp = mo + M;
            uint32_t sub = 0, cls = 0;
            uint32_t a = 0, sidx = 0;
            while (a < nb) {
                const uint32_t sob = __builtin_amdgcn_readlane(lo, a);
                const uint32_t bb0 = first_lane(__ballot(lane >= a && lane < nb && endp - sob > kSpan));
                uint32_t e = bb0 < nb ? bb0 : nb;
                // a source that starts in the prefix and ends in the output (the few of a job: they cross one byte boundary) stands alone
                // like a sequence larger than a sub-batch does: the stager copies it once everything in front of it is in HBM
                if (HIST) { const uint32_t bs = first_lane(__ballot(lane >= a && lane < nb && pre && off - mo < M)); if (bs < e) e = bs; }
                const bool giant = e == a;
                if (giant) e = a + 1u;
                const uint32_t oe = __builtin_amdgcn_readlane(endp, e - 1u);
                if (lane >= a && lane < e) {
                    sub = sidx;
                    if (giant) cls = 8u;
                    else if (M != 0u) {
                        // what the ring holds for certain when this sub-batch is resolved: from fill pointer + fetch-ahead - ring on
                        const uint32_t fpw = ((oe + rb + 15u) & ~15u) + kAheadB;
                        const uint32_t lov = fpw > R ? fpw - R : 0u;
                        const uint32_t sy = s0 + rb, dy = mo + rb;
                        const uint32_t di = dy & (R - 1u), si = sy & (R - 1u);
                        const bool wrap = di + M > R || si + M > R;
                        if (pre) cls = 13u;
                        else if (sy < lov) cls = 7u;
                        else if (M > 64u || wrap) cls = 6u;
                        else if (off < M) cls = (off == 1u || off == 2u || off == 4u) ? (M < 8u ? 9u : M <= 16u ? 10u : M <= 32u ? 11u : 12u) : 5u;
                        else cls = M < 8u ? 1u : M <= 16u ? 2u : M <= 32u ? 3u : 4u;
                    }
                }
                a = e; ++sidx;
            }
            // ---- the records of the batch; the lanes behind the tile's last token pad it (an empty sequence at the batch's end)
            {
                const uint32_t last_end = __builtin_amdgcn_readlane(endp, (nb - 1u) & 63u);
                const uint32_t last_sub = __builtin_amdgcn_readlane(sub, (nb - 1u) & 63u);
                u32x4 w;
                w[0] = act ? M : 0u; w[1] = (act ? mo : last_end) + rb;
                // bits 8..15: the resolver's round masks as flags (one v_and + v_cmp each there): 1 four-byte pieces (classes 1, 9),
                // 2 first pair of eight-byte pieces (2-4, 10-12), 4 second pair (3, 4, 11, 12), 8 third and fourth (4, 12),
                // 16 leaves the loop (5, 6), 32 run-length (9-12)
                const uint32_t fl = !act ? 0u : ((cls == 1u || cls == 9u) ? 1u : 0u) | (((cls >= 2u && cls <= 4u) || (cls >= 10u && cls <= 12u)) ? 2u : 0u) |
                                    ((cls == 3u || cls == 4u || cls == 11u || cls == 12u) ? 4u : 0u) | ((cls == 4u || cls == 12u) ? 8u : 0u) |
                                    ((cls == 5u || cls == 6u) ? 16u : 0u) | ((cls >= 9u && cls <= 12u) ? 32u : 0u);
                w[2] = (act ? sub : last_sub) | (fl << 8) | ((act ? lvl : 0u) << 16) | ((act ? cls : 0u) << 24); w[3] = act ? off : 0u;
                recs[tbase + i0 + lane] = w;
            }
        }
        if (__ballot(bad) && lane == 0u) c.st[j].failed = 1u;
    }
}
}  // namespace
__global__ __launch_bounds__(64) void lzf_seg_records_kernel(seg_ctx c) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTileStage];
    __shared__ uint16_t list[kTileTokMax + 64u];
    const uint32_t j = (c.rec_by_len || c.grouped) ? seg_job_of(c, blockIdx.y) : blockIdx.y;
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    // a prefix that an offset can still reach?  (existing output of 65 535 bytes or more hides it: the plan stage has the same rule)
    if (__builtin_amdgcn_readfirstlane((uint32_t)(job.prefix_len != 0 && job.out_existing_len < kSegPrefixReach)))
        seg_records_tiles<true>(c, j, sj, job, lane, stage, list);
    else
        seg_records_tiles<false>(c, j, sj, job, lane, stage, list);
}

}  // namespace lzf
