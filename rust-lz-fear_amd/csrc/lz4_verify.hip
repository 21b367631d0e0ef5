// lz4_verify.hip — lzf_decompress_verify_batch: does every job decode to exactly the bytes its `out` already holds?  Nothing is
// decoded and nothing but the results is written (lzf_verify_rules.h has the argument and the one definition of the result).
//
// One wavefront per job, and lzf_decoded_size_kernel's walk (lz4_decoded_size.hip): the same staged chunk of 64 x S compressed
// bytes, the same lane-parallel parse (lz4_decompress_parse_phase.inc), 64 tokens per round, the same scan of L + M and the same
// three position checks with their ballot.  Behind the checks of a clean round come the compares, every sequence at the position
// the scan gave it:
//   a literal run or a match of up to kOwn bytes below out_cap is compared by its own lane (16 bytes a step, the tail by one
//   overlapping load: nothing outside the run is read; no branch on a loaded byte, so both runs' loads are in flight together);
//   longer ones are compared by the whole wave, one after the other in stream order, 16 bytes a lane and 4 KiB a step;
//   the token that reaches beyond a chunk, which the walk takes ahead of its parse, is compared wave-wide too.
// Literals are read from the input in HBM / L2 (the chunk was staged from there a moment ago), the expected bytes and the match
// sources from `out`, a source in front of out[0] from the prefix's tail.  No load leaves input[0, input_len), prefix[0, prefix_len)
// or out[0, out_cap): 16-byte loads only where 16 bytes remain.  After the first mismatch the walk goes on without comparing —
// the status still has to come out of the whole block, and it precedes the bytes.
#include "lzf_seg_common.h"
#include "lzf_parse_helpers.h"
#include "lzf_verify_rules.h"

namespace lzf {

namespace {
static_assert(lzf_verify::kMaxLen == kMaxPosB && lzf_verify::MISMATCH == LZF_MISMATCH && lzf_verify::CONTRACT == LZF_CONTRACT, "lzf_verify_rules.h restates these");
constexpr uint32_t kOwn = 64;            // bytes of a run a lane compares by itself

// index of the first non-zero byte of x (x != 0)
__device__ __forceinline__ uint32_t first_byte16(u32x4 x) {
    return x[0] ? (uint32_t)__builtin_ctz(x[0]) >> 3 : x[1] ? 4u + ((uint32_t)__builtin_ctz(x[1]) >> 3)
         : x[2] ? 8u + ((uint32_t)__builtin_ctz(x[2]) >> 3) : 12u + ((uint32_t)__builtin_ctz(x[3]) >> 3);
}
__device__ __forceinline__ bool any16(u32x4 x) { return (x[0] | x[1] | x[2] | x[3]) != 0u; }

// One lane: the first i < n with a[i] != b[i], or n.  Reads a[0, n) and b[0, n) and nothing else: a piece at the front and one that
// ends with the run (they may overlap: the same bytes), whole pieces in between from 33 bytes on.  No branch depends on a loaded
// byte — the smallest index is kept with selects — so the loads of a lane's literal run and of its match are all in flight before
// the first of them is waited for: a round costs one trip to memory, not one per run.
__device__ __forceinline__ uint32_t lane_first_diff(cgu8* a, cgu8* b, uint32_t n) {
    uint32_t d = n;
    auto keep = [&](bool differs, uint32_t at) { d = differs && at < d ? at : d; };
    if (n >= 16u) {
        const u32x4 x = ld16(a) ^ ld16(b), y = ld16(a + n - 16u) ^ ld16(b + n - 16u);
        keep(any16(x), any16(x) ? first_byte16(x) : 0u);
        keep(any16(y), any16(y) ? n - 16u + first_byte16(y) : 0u);
        for (uint32_t i = 16u; i + 16u < n; i += 16u) {
            const u32x4 z = ld16(a + i) ^ ld16(b + i);
            keep(any16(z), any16(z) ? i + first_byte16(z) : 0u);
        }
    } else if (n >= 8u) {
        const uint64_t x = ld8(a) ^ ld8(b), y = ld8(a + n - 8u) ^ ld8(b + n - 8u);
        keep(x != 0ull, x ? (uint32_t)__builtin_ctzll(x) >> 3 : 0u);
        keep(y != 0ull, y ? n - 8u + ((uint32_t)__builtin_ctzll(y) >> 3) : 0u);
    } else if (n >= 4u) {
        const uint32_t x = ld4(a) ^ ld4(b), y = ld4(a + n - 4u) ^ ld4(b + n - 4u);
        keep(x != 0u, x ? (uint32_t)__builtin_ctz(x) >> 3 : 0u);
        keep(y != 0u, y ? n - 4u + ((uint32_t)__builtin_ctz(y) >> 3) : 0u);
    } else {
        for (uint32_t i = 0; i < n; ++i) keep(a[i] != b[i], i);
    }
    return d;
}

// The whole wave, uniform arguments: the first i < n with a[i] != b[i], or n (uniform).  4 KiB a step while that much remains
// (four loads of each side in flight per lane), then 1 KiB a step, the last piece bytewise.
__device__ __forceinline__ uint64_t wave_first_diff(cgu8* a, cgu8* b, uint64_t n, uint32_t lane) {
    uint64_t base = 0;
    for (; n - base >= 4096u; base += 4096u) {
        u32x4 x[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) x[k] = ld16(a + base + k * 1024u + lane * 16u) ^ ld16(b + base + k * 1024u + lane * 16u);
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const unsigned long long bal = __ballot(any16(x[k]));
            if (bal) {
                const uint32_t l = first_lane(bal);
                return base + k * 1024u + l * 16u + (uint32_t)__builtin_amdgcn_readlane(any16(x[k]) ? first_byte16(x[k]) : 0u, l);
            }
        }
    }
    for (; base < n; base += 1024u) {
        const uint64_t i = base + lane * 16u;
        uint32_t d = 16u;
        if (n - base >= 16u * (lane + 1u)) {
            const u32x4 x = ld16(a + i) ^ ld16(b + i);
            if (any16(x)) d = first_byte16(x);
        } else if (i < n) {
            const uint32_t m = (uint32_t)(n - i);
            for (uint32_t t = 0; t < m; ++t) if (a[i + t] != b[i + t]) { d = t; break; }
        }
        const unsigned long long bal = __ballot(d < 16u);
        if (bal) {
            const uint32_t l = first_lane(bal);
            return base + l * 16u + (uint32_t)__builtin_amdgcn_readlane(d, l);
        }
    }
    return n;
}

// A match of nm compared bytes at output position mo with offset off (off - mo <= plen, lzf_size::check): the first i < nm at which
// the source byte differs from out[mo + i], or nm.  The source starts in the prefix's tail where off > mo and goes on at out[0].
// CMP: lane_first_diff for one lane, wave_first_diff with uniform arguments.
template <class CMP>
__device__ __forceinline__ uint64_t match_first_diff(cgu8* pre, uint64_t plen, cgu8* out, uint64_t mo, uint32_t off, uint64_t nm, CMP cmp) {
    uint64_t done = 0;
    if ((uint64_t)off > mo) {
        const uint64_t back = (uint64_t)off - mo, np = nm < back ? nm : back;
        const uint64_t d = cmp(pre + (plen - back), out + mo, np);
        if (d < np) return d;
        done = np;
    }
    if (done < nm) return done + cmp(out + (mo + done - off), out + (mo + done), nm - done);
    return nm;
}

// One round of up to 64 clean sequences, lane j's with its literals at input position lit_at and output position lpos: the smallest
// failing position below cap, or kNone (uniform).  Positions rise with the lane, so the first lane that found something holds the
// round's smallest own-lane position; runs longer than kOwn follow, wave-wide, in stream order.  Shared by the one-wave kernel and
// the tile kernel of the latency class.
__device__ __forceinline__ uint64_t round_first_mismatch(cgu8* in, cgu8* pre, uint64_t plen, cgu8* out, uint64_t cap, uint32_t lane, bool act,
                                                         uint32_t lit_at, uint32_t sL, uint64_t sM, uint32_t off, bool has, uint64_t lpos) {
    auto lane_cmp = [](cgu8* a, cgu8* b, uint64_t n) -> uint64_t { return lane_first_diff(a, b, (uint32_t)n); };
    auto wave_cmp = [&](cgu8* a, cgu8* b, uint64_t n) -> uint64_t { return wave_first_diff(a, b, n, lane); };
    const uint64_t mo = lpos + sL;
    const uint32_t nl = act ? (uint32_t)lzf_verify::below_cap(lpos, sL, cap) : 0u;
    const uint64_t nm = act && has ? lzf_verify::below_cap(mo, sM, cap) : 0ull;
    const bool longl = nl > kOwn, longm = nm > kOwn;
    uint64_t mine = lzf_verify::kNone;
    if (nl && !longl) {
        const uint32_t d = lane_first_diff(in + lit_at, out + lpos, nl);
        if (d < nl) mine = lpos + d;
    }
    if (nm && !longm) {                  // (not behind the literals' answer: its loads go out with theirs)
        const uint64_t d = match_first_diff(pre, plen, out, mo, off, nm, lane_cmp);
        if (d < nm && mine == lzf_verify::kNone) mine = mo + d;
    }
    uint64_t best = lzf_verify::kNone;
    const uint32_t f = first_lane(__ballot(mine != lzf_verify::kNone));
    if (f < 64u) best = readlane64(mine, f);
    for (unsigned long long m = __ballot(longl || longm); m; m &= m - 1ull) {
        const uint32_t l = (uint32_t)__builtin_ctzll(m);
        const uint64_t p = readlane64(lpos, l);
        if (p >= best) break;                                        // everything from here on lies behind the finding
        const uint32_t L = (uint32_t)__builtin_amdgcn_readlane(sL, l);
        const uint64_t n1 = (uint32_t)__builtin_amdgcn_readlane(nl, l);
        if (n1 > kOwn) {
            const uint64_t d = wave_first_diff(in + (uint32_t)__builtin_amdgcn_readlane(lit_at, l), out + p, n1, lane);
            if (d < n1) { best = p + d; break; }
        }
        const uint64_t n2 = readlane64(nm, l);
        if (n2 > kOwn && p + L < best) {
            const uint64_t d = match_first_diff(pre, plen, out, p + L, (uint32_t)__builtin_amdgcn_readlane(off, l), n2, wave_cmp);
            if (d < n2) { best = p + L + d; break; }
        }
    }
    return best;
}
}  // namespace

template <int S, int TOKCAP, bool SKIP>
__global__ __launch_bounds__(64) void lzf_verify_kernel(const lzf_decompress_job* __restrict__ jobs, lzf_job_result* __restrict__ results,
                                                        uint32_t n_jobs, uint32_t* __restrict__ ticket, const uint32_t* __restrict__ perm,
                                                        const seg_job* __restrict__ done) {
    constexpr bool STAGE = true;
    constexpr uint32_t kChunk = 64u * S;               // compressed bytes whose tokens one parse covers
    constexpr uint32_t kCB = kChunk + 64u;             // staged bytes: the chunk + room for token bodies
    static_assert(kChunk <= 65536, "token positions are stored as u16 offsets into the chunk");
    static_assert(kCB % 16 == 0, "chunk buffer is filled in 16-byte pieces");
    __shared__ __attribute__((aligned(16))) uint8_t cbuf[kCB];
    __shared__ __attribute__((aligned(16))) uint8_t nxt[kChunk];
    constexpr uint32_t kExStride = (uint32_t)S + 4u;
    constexpr uint32_t kTokBytes = ((uint32_t)TOKCAP + 64u) * 2u;
    constexpr uint32_t kExBytes = 64u * kExStride;
    __shared__ __attribute__((aligned(16))) uint8_t tokex[kTokBytes > kExBytes ? kTokBytes : kExBytes];
    uint16_t* const toks = reinterpret_cast<uint16_t*>(tokex);
    const uint32_t lane = threadIdx.x;
    const uint32_t cbuf_a = lds_addr(cbuf), nxt_a = lds_addr(nxt), ex_a = lds_addr(tokex);
    auto wave_cmp = [&](cgu8* a, cgu8* b, uint64_t n) -> uint64_t { return wave_first_diff(a, b, n, lane); };

    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1u);
        t = rfl(t);
        if (t >= n_jobs) break;
        const uint32_t jid = perm ? perm[t] : t;       // (perm: the jobs longest input first, so that the launch does not end on a long one)
        if (SKIP && done[jid].done) continue;          // finished by the latency class below (uniform over the wave)
        const long long t_start = clock64();
        cgu8* __restrict__ in = as_global(jobs[jid].input);
        cgu8* pre = as_global(jobs[jid].prefix);
        cgu8* out = as_global((const uint8_t*)jobs[jid].out);      // history and the expected bytes: read, never written
        const uint64_t input_len = jobs[jid].input_len, plen = jobs[jid].prefix_len, existing = jobs[jid].out_existing_len;
        const uint64_t limit = jobs[jid].output_limit, cap = jobs[jid].out_cap;
        int status = LZF_OK;
        uint64_t o = existing;                         // output.len()
        uint64_t bad = lzf_verify::kNone;              // the smallest failing position so far (uniform)
        if (input_len >= kMaxPosB || existing >= kMaxPosB || plen >= kMaxPosB) {
            status = LZF_CONTRACT;
        } else {
            const uint32_t len = (uint32_t)input_len;
            const DecodeJob jv{in, nullptr, nullptr, len, 0u, 0u, 0ull, 0u};      // what the parse stage reads of a job: its input
            uint32_t cstart = 0;                       // a true token position (or len)
            // readers of the input in HBM / L2 for the one token looked at ahead of a chunk (wave-uniform addresses)
            auto g1 = [&](uint32_t p) -> uint32_t { return (uint32_t)in[p]; };
            auto g4 = [&](uint32_t p) -> uint32_t {
                if (len - p >= 4u) return ld4(in + p);
                uint32_t v = 0;
                for (uint32_t i = 0; p + i < len; ++i) v |= (uint32_t)in[p + i] << (8u * i);
                return v;
            };
            auto gff = [&](uint32_t p) -> uint32_t {           // 0xFF bytes from p on, eight at a time
                uint32_t n = 0;
                while (len - (p + n) >= 8u && ld8(in + p + n) == ~0ull) n += 8u;
                while (p + n < len && in[p + n] == 255u) ++n;
                return n;
            };
            while (cstart < len && status == LZF_OK) {
                // a token that reaches beyond the chunk: decoded ahead of the parse as in the size kernel, compared by the whole wave
                {
                    const uint32_t w = g4(cstart);
                    if ((w & 0xFFF0u) == 0xFFF0u || (w & 15u) == 15u) {
                        lzf_size::Seq s;
                        uint32_t next;
                        if (!lzf_size::decode_token(cstart, len, g4, g1, gff, s, next)) { status = LZF_UNEXPECTED_END; break; }
                        if (next - cstart > kChunk) {
                            const int code = s.has ? lzf_size::check(o + s.L, s.M, s.off, plen, limit) : LZF_OK;
                            if (code != LZF_OK) { status = code; break; }
                            if (bad == lzf_verify::kNone) {
                                const uint64_t nl = lzf_verify::below_cap(o, s.L, cap);
                                const uint64_t d = wave_first_diff(in + lzf_verify::literals_at(cstart, s.L), out + o, nl, lane);
                                if (d < nl) bad = o + d;
                            }
                            if (bad == lzf_verify::kNone && s.has) {
                                const uint64_t mo = o + s.L, nm = lzf_verify::below_cap(mo, s.M, cap);
                                const uint64_t d = match_first_diff(pre, plen, out, mo, s.off, nm, wave_cmp);
                                if (d < nm) bad = mo + d;
                            }
                            o = lzf_size::advance(o, s);
                            cstart = next;
                            continue;
                        }
                    }
                }
#define LZF_TOK_T uint16_t
#define LZF_THOP_RECORD thop_loop_record
#include "lz4_decompress_parse_phase.inc"
#undef LZF_THOP_RECORD
#undef LZF_TOK_T
                // the staged chunk's readers, and how many bytes from p on are 0xFF (no further than len); here the run ends within a chunk
                auto rdb = [&](uint32_t q) -> uint32_t { return sb.rdb(q); };
                auto rd4 = [&](uint32_t q) -> uint32_t { return sb.rd4(q); };
                auto ffrun = [&](uint32_t p) -> uint32_t {
                    uint32_t n = 0;
                    while (p + n < len && rdb(p + n) == 255u) ++n;
                    return n;
                };
                for (uint32_t tidx = 0; tidx < Tc; tidx += kWave) {
                    const bool act = lane < Tc - tidx;
                    // lanes past the list decode the round's first token again (masked off below)
                    const uint32_t tp = cstart + toks[act ? tidx + lane : tidx];
                    lzf_size::Seq s;
                    uint32_t next;
                    (void)lzf_size::decode_token(tp, len, rd4, rdb, ffrun, s, next);     // listed tokens are whole: the parse read them
                    const uint64_t tot = act ? (uint64_t)s.L + s.M : 0ull;
                    // the size kernel's rule for the 32-bit scan.  It looks at M alone although L + M is scanned, and the compare addresses
                    // below come out of this scan: an L of 2^24 needs more than 64 K length bytes, so such a token is longer than a chunk
                    // and was taken ahead of the parse above, never listed
                    const bool wide = __ballot(act && s.M >= (1ull << 24)) != 0ull;
                    const uint64_t incl = wave_scan_add64(tot, wide);
                    const uint64_t lpos = o + (incl - tot), mo = lpos + s.L;             // output.len() in front of / behind this lane's literals
                    const int code = act && s.has ? lzf_size::check(mo, s.M, s.off, plen, limit) : LZF_OK;
                    const uint32_t e = first_lane(__ballot(code != LZF_OK));
                    if (e < 64u) { status = __builtin_amdgcn_readlane(code, e); break; }
                    if (bad == lzf_verify::kNone)                                        // the round is clean: every lane's sequence at its own position
                        bad = round_first_mismatch(in, pre, plen, out, cap, lane, act, lzf_verify::literals_at(tp, s.L), s.L, s.M, s.off, s.has, lpos);
                    o += readlane64(incl, 63);
                }
                if (status == LZF_OK && cerr != LZF_OK) status = cerr;
                cstart = cend;
            }
        }
        if (lane == 0) {
            const lzf_verify::Verdict v = lzf_verify::conclude(status, o, bad, cap);
            results[jid].out_len = v.out_len;
            results[jid].status = v.status;
            results[jid].reserved = (uint32_t)((clock64() - t_start) >> 10);   // diagnostic: shader kilo-cycles spent on this job
        }
    }
}

template __global__ void lzf_verify_kernel<48, 768, false>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*, const uint32_t*, const seg_job*);
template __global__ void lzf_verify_kernel<48, 768, true>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*, const uint32_t*, const seg_job*);

// ---- the latency class: ONE BLOCK VERIFIED BY MANY WAVEFRONTS ----------------------------------------------------------------------
// Behind the size call's class (plan, parse, seam, lzf_size_tile_kernel: lz4_decoded_size_seg.hip):
//   finish   lzf_size_finish_kernel's scan and checks, and every tile's base position (the output position of its first token,
//            existing output included) kept in tile_base; a job of clean tiles gets done = 1 and its length in results[].out_len
//   tile     one wavefront per 2 KiB tile of a done job: the tile's true tokens again, 64 per round, each sequence compared at
//            base + tile-relative position (round_first_mismatch: the one-wave kernel's compares); the smallest failing position of
//            a job by a 64-bit atomic minimum in job_min (it starts as kNone)
//   end      one thread per job: the verdict of a done job from its length, job_min and out_cap (lzf_verify::conclude)
// Everything else — every error status, sizes outside the window — is left, untouched, to lzf_verify_kernel<.., SKIP>, last.
__global__ __launch_bounds__(64) void lzf_verify_finish_kernel(seg_ctx c, uint64_t* __restrict__ tile_base) {
    const uint32_t j = blockIdx.x;
    if (j >= c.n_jobs) return;
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    const uint64_t existing = job.out_existing_len, plen = job.prefix_len, limit = job.output_limit;
    const LZF_GLOBAL u32x4* const TS = (const LZF_GLOBAL u32x4*)c.tile_sum + (size_t)j * c.maxtile;
    uint64_t* const TB = tile_base + (size_t)j * c.maxtile;
    uint64_t total = 0;                                // the sums of the tiles in front of the round
    bool bad = false;
    for (uint32_t t0 = 0; t0 < sj.ntile; t0 += 64u) {
        const uint32_t t = t0 + lane;
        const u32x4 v = t < sj.ntile ? TS[t] : u32x4{0u, 0u, 0u, 0u};
        const lzf_size::TileSum ts{v[0], v[1], v[2], v[3]};
        const uint32_t ilo = wave_scan_add(ts.sum & 0xFFFFu), ihi = wave_scan_add(ts.sum >> 16);      // (as lzf_size_finish_kernel)
        const uint64_t incl = (uint64_t)ilo + ((uint64_t)ihi << 16);
        const uint64_t base = existing + total + (incl - ts.sum);
        bad = bad || !lzf_size::clean(ts, base, plen, limit);
        if (t < sj.ntile) TB[t] = base;
        total += (uint64_t)(uint32_t)__builtin_amdgcn_readlane(ilo, 63) + ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(ihi, 63) << 16);
    }
    if (__ballot(bad) != 0ull || total > 0xFFFFFFFFull) return;                  // not clean: the one-wave kernel's job
    if (lane == 0u) {
        c.results[j].out_len = existing + total;       // (the end kernel turns it into the verdict)
        c.results[j].status = LZF_OK;
        c.results[j].reserved = sj.ntile;              // diagnostic: the tiles the job was verified in
        c.st[j].done = 1u;
    }
}

__global__ __launch_bounds__(64) void lzf_verify_tile_kernel(seg_ctx c, const uint64_t* __restrict__ tile_base, unsigned long long* __restrict__ job_min) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kTileStage];
    __shared__ uint16_t list[kTileTokMax + 64u];
    const uint32_t j = seg_job_of(c, blockIdx.y);
    const seg_job sj = c.st[j];
    if (!sj.done) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    cgu8* __restrict__ in = as_global(job.input);
    cgu8* pre = as_global(job.prefix);
    cgu8* out = as_global((const uint8_t*)job.out);
    const uint32_t len = (uint32_t)job.input_len;
    const uint64_t plen = job.prefix_len, cap = job.out_cap;
    for (uint32_t t = blockIdx.x; t < sj.ntile; t += gridDim.x) {
        __syncthreads();
        const uint32_t n = tile_enumerate(c, j, t, lane, len, in, stage, list);
        const TileCtx tc{t * kSegTile, lds_addr(stage), len, in};
        uint64_t pos = tile_base[(size_t)j * c.maxtile + t];         // output position of the round's first sequence
        if (pos >= cap) continue;                                    // (positions rise: nothing of this tile is compared)
        uint64_t bad = lzf_verify::kNone;
        for (uint32_t i0 = 0; i0 < n && bad == lzf_verify::kNone; i0 += 64u) {
            const bool act = i0 + lane < n;
            Tok k; k.L = 0; k.M = 0; k.off = 0; k.src = 0; k.err = false;
            if (act) k = tile_decode<true>(tc, tc.tstart + list[i0 + lane]);      // (a done job: every token decodes, lengths below the clamp)
            const uint32_t tot = k.L + k.M;
            uint64_t incl;
            if (__ballot(tot >= (1u << 24)) == 0ull) incl = wave_scan_add(tot);
            else incl = (uint64_t)wave_scan_add(tot & 0xFFFFu) + ((uint64_t)wave_scan_add(tot >> 16) << 16);
            bad = round_first_mismatch(in, pre, plen, out, cap, lane, act, k.src, k.L, k.M, k.off, k.M != 0u, pos + (incl - tot));
            pos += readlane64(incl, 63);
        }
        if (bad != lzf_verify::kNone && lane == 0u) atomicMin(&job_min[j], (unsigned long long)bad);
    }
}

__global__ __launch_bounds__(256) void lzf_verify_end_kernel(seg_ctx c, const unsigned long long* __restrict__ job_min) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= c.n_jobs || !c.st[j].done) return;
    const lzf_verify::Verdict v = lzf_verify::conclude(LZF_OK, c.results[j].out_len, job_min[j], c.jobs[j].out_cap);
    c.results[j].out_len = v.out_len;
    c.results[j].status = v.status;
}

}  // namespace lzf
