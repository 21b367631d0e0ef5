// lz4_decode_head.hip — lzf_decompress_head_batch: the first bytes of every job's block, out_cap being the target at which the
// decode stops (lzf_head_rules.h has the rule and the one definition of the result).
//
// One wavefront per job, jobs drawn from a counter, and lzf_decoded_size_kernel's walk (lz4_decoded_size.hip): the same staged
// chunk of 64 x S compressed bytes, the same lane-parallel parse (lz4_decompress_parse_phase.inc), 64 tokens per round, the same
// scan of L + M and the same three position checks with their ballot.  What is added:
//   the stop   a lane whose sequence starts at or beyond the target is switched off before the checks (positions rise with the
//              lane: the live lanes are a prefix of the round), and a round with such a lane is the job's last: no further chunk is
//              staged, so a 64-byte head of a 4 MiB block costs one chunk;
//   the copies behind the checks of a clean round, straight into `out` (no ring: a head is short), clamped by lzf_head::clamp:
//     1. every lane moves its own literal run of up to kOwn bytes from the input, and its own match of up to kOwn bytes where the
//        source lies wholly in front of the round's first byte or wholly in the prefix — nothing this round writes;
//     2. longer literal runs go wave-wide, 16 bytes a lane;
//     3. the matches left over — a source inside the round, a source that crosses out[0], anything longer than kOwn — follow one
//        after the other in stream order, wave-wide: a period of 16 and more in pieces of `offset` bytes (a piece never
//        reads what it writes), a shorter period from the pattern held in registers.
//   In front of every step that reads what the wave wrote, the wave waits for its own stores (wave_store_fence).
// A token that reaches beyond a chunk is taken ahead of the parse as in the size kernel and copied wave-wide.
// No load leaves input[0, input_len), prefix[0, prefix_len) or out[0, target), no store leaves out[out_existing_len, target): 16-byte
// pieces only where 16 bytes remain, the ends two-ended or bytewise.
#include "lzf_device.h"
#include "kernels.h"
#include "lzf_copy_helpers.h"
#include "lzf_parse_helpers.h"
#include "lzf_head_rules.h"

namespace lzf {

namespace {
static_assert(lzf_head::kMaxLen == kMaxPosB && lzf_head::CONTRACT == LZF_CONTRACT, "lzf_head_rules.h restates these");
constexpr uint32_t kOwn = 64;            // bytes of a run a lane moves by itself
constexpr uint32_t kStep = 1024;         // bytes the wave moves per step: 16 a lane

__device__ __forceinline__ void st8(gu8* p, uint64_t v) { reinterpret_cast<LZF_GLOBAL U8B*>(p)->v = v; }
__device__ __forceinline__ void st4(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL U4B*>(p)->v = v; }
__device__ __forceinline__ void st2(gu8* p, uint32_t v) { reinterpret_cast<LZF_GLOBAL U2B*>(p)->v = (uint16_t)v; }

// One lane: dst[0, n) = src[0, n), n <= kOwn, the ranges apart.  Reads src[0, n) and writes dst[0, n) and nothing else: a piece at
// the front and one that ends with the run (they may overlap: the same bytes), whole pieces in between from 33 bytes on.
__device__ __forceinline__ void lane_copy(gu8* dst, cgu8* src, uint32_t n) {
    if (n >= 16u) {
        const u32x4 a = ld16(src), z = ld16(src + n - 16u);
        u32x4 m0 = a, m1 = a;
        if (n > 32u) m0 = ld16(src + 16u);
        if (n > 48u) m1 = ld16(src + 32u);
        st16(dst, a);
        if (n > 32u) st16(dst + 16u, m0);
        if (n > 48u) st16(dst + 32u, m1);
        st16(dst + n - 16u, z);
    } else if (n >= 8u) {
        const uint64_t a = ld8(src), z = ld8(src + n - 8u);
        st8(dst, a); st8(dst + n - 8u, z);
    } else if (n >= 4u) {
        const uint32_t a = ld4(src), z = ld4(src + n - 4u);
        st4(dst, a); st4(dst + n - 4u, z);
    } else if (n >= 2u) {
        const uint32_t a = ld2(src), z = ld2(src + n - 2u);
        st2(dst, a); st2(dst + n - 2u, z);
    } else if (n == 1u) {
        dst[0] = src[0];
    }
}

// The whole wave, uniform arguments: dst[0, n) = src[0, n), the ranges apart and the source written (and waited for) before the call.
__device__ __forceinline__ void wave_copy_apart(gu8* dst, cgu8* src, uint64_t n, uint32_t lane) {
    uint64_t base = 0;
    for (; n - base >= kStep; base += kStep) st16(dst + base + lane * 16u, ld16(src + base + lane * 16u));
    const uint32_t rest = (uint32_t)(n - base), whole = rest & ~15u;
    if (lane * 16u < whole) st16(dst + base + lane * 16u, ld16(src + base + lane * 16u));
    if (lane < rest - whole) dst[base + whole + lane] = src[base + whole + lane];
}

// The whole wave, uniform arguments: the first nm bytes of a match at output position mo with offset off (off - mo <= plen,
// lzf_size::check).  Everything in front of mo is written and waited for.  The source starts in the prefix's tail where off > mo
// and goes on at out[0]; where the match overlaps itself (off < nm) it is moved in pieces that end in front of what they write,
// with a wait in between — or, for a period below 16, from the period's bytes in two registers, without further loads.
__device__ __forceinline__ void wave_match(gu8* out, cgu8* pre, uint64_t plen, uint64_t mo, uint32_t off, uint64_t nm, uint32_t lane) {
    uint64_t done = 0;
    if ((uint64_t)off > mo) {
        const uint64_t back = (uint64_t)off - mo, np = nm < back ? nm : back;
        wave_copy_apart(out + mo, pre + (plen - back), np, lane);
        done = np;
        if (done == nm) return;
        wave_store_fence();
    }
    if (off >= 16u) {
        while (done < nm) {
            const uint64_t left = nm - done;
            const uint32_t w = left < off ? (uint32_t)left : off;
            wave_copy_apart(out + mo + done, (cgu8*)out + (mo + done - off), w, lane);
            done += w;
            if (done < nm) wave_store_fence();
        }
        return;
    }
    // the period: out[mo + done - off, mo + done), byte k in bits 8k of (lo, hi); every lane reads the same addresses
    cgu8* const p = (cgu8*)out + (mo + done - off);
    uint64_t lo = 0, hi = 0;
    for (uint32_t k = 0; k < off; ++k) {
        const uint64_t b = p[k];
        if (k < 8u) lo |= b << (8u * k); else hi |= b << (8u * (k - 8u));
    }
    gu8* const d = out + mo + done;
    const uint64_t left = nm - done;
    uint32_t pb = 0;                                   // base % off
    for (uint64_t base = 0; base < left; base += kStep, pb = (pb + kStep) % off) {
        const uint64_t i0 = base + lane * 16u;
        if (i0 >= left) break;
        uint32_t ph = (pb + lane * 16u) % off;
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 16u; ++j) {
            const uint32_t b = (uint32_t)((ph < 8u ? lo >> (8u * ph) : hi >> (8u * (ph - 8u))) & 255ull);
            v[j >> 2] |= b << (8u * (j & 3u));
            ph = ph + 1u == off ? 0u : ph + 1u;
        }
        if (left - i0 >= 16u) st16(d + i0, v);
        else {
#pragma unroll
            for (uint32_t j = 0; j < 15u; ++j) if (i0 + j < left) d[i0 + j] = (uint8_t)(v[j >> 2] >> (8u * (j & 3u)));
        }
    }
}
}  // namespace

template <int S, int TOKCAP>
__global__ __launch_bounds__(64) void lzf_decode_head_kernel(const lzf_decompress_job* __restrict__ jobs, lzf_job_result* __restrict__ results,
                                                             uint32_t n_jobs, uint32_t* __restrict__ ticket) {
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

    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1u);
        t = rfl(t);
        if (t >= n_jobs) break;
        const uint32_t jid = t;                        // (no launch order: a job costs what its target asks for, not what its input holds)
        const long long t_start = clock64();
        cgu8* __restrict__ in = as_global(jobs[jid].input);
        cgu8* pre = as_global(jobs[jid].prefix);
        gu8* out = as_global(jobs[jid].out);
        const uint64_t input_len = jobs[jid].input_len, plen = jobs[jid].prefix_len, existing = jobs[jid].out_existing_len;
        const uint64_t limit = jobs[jid].output_limit, cap = jobs[jid].out_cap;      // cap: the target
        int status = LZF_OK;
        uint64_t o = existing;                         // output.len()
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
            // the walk ends in front of the first sequence at or beyond the target: nothing of it is read
            while (cstart < len && status == LZF_OK && !lzf_head::stops(o, cap)) {
                // a token that reaches beyond the chunk: decoded ahead of the parse as in the size kernel, moved by the whole wave
                {
                    const uint32_t w = g4(cstart);
                    if ((w & 0xFFF0u) == 0xFFF0u || (w & 15u) == 15u) {
                        lzf_size::Seq s;
                        uint32_t next;
                        if (!lzf_size::decode_token(cstart, len, g4, g1, gff, s, next)) { status = LZF_UNEXPECTED_END; break; }
                        if (next - cstart > kChunk) {
                            const int code = s.has ? lzf_size::check(o + s.L, s.M, s.off, plen, limit) : LZF_OK;
                            if (code != LZF_OK) { status = code; break; }
                            const lzf_head::Clamp c = lzf_head::clamp(o, s, cap);
                            wave_copy_apart(out + o, in + lzf_head::literals_at(cstart, s.L), c.nl, lane);
                            wave_store_fence();
                            if (c.nm) {
                                wave_match(out, pre, plen, o + s.L, s.off, c.nm, lane);
                                wave_store_fence();
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
                bool stopped = false;
                for (uint32_t tidx = 0; tidx < Tc; tidx += kWave) {
                    const bool listed = lane < Tc - tidx;
                    // lanes past the list decode the round's first token again (masked off below)
                    const uint32_t tp = cstart + toks[listed ? tidx + lane : tidx];
                    lzf_size::Seq s;
                    uint32_t next;
                    (void)lzf_size::decode_token(tp, len, rd4, rdb, ffrun, s, next);     // listed tokens are whole: the parse read them
                    const uint64_t tot = listed ? (uint64_t)s.L + s.M : 0ull;
                    // the size kernel's rule for the 32-bit scan (an L of 2^24 needs more than 64 K length bytes: such a token is longer
                    // than a chunk and was taken ahead of the parse above, never listed)
                    const bool wide = __ballot(listed && s.M >= (1ull << 24)) != 0ull;
                    const uint64_t incl = wave_scan_add64(tot, wide);
                    const uint64_t lpos = o + (incl - tot), mo = lpos + s.L;             // output.len() in front of / behind this lane's literals
                    const bool act = listed && !lzf_head::stops(lpos, cap);              // (positions rise: the live lanes come first)
                    const int code = act && s.has ? lzf_size::check(mo, s.M, s.off, plen, limit) : LZF_OK;
                    const uint32_t e = first_lane(__ballot(code != LZF_OK));
                    if (e < 64u) { status = __builtin_amdgcn_readlane(code, e); break; }
                    // the round is clean: the copies
                    lzf_head::Clamp c = lzf_head::clamp(lpos, s, cap);
                    if (!act) { c.nl = 0u; c.nm = 0ull; }
                    const uint32_t lit_at = lzf_head::literals_at(tp, s.L);
                    const bool from_pre = (uint64_t)s.off > mo;                          // the source starts in the prefix's tail
                    const uint64_t back = from_pre ? (uint64_t)s.off - mo : 0ull;
                    // a match nothing of this round feeds: wholly in the prefix, or ending in front of the round's first byte
                    const bool own_m = c.nm != 0ull && c.nm <= kOwn && (from_pre ? c.nm <= back : mo - s.off + c.nm <= o);
                    if (__ballot(own_m) != 0ull) wave_store_fence();                     // their sources: what earlier rounds wrote
                    if (c.nl != 0u && c.nl <= kOwn) lane_copy(out + lpos, in + lit_at, c.nl);
                    if (own_m) lane_copy(out + mo, from_pre ? pre + (plen - back) : (cgu8*)out + (mo - s.off), (uint32_t)c.nm);
                    for (unsigned long long m = __ballot(c.nl > kOwn); m; m &= m - 1ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(m);
                        wave_copy_apart(out + readlane64(lpos, l), in + (uint32_t)__builtin_amdgcn_readlane(lit_at, l),
                                        (uint32_t)__builtin_amdgcn_readlane(c.nl, l), lane);
                    }
                    const unsigned long long later = __ballot(c.nm != 0ull && !own_m);
                    if (later) wave_store_fence();
                    for (unsigned long long m = later; m; m &= m - 1ull) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(m);
                        wave_match(out, pre, plen, readlane64(mo, l), (uint32_t)__builtin_amdgcn_readlane(s.off, l), readlane64(c.nm, l), lane);
                        wave_store_fence();
                    }
                    o += readlane64(incl, 63);
                    if (__ballot(listed && !act) != 0ull) { stopped = true; break; }     // (o is at or beyond the target now)
                }
                if (status == LZF_OK && !stopped && !lzf_head::stops(o, cap) && cerr != LZF_OK) status = cerr;
                cstart = cend;
            }
        }
        if (lane == 0) {
            results[jid].out_len = status == LZF_OK ? lzf_head::reported(o, cap, existing) : o;
            results[jid].status = status;
            results[jid].reserved = (uint32_t)((clock64() - t_start) >> 10);   // diagnostic: shader kilo-cycles spent on this job
        }
    }
}

template __global__ void lzf_decode_head_kernel<48, 768>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*);

}  // namespace lzf
