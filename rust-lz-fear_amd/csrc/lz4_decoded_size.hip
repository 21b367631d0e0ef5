// lz4_decoded_size.hip — lzf_decompressed_size_batch: the status and output.len() of raw::decompress_raw
// (src/raw/decompress.rs:58-99) for every job, without decoding a byte.
//
// Every DecodeError depends on positions and lengths only (lzf_size_rules.h), so the kernel parses tokens and adds lengths:
//   one wavefront per job; the resident waves draw jobs from a counter — longest input first when there are more jobs than
//   resident waves (perm) — so a batch of uneven jobs does not wait for its longest one.  Per chunk of 64 x S compressed bytes the wave stages the bytes in LDS and lists the chunk's tokens with the
//   decompress kernels' lane-parallel parse (lz4_decompress_parse_phase.inc, described in lz4_decompress_batched.hip).  Then,
//   64 tokens per round: lane j decodes token j (lzf_size_rules.h: the common token without a loop), a wave inclusive scan of L + M gives every lane its position, every lane evaluates the three position checks of
//   its sequence, a ballot picks the first failing lane — stream order, as in the reference — and the carried position moves
//   on by the round's sum.  Compressed bytes come from HBM once; nothing but the result is written: no ring, no copy stage,
//   `prefix`, `out` and `out_cap` of the job are never looked at.  A token that reaches beyond its chunk (megabytes of 0xFF length
//   bytes, literals over many chunks) is decoded ahead of the parse, its 0xFF run eight bytes at a time.
// A call of few large blocks goes through the latency class first (lz4_decoded_size_seg.hip: a block summed up by many wavefronts);
// this kernel then runs last, over the whole call, and skips the jobs that class finished (SKIP, `done`).
// UnexpectedEnd is the parse's finding (cerr: right behind the chunk's listed tokens); inside a sequence it precedes the
// position checks (:63-71 before :72), and the failing sequence is never listed, so the order is the reference's.
#include "lzf_device.h"
#include "kernels.h"
#include "lzf_copy_helpers.h"
#include "lzf_parse_helpers.h"
#include "lzf_size_rules.h"

namespace lzf {

template <int S, int TOKCAP, bool SKIP>
__global__ __launch_bounds__(64) void lzf_decoded_size_kernel(const lzf_decompress_job* __restrict__ jobs, lzf_job_result* __restrict__ results,
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

    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(ticket, 1u);
        t = rfl(t);
        if (t >= n_jobs) break;
        const uint32_t jid = perm ? perm[t] : t;       // (perm: the jobs longest input first, so that the launch does not end on a long one)
        if (SKIP && done[jid].done) continue;          // finished by the latency class (lz4_decoded_size_seg.hip; uniform over the wave)
        const long long t_start = clock64();
        cgu8* __restrict__ in = as_global(jobs[jid].input);
        const uint64_t input_len = jobs[jid].input_len, plen = jobs[jid].prefix_len, existing = jobs[jid].out_existing_len;
        const uint64_t limit = jobs[jid].output_limit;
        int status = LZF_OK;
        uint64_t o = existing;                         // output.len()
        if (input_len >= kMaxPosB || existing >= kMaxPosB || plen >= kMaxPosB) {
            status = LZF_CONTRACT;
        } else {
            const uint32_t len = (uint32_t)input_len;
            const DecodeJob jv{in, nullptr, nullptr, len, 0u, 0u, 0ull, 0u};      // what the parse stage reads of a job: its input (there is no output here)
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
                // A token that reaches beyond the chunk (a length run of 0xFF bytes, literals over chunks) is taken here, by the
                // whole wave at once: the parse would walk its length bytes one at a time, three times over, and stage literals
                // nobody looks at.  cstart is a true token position, so a failure here is the sequence's UnexpectedEnd.
                {
                    const uint32_t w = g4(cstart);
                    if ((w & 0xFFF0u) == 0xFFF0u || (w & 15u) == 15u) {
                        lzf_size::Seq s;
                        uint32_t next;
                        if (!lzf_size::decode_token(cstart, len, g4, g1, gff, s, next)) { status = LZF_UNEXPECTED_END; break; }
                        if (next - cstart > kChunk) {
                            const int code = s.has ? lzf_size::check(o + s.L, s.M, s.off, plen, limit) : LZF_OK;
                            if (code != LZF_OK) { status = code; break; }
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
                    // 32-bit scan: the literals of a round lie in the input (sum of L <= len < 2^31) and 64 match lengths below
                    // 2^24 add up to less than 2^30; any longer match sends the round through the 64-bit scan
                    const bool wide = __ballot(act && s.M >= (1ull << 24)) != 0ull;
                    const uint64_t incl = wave_scan_add64(tot, wide);
                    const uint64_t mo = o + (incl - tot) + s.L;                          // output.len() behind this lane's literals
                    const int code = act && s.has ? lzf_size::check(mo, s.M, s.off, plen, limit) : LZF_OK;
                    const uint32_t e = first_lane(__ballot(code != LZF_OK));
                    if (e < 64u) { status = __builtin_amdgcn_readlane(code, e); break; }
                    o += readlane64(incl, 63);
                }
                if (status == LZF_OK && cerr != LZF_OK) status = cerr;
                cstart = cend;
            }
        }
        if (lane == 0) {
            results[jid].out_len = o;
            results[jid].status = status;
            results[jid].reserved = (uint32_t)((clock64() - t_start) >> 10);   // diagnostic: shader kilo-cycles spent on this job
        }
    }
}

template __global__ void lzf_decoded_size_kernel<48, 768, false>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*, const uint32_t*, const seg_job*);
template __global__ void lzf_decoded_size_kernel<48, 768, true>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*, const uint32_t*, const seg_job*);

}  // namespace lzf
