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
// The walk of one job (lz4_decode_head_walk.inc) and its copies (lz4_decode_head_copies.inc) are textual includes: the frame head
// kernel (frame_device_head.hip) runs the same body on the jobs of a frame's compressed blocks.
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

#include "lz4_decode_head_copies.inc"
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
        // the job's walk, chunk by chunk, 64 tokens a round (for (tidx = 0; tidx < Tc; tidx += kWave)): shared with lzf_frame_head_kernel
#include "lz4_decode_head_walk.inc"
        if (lane == 0) {
            results[jid].out_len = status == LZF_OK ? lzf_head::reported(o, cap, existing) : o;
            results[jid].status = status;
            results[jid].reserved = (uint32_t)((clock64() - t_start) >> 10);   // diagnostic: shader kilo-cycles spent on this job
        }
    }
}

template __global__ void lzf_decode_head_kernel<48, 768>(const lzf_decompress_job*, lzf_job_result*, uint32_t, uint32_t*);

}  // namespace lzf
