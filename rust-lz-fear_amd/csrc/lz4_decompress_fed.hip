// lz4_decompress_fed.hip — raw::decompress_raw (src/raw/decompress.rs:58-138) for batches beyond what the chip holds at once,
// with the PARSE taken out of the block's own wavefronts: the token positions of every block of the batch come from the hop
// parse of the segmented pipeline (lzf_seg_parse_kernel: one bit per compressed byte, 3.8 wave-instructions per sequence against
// the 13.0 of the in-kernel region parse of lz4_decompress_paired.hip), and the kernel here only FEEDS its copy stage from that
// map (lz4_decompress_feed_phase.inc: bit map -> token list) and runs the COPY stage (lz4_decompress_batch_phase.inc) with a
// set-up of its own (LZF_FED_DECODE: each listed token decoded once, the chain verified link by link before a batch writes
// anything).  The seam stage of the segmented pipeline is not part of this path: the wavefront walks the true chain and carries
// `expect`, the position of its next token, which says from where a chunk's marks are the true tokens; the few windows in which a
// chunk's chain has not fallen in step yet are walked token by token (walk mode, lz4_decompress_feed_phase.inc).
//
//   lzf_decompress_fed_kernel<RING, W, TOKCAP>        one wavefront per block: feed a window of 32 * W compressed bytes from where
//                                                     the chain stands, copy it; a short last batch waits for the next window
//
// Contract with the dispatch (lzf_dispatch.h, capi_drivers.hip): a job is taken only when the plan stage found it eligible (sizes inside the bit map's
// window); a job is FINISHED here (results written, seg_job::done set) only when it decodes cleanly over a verified chain.
// Everything else — every DecodeError, a capacity problem — is left untouched for the pair kernel launched behind this one, which
// decodes the job from its first byte and reports the reference's status.  What this kernel wrote into `out` before it gave up
// is a prefix of what that kernel writes again.
#include "lzf_device.h"
#include "kernels.h"
#include "lzf_copy_helpers.h"
#include "lzf_phase_timers.h"
#include "lzf_fed_window.h"
#include "lzf_dispatch.h"

namespace lzf {

// the XCD this wavefront runs on (0..7 on MI355X)
__device__ __forceinline__ uint32_t xcc_id() {
    uint32_t v; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v)); return v & 15u;
}

// ---------------------------------------------------------------------------------------------------------------------
// The launch is a fixed set of SLOTS — as many wavefronts as the device holds at once (capi_drivers.hip counts them) — that share the
// jobs out in PIECES instead of one workgroup per job.  With one workgroup per job a launch of 2.2 jobs per slot takes three
// rounds of the longest jobs' time, and inside a round every slot waits for the longest job (the timeline of round 6: 86 ms for
// 66 ms of work; a block costs 42 .. 86 M cycles and nothing cheap predicts which).  Here every job is cut into `pieces`
// stretches of equal compressed length, and the slots draw TICKETS from one counter: ticket t is piece t / n of the job of rank
// t % n in launch order — lap after lap over all jobs, so all of them advance together and end together, and a slot that gets
// cheap pieces simply draws more tickets.  A piece starts from the decoder state the piece before it parked (next round, chain
// carry, output position; the ring is re-filled from `out`) and waits for it if it has to: it was drawn n tickets earlier, and
// a launch has more jobs than slots, so as a rule it is long done.
// Hand-overs stay inside one XCD: the wavefronts read which XCD they run on (HW_REG_XCC_ID) and every XCD has its own ticket
// counter over its own share of the jobs (rank % number of XCDs).  What a piece wrote is then in the L2 its successor reads
// through — a wait for the stores and an L1 invalidate are the whole hand-over.  Across XCDs it would take a write-back of the
// writer's whole L2 (buffer_wbl2: measured ~150 us of the wave per hand-over, 98 -> 115 ms per call at 64 pieces per job).
// ---------------------------------------------------------------------------------------------------------------------
template <int RING, int W, int TOKCAP>
__global__ LZF_FED_BOUNDS void lzf_decompress_fed_kernel(fed_args a) {      // (kernels.h: six waves per SIMD, bound on the declaration too)
    constexpr uint32_t kSpanMax = RING / 3;            // output bytes one batch may produce
    constexpr uint32_t kNearHist = RING - kSpanMax;    // history before the batch that stays intact in the ring
    constexpr uint32_t kRound = 32u * (uint32_t)W;     // compressed bytes whose tokens one round lists
    constexpr uint32_t kCB = kRound + 128u;            // staged bytes: the round + room for the bodies of its last tokens
    static_assert(W >= 1 && W <= 64 && kRound == (uint32_t)kFedwRound, "a window is one bit-map word per lane (whose owner is worked out per word: lzf_fed_window.h)");
    static_assert(TOKCAP >= (int)(kRound / 3u + 1u), "a round's tokens (at least three bytes each) fit the list");
    static_assert(kCB % 16 == 0, "the round is staged in 16-byte pieces");
    __shared__ __attribute__((aligned(16))) uint8_t ring[RING];
    __shared__ __attribute__((aligned(16))) uint8_t cbuf[kCB];
    __shared__ __attribute__((aligned(16))) uint16_t toks[TOKCAP];
    static_assert(RING != 4096 || W != 32 || TOKCAP != 352 || lzf_dispatch::lds_alloc(sizeof ring + sizeof cbuf + sizeof toks) == lzf_dispatch::kFedLdsAlloc, "lzf_dispatch.h: the residency the census falls back on");

    const uint32_t lane = threadIdx.x;
    if (a.census) {
        // How many workgroups of THIS kernel (its LDS, registers) does the device hold at once?  Every workgroup counts itself in,
        // stays for 300 us and reads the count when it leaves: the first residents read the residency, later ones more; the minimum
        // is the answer.  (The schedule needs the true number: a slot that starts late finishes late, and the slot that waits for
        // its hand-over with it.)
        if (lane == 0u) {
            __hip_atomic_fetch_or(&a.census[2], 1u << (xcc_id() & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ... and on which XCDs they run
            __hip_atomic_fetch_add(&a.census[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long t0 = wall_clock64();
            while (wall_clock64() - t0 < 30000ull) __builtin_amdgcn_s_sleep(16);
            const uint32_t seen = __hip_atomic_load(&a.census[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&a.census[1], seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        return;
    }
    const uint32_t n = a.n_jobs, pieces = a.pieces;
    // this wavefront's XCD -> its group of jobs (ranks g, g + ng, g + 2 ng, ...) and that group's ticket counter
    // (whole jobs need no hand-over: one group, one counter)
    const uint32_t xcc = xcc_id() & 31u;
    if (pieces > 1u && !((a.xcc_mask >> xcc) & 1u)) return;           // (an XCD the census did not see: no jobs were given to it)
    const uint32_t ng = pieces > 1u ? (uint32_t)__popc(a.xcc_mask) : 1u, g = pieces > 1u ? (uint32_t)__popc(a.xcc_mask & ((1u << xcc) - 1u)) : 0u;
    const uint32_t n_g = lzf_fedw_group_jobs(n, g, ng);
#ifdef LZF_ANALYSIS
    const uint32_t n_tickets = n_g * (a.stop_piece && a.stop_piece < pieces ? a.stop_piece : pieces);      // (lzf_debug_fed: the tickets of pieces >= stop_piece are not drawn)
#else
    const uint32_t n_tickets = n_g * pieces;
#endif
    for (;;) {
    uint32_t tk = 0;
    if (lane == 0u) tk = __hip_atomic_fetch_add(a.ticket + g * kFedTicketStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tk = __builtin_amdgcn_readfirstlane(tk);
    if (tk >= n_tickets) break;
    const uint32_t piece = lzf_fedw_ticket_piece(tk, n_g), k = lzf_fedw_ticket_rank(tk, piece, n_g, g, ng);
    const uint32_t jid = a.perm ? a.perm[k] : k;
    const seg_job sj = a.st[jid];
    if (!sj.eligible || sj.failed || sj.done) continue;
    LZF_GLOBAL fed_state* const fs = (LZF_GLOBAL fed_state*)a.state + jid;
    const lzf_decompress_job job = a.jobs[jid];
    const long long t_start = clock64();
#ifdef LZF_DBG_TIMELINE
    const unsigned long long t_wall0 = wall_clock64();
#endif

    int status = LZF_OK;
    bool bailed = false, parked = false;
    uint32_t o = 0;
    PhaseTimers ph;
#ifdef LZF_DBG_FED_COUNT   // analysis: [0] batches, [1] windows listed from the map, [2] windows walked, [3] trips of the match-round loop, [4] overlapping cooperative matches whose offset is a power of two (no division), [5] store fences in front of a batch's far / slow sources (need > safe), of this wave's share of the job (LZF_FED_PIECES=1: the job) -> results[].reserved
    uint32_t dbg_fed[6] = {0u, 0u, 0u, 0u, 0u, 0u};
#endif
    if (LZF_DECODE_JOB_OUT_OF_CONTRACT(job)) continue;      // (LZF_CONTRACT: the pair kernel says so)
    {
        const DecodeJob jv = LZF_DECODE_JOB_VIEW(job);
        const OutRing<RING> rg{ring, jv.out, jv.rb, lane, lds_addr(ring)};
        const uint32_t cbuf_a = lds_addr(cbuf);
        const LZF_GLOBAL uint32_t* const fed_bits = (const LZF_GLOBAL uint32_t*)a.bits + (size_t)jid * a.maxch * kSegChunkWords;
        uint32_t expect = 0;                 // where the next token of the chain starts (len: the chain has ended)
        uint32_t cstart = 0;
        o = (uint32_t)job.out_existing_len;
        // this piece: the tokens that start in rounds [piece, piece + 1) * per of the job's input (lzf_fed_window.h)
        const uint32_t piece_end = lzf_fedw_piece_end(jv.len, pieces, piece);
        if (piece > 0u) {
            // the piece before this one was drawn n tickets ago: as a rule it is done; else wait for it (bounded), then take its state over
            uint32_t f = 0;
            for (uint32_t spin = 0; spin < (1u << 22); ++spin) {
                f = __hip_atomic_load(&fs->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (f >= piece) break;
                __builtin_amdgcn_s_sleep(32);
            }
            f = __builtin_amdgcn_readfirstlane(f);
            if (f != piece) continue;        // the job ended in an earlier piece (kFedEnded), or that piece never came: the pair kernel looks at what is left
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");       // (this compute unit's L1 may hold lines of `out` from an earlier piece of the job)
            expect = fs->expect; o = fs->o;  // (a short batch the piece before left at its end is simply this piece's first)
        }
        uint32_t safe = o;   // out[0, safe) is visible to this wave's global loads
        uint32_t pend = o;   // out[pend, o) is the last batch, still only in the ring: the next batch flushes it behind its far loads, or the drain below
        if (o > 0) rg.fill(o > (uint32_t)RING ? o - RING : 0u, o);   // Vec content on entry (or what the other slot wrote) = history
        ph.start();          // (section 1 here with the tokens' decode and the chain check: lzf_phase_timers.h)
#if defined(LZF_FED_FIXED_ROUNDS)
        constexpr int kFixed = 1;
        const uint32_t fed_carry = 0u;
#elif defined(LZF_ANALYSIS)
        constexpr int kFixed = 0;
        const uint32_t fed_carry = a.carry < kWave ? a.carry : kWave - 1u;      // (LZF_FED_CARRY)
#else
        constexpr int kFixed = 0;
        constexpr uint32_t fed_carry = kFedwCarry;
#endif
        bool fed_walk = false;               // this window is listed by walking the chain, not from the bit map
        // INVARIANT of the loop: a pass either ends the job for this kernel (status, bailed), parks it, asks for the same window again
        // in walk mode (once: a failure in walk mode ends the job), or runs at least one batch — a window's first batch is never
        // carried, and a batch that passes its checks moves `expect` on by a token or more.  The last `if` holds the loop to that.
        while (expect < jv.len && status == LZF_OK) {
            if (expect >= piece_end) { parked = true; break; }      // the next piece's
            const uint32_t expect_in = expect;
            cstart = lzf_fedw_start(expect, kFixed);
            __syncthreads();                 // (one wave: orders the re-use of cbuf / toks between windows)
#ifdef LZF_DBG_FED_COUNT
            ++dbg_fed[fed_walk ? 2 : 1];
#endif
#include "lz4_decompress_feed_phase.inc"
            if (Tc) {
#define LZF_FED_DECODE
#ifdef LZF_FED_FAR_LATE
#define LZF_FAR_LATE
#endif
#include "lz4_decompress_batch_phase.inc"
#undef LZF_FAR_LATE
#undef LZF_FED_DECODE
            }
            if (bail) {
                if (fed_walk) { bailed = true; break; }              // the chain itself fails: the pair kernel reports it
                fed_walk = true; continue;                           // the map is wrong about this window: walk it from `expect`
            }
            fed_walk = false;
            if (expect == expect_in && status == LZF_OK) { bailed = true; break; }      // (no progress: never, by the invariant — and never a spin)
        }
        // The drain: whichever way the loop ended — parked, the chain's end, a status, a bail — the last batch goes to `out` here, in front of the
        // hand-over's wait and of results[].  An error is raised before its batch writes anything, so `out` holds what it held when every batch
        // flushed itself: all of the job up to the failing batch, a prefix of what the pair kernel writes again.  (A solo sequence that fails
        // leaves nothing pending: pend >= o.)
        if (pend < o && !(LZF_DBG_SKIP & 16)) rg.flush(pend, o);
        if (parked && status == LZF_OK && !bailed) {
            // hand the job on: what this wave wrote must be visible to another compute unit before the flag is
            if (lane == 0u) { fs->expect = expect; fs->o = o; }
            // (no release fence: the next piece runs on this XCD and reads through the same L2 — the stores only have to have arrived there)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0u) __hip_atomic_store(&fs->flag, piece + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
    }
    if (pieces > 1u && lane == 0u) __hip_atomic_store(&fs->flag, kFedEnded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // finished or given up: later tickets of the job pass
    if (bailed || status != LZF_OK) continue;        // not ours: the pair kernel decodes the job again and reports the status
    if (lane == 0) {
        a.results[jid].out_len = o;
        a.results[jid].status = LZF_OK;
#ifdef LZF_DBG_FED_COUNT
        a.results[jid].reserved = dbg_fed[LZF_DBG_FED_COUNT];
#elif defined(LZF_DBG_PHASE_SEL)
        ph.report(a.results[jid]);
#elif defined(LZF_DBG_TIMELINE)   // analysis: when the job ran, on the 100 MHz wall clock every wave reads alike (units of 2.56 us): start << 16 | end
        a.results[jid].reserved = (uint32_t)(((t_wall0 >> 8) & 0xFFFFull) << 16) | (uint32_t)((wall_clock64() >> 8) & 0xFFFFull);
#else
        a.results[jid].reserved = (uint32_t)((clock64() - t_start) >> 10);   // diagnostic: shader kilo-cycles spent on this job
#endif
        a.st[jid].done = 1u;
    }
    }
}

// Before the launch: every job's hand-over flag and the ticket counter cleared.
__global__ __launch_bounds__(256) void lzf_fed_reset_kernel(fed_args a) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < 32u) a.ticket[k * kFedTicketStride] = 0u;
    if (k < a.n_jobs) a.state[k].flag = 0u;
}

#define LZF_INSTF(NAME, RG, W_, T) template __global__ void lzf_decompress_fed_kernel<RG, W_, T>(fed_args);
LZF_FED_VARIANTS(LZF_INSTF)
#undef LZF_INSTF

}  // namespace lzf
