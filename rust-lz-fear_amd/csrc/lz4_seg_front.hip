// lz4_seg_front.hip — the front of the segmented pipeline (lzf_seg_common.h, kernels.h): plan, parse, seam.  Three paths start here: the
// segmented decode (all three, then lz4_seg_tiles.hip and lz4_seg_resolve.hip), the fed call (plan and parse with seg_ctx::fed, then
// lz4_decompress_fed.hip) and the size call's latency class (all three with seg_ctx::size_only, then lz4_decoded_size_seg.hip).
#include "lzf_seg_common.h"
#include "lzf_dispatch.h"
#include <type_traits>

namespace lzf {
namespace {

constexpr uint32_t S = kSegRegion;
constexpr uint32_t kCB = kSegChunk;                // staged bytes of a chunk (with the rows: 20 480 bytes of LDS, eight chunks per CU; tokens that reach over the end take the general routine)
// Walks of the fixed point a lane keeps beside its live one (11 VGPRs each: entry, exit, merge position, the eight words of row B).
// LDS holds the parse kernel to two waves per SIMD, so the registers cost no residency.  -DLZF_PARSE_MEMO=2: the depth A/B of profiles/parse_memo.txt.
#ifndef LZF_PARSE_MEMO
#define LZF_PARSE_MEMO 1
#endif
constexpr uint32_t kParseMemo = LZF_PARSE_MEMO;
static_assert(kParseMemo == 1u || kParseMemo == 2u, "one or two saved walks");
constexpr uint32_t kNoEntry = ~0u;                 // an empty slot: no entry has this value (chunk-relative positions stay below 2^31)

__device__ __forceinline__ constexpr uint32_t seg_nch(uint32_t len) {
    return len <= kSegChunk ? 1u : 1u + (len - kSegChunk + kSegStride - 1u) / kSegStride;
}
// (the host sizes the bit maps with its own copy)
static_assert(seg_nch(1u) == lzf_dispatch::seg_nch(1u) && seg_nch(kSegChunk) == lzf_dispatch::seg_nch(kSegChunk) && seg_nch(kSegChunk + 1u) == lzf_dispatch::seg_nch(kSegChunk + 1u) &&
              seg_nch(kSegChunk + kSegStride + 1u) == lzf_dispatch::seg_nch(kSegChunk + kSegStride + 1u) && seg_nch(lzf_dispatch::kSegMaxIn) == lzf_dispatch::seg_nch(lzf_dispatch::kSegMaxIn),
              "lzf_dispatch.h restates seg_nch");

}  // namespace

// =====================================================================================================================
// plan
// =====================================================================================================================
__global__ __launch_bounds__(256) void lzf_seg_plan_kernel(seg_ctx c) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j == 0u && c.rec_top) *c.rec_top = 0ull;
    if (j >= c.n_jobs) return;
    const lzf_decompress_job job = c.jobs[j];
    seg_job s;
    s.failed = 0; s.done = 0; s.ntok = 0; s.outb = 0; s.pad = 0; s.rec_off = 0; s.pad2 = 0;
    const bool in_window = job.input_len >= c.min_in && job.input_len <= c.max_in;
    if (c.size_only)     // nothing is decoded: no `out`, prefix and existing output are lengths (beyond 2 GiB: the one-wave kernel's LZF_CONTRACT); an empty input has no bytes to point at
        s.eligible = (in_window && (job.input != nullptr || job.input_len == 0) && job.prefix_len < kMaxPosB && job.out_existing_len < kMaxPosB) ? 1u : 0u;
    else {
        // history (a prefix, existing output) in 31-bit positions like everything else; existing output of 65 535 bytes or more hides the
        // prefix for good (an offset is at most 65 535): such a job is decoded as one without a prefix, whatever its pointer
        const bool history = job.prefix_len < kMaxPosB && job.out_existing_len < kMaxPosB &&
                             (job.prefix_len == 0 || job.out_existing_len >= kSegPrefixReach || job.prefix != nullptr);
        s.eligible = ((c.fed || history) && in_window && job.input != nullptr && job.out != nullptr) ? 1u : 0u;
    }
    const uint32_t len = s.eligible ? (uint32_t)job.input_len : 0u;
    s.nch = s.eligible && !(c.size_only && len == 0u) ? seg_nch(len) : 0u;
    s.ntile = (len + kSegTile - 1u) / kSegTile;
    if (s.nch > c.maxch || s.ntile > c.maxtile) { s.eligible = 0; s.nch = 0; s.ntile = 0; }
    c.st[j] = s;
    // the launch order of a fed call: the bytes' share of the job's cost; the parse adds the sequences, chunk by chunk.  A job the
    // map does not cover gets a guess by its length in their place: input_len >> 4, the guess lzf_decompress_cost_kernel makes for an
    // input too short to sample — here WITH the bytes' share on top, as every other job of the call has it (that kernel's short path
    // leaves the share out: tests/launch_order_cases.py models both as they are).
    if (c.est) {
        const uint32_t l31 = job.input_len > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)job.input_len;
        c.est[j] = (s.eligible ? 0u : l31 >> 4) + (c.len_shift < 32u ? l31 >> c.len_shift : 0u);
    }
}

// =====================================================================================================================
// parse: the chain of tokens that starts at a chunk's first byte, as a bit map
// =====================================================================================================================
// A chunk is 64 regions of 256 bytes, one per lane, staged in LDS.
//   pass 0   every lane walks from its region start and marks the tokens it visits in row A, keeps its exit;
//   pass k   entry[i] = max(exit[0..i-1]) (lane 0: the chunk's first byte); a lane whose entry changed walks again from it,
//            marking row B, until it steps on a token marked in row A — from there on it IS the pass-0 chain — or leaves
//            the region; repeated until no entry changes (about five passes on compressed text and binaries).
//            A region's result for an entry depends on the chunk's bytes and on row A alone, and neither changes during the passes:
//            the result a new entry displaces (walked entry, exit, merge position, row B) is kept in registers, kParseMemo deep, and a
//            lane whose entry comes back — the lane below corrected itself and its exit returned — takes it back without a walk.
//            A pass lasts as long as its slowest walking lane, so the passes get shorter, not fewer (tools/parse_memo_model.c).
//   result   row = (A from the merge position on) | B; exit of the chunk = max of the exits.
// A plain hop is ONE unaligned 4-byte LDS read from position - 1: [previous token's match-length extension byte, token,
// first literal-length extension byte, ...].  Tokens a plain hop cannot express (0xFF length bytes, the last 24 bytes of
// the input) go through the general routine.
// -DLZF_DBG_PARSE_TIME (analysis): cycles of a parse wave by section, summed over the launch — 0 staging (loads issued and waited for,
// LDS stores), 1 pass 0, 2 the fixed-point passes, 3 the rows written out; [4] chunks, [5] workgroups that had one; [6] / [7] the hops the
// wave made in the plain-hop loop (one per half of a trip: a count kept by the scalar unit inside the loop) in pass 0 / in the fixed-point passes;
// [8] / [9] the lookups of the saved walks (a lane whose entry changed, in any pass) / the lookups that hit.
// lzf_debug_parse_timers() reads (and clears) the sums: tools/parse_staging.py.
#ifdef LZF_DBG_PARSE_TIME
__device__ unsigned long long lzf_dbg_parse_cycles[10];
#define PT_START() long long pt_t = clock64(); unsigned long long pt[4] = {0, 0, 0, 0}; uint32_t pt_n = 0, pt_hops[2] = {0, 0}, pt_memo[2] = {0, 0}
#define PT_MEMO(look, hit) do { pt_memo[0] += (uint32_t)__popcll(__ballot(look)); pt_memo[1] += (uint32_t)__popcll(__ballot(hit)); } while (0)
#define PT_MARK(i) do { const long long tn_ = clock64(); pt[i] += (unsigned long long)(tn_ - pt_t); pt_t = tn_; } while (0)
#define PT_CHUNK() (++pt_n)
#define PT_HOP_ASM "s_add_u32 %[nh], %[nh], 1\n\t"
#define PT_HOPS(mode, n) (pt_hops[mode] += (n))
#define PT_REPORT() do { if (lane == 0u && pt_n) { for (int i_ = 0; i_ < 4; ++i_) atomicAdd(&lzf_dbg_parse_cycles[i_], pt[i_]); \
                                                     atomicAdd(&lzf_dbg_parse_cycles[4], (unsigned long long)pt_n); atomicAdd(&lzf_dbg_parse_cycles[5], 1ull); \
                                                     atomicAdd(&lzf_dbg_parse_cycles[6], (unsigned long long)pt_hops[0]); atomicAdd(&lzf_dbg_parse_cycles[7], (unsigned long long)pt_hops[1]); \
                                                     atomicAdd(&lzf_dbg_parse_cycles[8], (unsigned long long)pt_memo[0]); atomicAdd(&lzf_dbg_parse_cycles[9], (unsigned long long)pt_memo[1]); } } while (0)
#else
#define PT_MEMO(look, hit) do { } while (0)
#define PT_START() do { } while (0)
#define PT_MARK(i) do { } while (0)
#define PT_CHUNK() do { } while (0)
#define PT_HOP_ASM ""
#define PT_HOPS(mode, n) do { } while (0)
#define PT_REPORT() do { } while (0)
#endif
__global__ __launch_bounds__(64) void lzf_seg_parse_kernel(seg_ctx c) {
    // one array: rows A, rows B, the chunk's bytes.  A hop reads 4 bytes from position - 1: for the chunk's first byte that is the last
    // byte of row B (any value: a walk's first hop does not look at it), and no hop lands on the last two bytes (see `fe`).
    __shared__ __attribute__((aligned(16))) uint8_t lds_parse[2u * 64u * 8u * 4u + kCB];
    static_assert(sizeof(lds_parse) == 20480, "eight chunks per CU: an eighth of 160 KiB each");
    uint32_t* const rowsA = reinterpret_cast<uint32_t*>(lds_parse);
    uint32_t* const rowsB = rowsA + 64u * 8u;
    const uint32_t j = seg_job_of(c, blockIdx.y);
    const seg_job sj = c.st[j];
    if (!sj.eligible) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    cgu8* __restrict__ in = as_global(job.input);
    const uint32_t len = (uint32_t)job.input_len;
    uint8_t* const cbuf = lds_parse + 2u * 64u * 8u * 4u;
    const uint32_t cbuf_a = lds_addr(cbuf);
    // word w of a lane's row lives at [w * 64 + lane]: the 64 lanes of an access hit 64 different banks
#define ROWA(w) rowsA[(w) * 64u + lane]
#define ROWB(w) rowsB[(w) * 64u + lane]

    PT_START();
    for (uint32_t h = blockIdx.x; h < sj.nch; h += gridDim.x) {
        const uint32_t cstart = h * kSegStride;
        __syncthreads();                         // (one wave: orders the LDS re-use between iterations)
        // ---- stage in[cstart, cstart + kCB) (zeros beyond the input): ONE round trip — a lane's kLd 16-byte loads are all issued before
        //      the first is waited for (a fully unrolled register array; issued four at a time, a chunk cost four dependent HBM round trips
        //      before its first hop).  No branch around a load: a lane whose 16 bytes end behind `avail` loads the last whole 16 bytes in
        //      front of it instead — nothing at or beyond in + len is read — and stores zeros.
        {
            const uint32_t avail = len - cstart < kCB ? len - cstart : kCB;
            cgu8* g = in + cstart;
            constexpr uint32_t kLd = kCB / 1024u;
            u32x4 v[kLd];
            if (avail >= 16u) {
#pragma unroll
                for (uint32_t k = 0; k < kLd; ++k) { const uint32_t i = k * 1024u + lane * 16u; v[k] = ld16(g + (i < avail - 16u ? i : avail - 16u)); }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kLd; ++k) v[k] = u32x4{0, 0, 0, 0};
            }
            if (avail == kCB) {
#pragma unroll
                for (uint32_t k = 0; k < kLd; ++k) *reinterpret_cast<u32x4*>(&cbuf[k * 1024u + lane * 16u]) = v[k];
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kLd; ++k) { const uint32_t i = k * 1024u + lane * 16u; *reinterpret_cast<u32x4*>(&cbuf[i]) = i + 16u <= avail ? v[k] : u32x4{0, 0, 0, 0}; }
            }
            { const uint32_t t0 = avail & ~15u; if (t0 < kCB && lane < (avail & 15u)) cbuf[t0 + lane] = g[t0 + lane]; }   // the ragged end of the input
        }
        PT_MARK(0);
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) { ROWA(i) = 0u; ROWB(i) = 0u; }
        const uint32_t room = len - cstart;                                      // bytes from the chunk start to the end of the input
        // a plain hop lands below fe (chunk-relative): 24 bytes short of the input's end, and 2 short of the staged bytes — a lane reads the
        // 4 bytes from its position - 1 wherever it has landed (the extension byte of the token before is checked there), and a read
        // that crosses the end of the workgroup's LDS returns zeros for all four
        const uint32_t fe = room > 24u ? (room - 24u < kCB - 2u ? room - 24u : kCB - 2u) : 0u;
        const uint32_t rb0 = lane * S, end_r = rb0 + S;

        auto rdb = [&](uint32_t q) -> uint32_t { const uint32_t r_ = q - cstart; if (r_ < kCB) return (uint32_t)cbuf[r_]; return (uint32_t)in[q]; };
        auto rd8 = [&](uint32_t q) -> uint64_t { const uint32_t r_ = q - cstart; if (r_ + 8u <= kCB) return lds_ld64u(cbuf_a + r_); return ld8(in + q); };
        auto token_next = [&](uint32_t p, uint32_t& next) -> bool { return token_next_gen(len, p, next, rd8, rdb); };
        // MODE 0: mark in row A.  MODE 1: stop on a token marked in row A (merged), mark in row B.
        // Walks from r (chunk-relative) to the first token at or beyond end_r; returns where it stopped.
        auto walk = [&](uint32_t r, bool go, bool& merged, auto MODE) -> uint32_t {
            constexpr int mode = decltype(MODE)::value;
            const uint32_t stop = go ? (end_r < fe ? end_r : fe) : 0u;
            for (;;) {
#ifndef LZF_SEG_NOASM
                // ---- plain hops, hand-scheduled (the walks are chains of dependent instructions: every one counts; hipcc's version of
                //      this loop spends ~20 scalar instructions per hop on lane masks).  A lane is in the loop while it is in EXEC and leaves it
                //      for good when its hop is not a plain one: past the stop position, parked for the general routine, on a token marked in
                //      row A (mode 1), or because the previous token's match length turned out to go on (0xFF extension byte: the lane steps
                //      back to that token, which the general routine then takes).
                //      TWO hops per trip, the halves with the roles of the two position registers swapped: the first half hops from r, with
                //      the token before it in q, and writes the next position over q; the second half hops from q with r before it and
                //      writes r.  No register is copied, and every other back-edge is an s_cbranch_execz that is not taken as a rule.
                //      A lane's position when it leaves is the register its last hop STARTED from: a hop that is not plain does not move, and
                //      the step back selects the other register into it first.  (The other register is NOT the same position then: the
                //      next-position add has already written it when the stop compare takes the lane out.)  Which register that is stands
                //      in bit 16 of mxp: each half writes mxp, with its own bit 16, before the first compare that lets a lane go, so the bit
                //      always names the register of the half the lane left in.  Behind the loop r is taken from q where the bit is set;
                //      nothing else of the loop's state is read after it.
                //      Nothing inside a trip goes through the scalar unit but the wait and the two branches: the step back leaves with the
                //      stop compare, which sees ~0 in its place.  19 vector + 2 LDS instructions per hop (mode 1: 23 + 3).
                //      mxp (low half) = the byte in front of the token that means "not plain": 0xFF when the previous token's match
                //      nibble was 15, else 0x100 (no byte has that value).
                {
                    // (the registers the loop writes are early-clobber: mxp starts as 0x100, and an input of the same value — v100 — would
                    //  otherwise share its register, which turns the select that writes mxp into "0xFF or what it was")
                    uint32_t mxp = 0x100u, q = r, mg = merged ? 1u : 0u;
                    const uint32_t stopv = stop;
                    const unsigned long long m0 = __ballot(go && !merged && r < stop);
                    uint32_t a_, w_, t_, x_, y_, bit_, mk_;
                    unsigned long long sv, sc, sb;
                    uint32_t nh = 0;                       // (LZF_DBG_PARSE_TIME: hops of the wave)
                    // row word of position r: rows[(r >> 5) - 8 * lane][lane] = rowsA + ((r >> 5) << 8) + 4 * lane - (lane << 11)  (mod 2^32)
                    const uint32_t rowa2 = lds_addr(rowsA) + lane * 4u - (lane << 11), rowd = lds_addr(rowsB) - lds_addr(rowsA);
                    const uint32_t vzero = 0u, vff = 0xFFu, v100 = 0x100u, vffq = 0x100FFu, v100q = 0x10100u, vf00 = 0xF00u;     // (registers: a literal beside a mask is one constant too many)
                    // one hop from P with the token before it in Q; the next position goes to Q.  C100 / VFF: the two values of mxp this half writes.
                    // The match nibble's compare goes to an SGPR pair of its own and the literal nibble's to vcc, each standing between
                    // the other and its readers: no select reads a mask in the two issue slots behind the compare that wrote it.  The
                    // mark's address is worked out behind the last compare that writes EXEC, on the way to the branch.
#define SEG_HOP_STEP_BACK(P, Q, L) \
                            "s_waitcnt lgkmcnt(0)\n\t" \
                            "v_cmp_ne_u32_sdwa vcc, %[w], %[mxp] src0_sel:BYTE_0 src1_sel:WORD_0\n\t"   /* no step back */ \
                            "v_and_b32 %[a], 0xf00, %[w]\n\t" \
                            "v_bfe_u32 " L ", %[w], 12, 4\n\t" \
                            "v_cndmask_b32 %[t], -1, " P ", vcc\n\t"                                   /* what the stop compare sees */ \
                            "v_cndmask_b32 " P ", " Q ", " P ", vcc\n\t"
#define SEG_HOP_NEXT(P, Q, C100, VFF, L) \
                            "v_cmp_eq_u32_e64 %[sb], %[a], %[vf00]\n\t"                                /* match nibble 15 */ \
                            "v_cmp_eq_u32 vcc, 15, " L "\n\t"                                          /* literal nibble 15 */ \
                            "v_lshlrev_b32 %[bit], " P ", 1\n\t" \
                            "v_cndmask_b32_e64 %[mxp], " C100 ", " VFF ", %[sb]\n\t" \
                            "v_addc_co_u32 " Q ", %[sc], 3, " P ", %[sb]\n\t"                          /* token, offset, the match extension byte */ \
                            "v_cmpx_lt_u32_e64 %[sc], %[t], %[stop]\n\t"                               /* (vcc stays) */
#define SEG_HOP_LITERALS(Q, L) \
                            "v_cndmask_b32_sdwa %[a], %[vz], %[w], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2\n\t" \
                            "v_addc_co_u32 " L ", vcc, " L ", %[a], vcc\n\t" \
                            "v_add_u32 " Q ", " Q ", " L "\n\t"
#define SEG_HOP_PARK(Q) \
                            "v_cmpx_ne_u32 vcc, 0xff, %[a]\n\t"                                        /* 0xFF extension of the literal length: parked */ \
                            "v_cmpx_gt_u32 vcc, %[fe], " Q "\n\t"
#define SEG_HOP0(P, Q, C100, VFF) \
                            PT_HOP_ASM \
                            "v_add_u32 %[a], %[cbm1], " P "\n\t" \
                            "ds_read_b32 %[w], %[a]\n\t" \
                            SEG_HOP_STEP_BACK(P, Q, "%[x]") \
                            SEG_HOP_NEXT(P, Q, C100, VFF, "%[x]") \
                            SEG_HOP_LITERALS(Q, "%[x]") \
                            SEG_HOP_PARK(Q) \
                            "v_lshrrev_b32 %[x], 5, " P "\n\t" \
                            "v_lshl_add_u32 %[x], %[x], 8, %[rowa2]\n\t" \
                            "ds_or_b32 %[x], %[bit]\n\t"
#define SEG_HOP1(P, Q, C100, VFF) \
                            PT_HOP_ASM \
                            "v_add_u32 %[a], %[cbm1], " P "\n\t" \
                            "v_lshrrev_b32 %[x], 5, " P "\n\t" \
                            "ds_read_b32 %[w], %[a]\n\t" \
                            "v_lshl_add_u32 %[x], %[x], 8, %[rowa2]\n\t" \
                            "ds_read_b32 %[mk], %[x]\n\t" \
                            SEG_HOP_STEP_BACK(P, Q, "%[y]") \
                            "v_bfe_u32 %[mk], %[mk], " P ", 1\n\t" \
                            SEG_HOP_NEXT(P, Q, C100, VFF, "%[y]") \
                            "v_or_b32 %[mg], %[mg], %[mk]\n\t"                                         /* below the stop position on a token of the pass-0 chain: merged */ \
                            SEG_HOP_LITERALS(Q, "%[y]") \
                            "v_cmpx_eq_u32 vcc, 0, %[mk]\n\t" \
                            SEG_HOP_PARK(Q) \
                            "v_add_u32 %[x], %[x], %[rowd]\n\t"                                        /* the same word of row B */ \
                            "ds_or_b32 %[x], %[bit]\n\t"
                    if (mode == 0) {
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            "s_and_b64 exec, exec, %[m0]\n\t"
                            "s_cbranch_execz Ld%=\n"
                            "Lw%=:\n\t"
                            SEG_HOP0("%[r]", "%[q]", "%[v100]", "%[vff]")
                            "s_cbranch_execz Ld%=\n\t"
                            SEG_HOP0("%[q]", "%[r]", "%[v100q]", "%[vffq]")
                            "s_cbranch_execnz Lw%=\n"
                            "Ld%=:\n\t"
                            "s_mov_b64 exec, %[sv]"
                            : [r] "+&v"(r), [q] "+&v"(q), [mxp] "+&v"(mxp),
                              [a] "=&v"(a_), [w] "=&v"(w_), [t] "=&v"(t_), [x] "=&v"(x_), [bit] "=&v"(bit_), [sv] "=&s"(sv), [sc] "=&s"(sc), [sb] "=&s"(sb), [nh] "+s"(nh)
                            : [cbm1] "s"(cbuf_a - 1u), [fe] "s"(fe), [stop] "v"(stopv), [rowa2] "v"(rowa2), [vz] "v"(vzero), [vff] "v"(vff), [v100] "v"(v100), [vffq] "v"(vffq), [v100q] "v"(v100q), [vf00] "v"(vf00), [m0] "s"(m0)
                            : "vcc", "scc", "memory");
                    } else {
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            "s_and_b64 exec, exec, %[m0]\n\t"
                            "s_cbranch_execz Ld%=\n"
                            "Lw%=:\n\t"
                            SEG_HOP1("%[r]", "%[q]", "%[v100]", "%[vff]")
                            "s_cbranch_execz Ld%=\n\t"
                            SEG_HOP1("%[q]", "%[r]", "%[v100q]", "%[vffq]")
                            "s_cbranch_execnz Lw%=\n"
                            "Ld%=:\n\t"
                            "s_mov_b64 exec, %[sv]"
                            : [r] "+&v"(r), [q] "+&v"(q), [mxp] "+&v"(mxp), [mg] "+&v"(mg),
                              [a] "=&v"(a_), [w] "=&v"(w_), [t] "=&v"(t_), [x] "=&v"(x_), [y] "=&v"(y_), [bit] "=&v"(bit_), [mk] "=&v"(mk_), [sv] "=&s"(sv), [sc] "=&s"(sc), [sb] "=&s"(sb), [nh] "+s"(nh)
                            : [cbm1] "s"(cbuf_a - 1u), [fe] "s"(fe), [stop] "v"(stopv), [rowa2] "v"(rowa2), [rowd] "v"(rowd), [vz] "v"(vzero), [vff] "v"(vff), [v100] "v"(v100), [vffq] "v"(vffq), [v100q] "v"(v100q), [vf00] "v"(vf00), [m0] "s"(m0)
                            : "vcc", "scc", "memory");
                    }
#undef SEG_HOP_STEP_BACK
#undef SEG_HOP_NEXT
#undef SEG_HOP_LITERALS
#undef SEG_HOP_PARK
#undef SEG_HOP0
#undef SEG_HOP1
                    if (mxp & 0x10000u) r = q;             // the lane's last hop started in the second half
                    merged = mg != 0u;
                    PT_HOPS(mode, nh);
                }
#else
                // the same loop in C++: two hops per trip, the second with the two position registers in each other's role
                uint32_t mxp = 0, q = r;
                bool act = go && !merged && r < stop, in_q = false;        // in_q: the lane's last hop started from q (the asm: bit 16 of mxp)
                // one hop from p, the token before it in o; the next position goes to o
                auto hop = [&](uint32_t& p, uint32_t& o, bool second) {
                    uint32_t lo;
                    asm volatile("ds_read_b32 %0, %1" : "=v"(lo) : "v"(cbuf_a + (act ? p : 0u) - 1u) : "memory");
                    uint32_t mk = 0;
                    const uint32_t bi = (act ? p : rb0) - rb0;
                    if (mode == 1) mk = *reinterpret_cast<const volatile uint32_t*>(&ROWA((bi >> 5) & 7u)) >> (bi & 31u);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    const uint32_t e0 = lo & 255u;
                    if (act && mxp != 0u && e0 == 255u) { p = o; act = false; }       // the previous token's match length goes on: not plain (p == o now)
                    if (act) in_q = second;
                    if (act && p >= stop) act = false;
                    if (mode == 1) { if (act && (mk & 1u)) { merged = true; act = false; } }
                    if (act) {
                        const uint32_t L0 = (lo >> 12) & 15u, M0 = (lo >> 8) & 15u, b1 = (lo >> 16) & 255u;
                        const uint32_t isx = L0 == 15u ? 1u : 0u;
                        const uint32_t Lt = L0 + (isx ? b1 : 0u);
                        const uint32_t mx = M0 == 15u ? 1u : 0u;
                        const uint32_t pn = p + 3u + isx + Lt + mx;
                        const bool plain = !(isx && b1 == 255u) && pn < fe;
                        if (plain) {
                            if (mode == 0) ROWA((bi >> 5) & 7u) |= 1u << (bi & 31u); else ROWB((bi >> 5) & 7u) |= 1u << (bi & 31u);
                            o = pn; mxp = mx;
                        } else {
                            act = false;                                  // parked: the general routine takes this token
                        }
                    }
                };
                while (__any(act)) {
                    hop(r, q, false);
                    if (!__any(act)) break;
                    hop(q, r, true);
                }
                if (in_q) r = q;                                          // a hop that is not plain leaves the lane where it started
#endif
                // the general routine serves parked lanes and lanes near the end of the input
                const uint32_t pa = cstart + r;
                const bool slow = go && !merged && r < end_r && pa < len;
                if (!__any(slow)) break;
                if (slow) {
                    const uint32_t bi = r - rb0;
                    if (mode == 1 && ((ROWA((bi >> 5) & 7u) >> (bi & 31u)) & 1u)) merged = true;
                    else {
                        if (mode == 0) ROWA((bi >> 5) & 7u) |= 1u << (bi & 31u); else ROWB((bi >> 5) & 7u) |= 1u << (bi & 31u);
                        uint32_t nx;
                        if (!token_next(pa, nx)) nx = len;                // (an error on the true chain is found again by the tile stages)
                        r = nx - cstart;
                    }
                }
            }
            return r;
        };
        using M0T = std::integral_constant<int, 0>; using M1T = std::integral_constant<int, 1>;
        const bool in_input = cstart + rb0 < len;
        bool mdummy = false;
        const uint32_t x0 = walk(rb0, in_input, mdummy, M0T{});
        PT_MARK(1);
        uint32_t X = in_input ? x0 : 0u, walked = rb0, mpos = rb0;
        // the saved walks, newest first: (entry, X, mpos, row B) of results a new entry displaced.  Empty at the start of every chunk — a
        // slot of the chunk before with the same chunk-relative entry would bring back a row of other bytes.  `fresh`: the live result is
        // pass 0's, which is not worth a slot (the region start merges on its first hop).
        uint32_t sv_e[kParseMemo], sv_X[kParseMemo], sv_m[kParseMemo], sv_row[kParseMemo][8];
#pragma unroll
        for (uint32_t k = 0; k < kParseMemo; ++k) {
            sv_e[k] = kNoEntry; sv_X[k] = 0u; sv_m[k] = 0u;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) sv_row[k][i] = 0u;
        }
        bool fresh = true;
        for (uint32_t pass = 0; pass < 80u; ++pass) {
            const uint32_t entry = wave_prev(wave_scan_max(X), 0u);
            const bool redo = in_input && entry != walked && lane != 0u;
            if (!__any(redo)) break;
            // ---- the lookup, for all lanes alike (selects, no branch): the live row is read whole, the saved walk of this entry (or an
            //      empty row) takes its place, and the live result goes to the first slot — the slot that was hit, or the oldest, makes room
            uint32_t lb[8];
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) lb[i] = ROWB(i);
            bool hit = false, hitk[kParseMemo], below[kParseMemo];
#pragma unroll
            for (uint32_t k = 0; k < kParseMemo; ++k) { below[k] = hit; hitk[k] = redo && !hit && entry == sv_e[k]; hit = hit || hitk[k]; }
            PT_MEMO(redo, hit);
            uint32_t rX = 0u, rM = 0u, rrow[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t k = 0; k < kParseMemo; ++k) {
                rX = hitk[k] ? sv_X[k] : rX; rM = hitk[k] ? sv_m[k] : rM;
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) rrow[i] = hitk[k] ? sv_row[k][i] : rrow[i];
            }
            const bool put = redo && !fresh;
#pragma unroll
            for (uint32_t k = kParseMemo - 1u; k > 0u; --k) {
                const bool sh = put && !below[k];
                sv_e[k] = sh ? sv_e[k - 1u] : sv_e[k]; sv_X[k] = sh ? sv_X[k - 1u] : sv_X[k]; sv_m[k] = sh ? sv_m[k - 1u] : sv_m[k];
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) sv_row[k][i] = sh ? sv_row[k - 1u][i] : sv_row[k][i];
            }
            sv_e[0] = put ? walked : sv_e[0]; sv_X[0] = put ? X : sv_X[0]; sv_m[0] = put ? mpos : sv_m[0];
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) { sv_row[0][i] = put ? lb[i] : sv_row[0][i]; ROWB(i) = redo ? rrow[i] : lb[i]; }
            walked = redo ? entry : walked;
            fresh = fresh && !redo;
            // ---- a lane that found its entry sits the walk out, as one whose entry lies beyond its region does
            const bool wk = redo && !hit;
            const bool inreg = wk && entry < end_r && cstart + entry < len;
            bool mg = false;
            const uint32_t x1 = walk(inreg ? entry : end_r, inreg, mg, M1T{});
            if (wk) {
                if (!inreg) { X = entry; mpos = end_r; }
                else if (mg) { X = x0; mpos = x1; }
                else { X = x1; mpos = end_r; }
            } else if (hit) { X = rX; mpos = rM; }
        }
        PT_MARK(2);
        // ---- the rows and the exit
        {
            const uint32_t mb = mpos - rb0;                    // 0..256: row A is valid from this bit on
            u32x4 o0, o1;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                const uint32_t wb = mb >> 5;
                const uint32_t keep = i < wb ? 0u : i == wb ? ~((1u << (mb & 31u)) - 1u) : ~0u;
                const uint32_t v = in_input ? ((ROWA(i) & keep) | ROWB(i)) : 0u;
                if (i < 4u) o0[i] = v; else o1[i - 4u] = v;
            }
            LZF_GLOBAL u32x4* dst = (LZF_GLOBAL u32x4*)(c.bits + ((size_t)j * c.maxch + h) * kSegChunkWords + lane * 8u);
            dst[0] = o0; dst[1] = o1;
            if (!c.fed) {                                      // (the seam stage's input: the fed kernel carries the chain itself)
                const uint32_t xm = __builtin_amdgcn_readlane(wave_scan_max(X), 63);
                uint64_t xe = (uint64_t)cstart + xm;
                if (xe > len) xe = len;
                if (lane == 0u) c.xexit[(size_t)j * c.maxch + h] = (uint32_t)xe;
            }
            if (c.est) {
                // the job's sequences for the launch order: the marks this chunk owns (chunk 0 its whole row, chunk h >= 1 from kSegOverlap
                // on: the regions of lanes 8 ..), counted from the words just stored
                uint32_t cnt = 0;
                if (h == 0u || rb0 >= kSegOverlap) cnt = (uint32_t)(__popc(o0[0]) + __popc(o0[1]) + __popc(o0[2]) + __popc(o0[3]) + __popc(o1[0]) + __popc(o1[1]) + __popc(o1[2]) + __popc(o1[3]));
                const uint32_t tot = __builtin_amdgcn_readlane(wave_scan_add(cnt), 63);
                if (lane == 0u) __hip_atomic_fetch_add(&c.est[j], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        PT_MARK(3);
        PT_CHUNK();
    }
    PT_REPORT();
}

#undef ROWA
#undef ROWB
#undef PT_START
#undef PT_MARK
#undef PT_CHUNK
#undef PT_HOP_ASM
#undef PT_HOPS
#undef PT_MEMO
#undef PT_REPORT

// =====================================================================================================================
// seam: from which position on is a chunk's chain the true one
// =====================================================================================================================
__global__ __launch_bounds__(64) void lzf_seg_seam_kernel(seg_ctx c) {
    __shared__ uint16_t patch[kSegStride / 3u + 8u];
    constexpr uint32_t kWin = 2048;                                   // compressed bytes a staged window covers
    __shared__ __attribute__((aligned(16))) uint8_t wbytes[kWin + 128u];
    __shared__ uint32_t wbits[kWin / 32u + 2u];
    if (blockIdx.x >= c.g_n) return;
    const uint32_t j = c.grouped ? seg_job_of(c, blockIdx.x) : blockIdx.x;
    const seg_job sj = c.st[j];
    if (!sj.eligible) return;
    const uint32_t lane = threadIdx.x & 63u;
    const lzf_decompress_job job = c.jobs[j];
    cgu8* __restrict__ in = as_global(job.input);
    const uint32_t len = (uint32_t)job.input_len;
    LZF_GLOBAL uint32_t* const X = (LZF_GLOBAL uint32_t*)c.xexit + (size_t)j * c.maxch;
    LZF_GLOBAL uint32_t* const VF = (LZF_GLOBAL uint32_t*)c.vfrom + (size_t)j * c.maxch;
    LZF_GLOBAL uint32_t* const B = (LZF_GLOBAL uint32_t*)c.bits + (size_t)j * c.maxch * kSegChunkWords;
    auto bit = [&](uint32_t h, uint32_t pos) -> bool {          // pos inside chunk h's range
        const uint32_t r = pos - h * kSegStride;
        return (B[(size_t)h * kSegChunkWords + (r >> 5)] >> (r & 31u)) & 1u;
    };
    if (lane == 0u) VF[0] = 0u;
    bool carry_valid = false; uint32_t carry_e = 0;
    bool failed = false;
    for (uint32_t h0 = 1; h0 < sj.nch && !failed; h0 += 64u) {
        const uint32_t gn = sj.nch - h0 < 64u ? sj.nch - h0 : 64u;
        const uint32_t h = h0 + lane;
        const bool act = lane < gn;
        const uint32_t e = act ? X[h - 1u] : 0u;
        const uint32_t endh = h * kSegStride + kSegChunk;
        // 0: the true chain (if it enters at e) is on this chunk's chain from e on; 1: it jumps over the chunk; 2: neither
        uint32_t code = 0;
        if (act) code = (e >= len || e >= endh) ? 1u : (bit(h, e) ? 0u : 2u);
        uint32_t k = 0;
        while (k < gn && !failed) {
            uint32_t e_true;
            if (!carry_valid) {
                const uint32_t kk0 = first_lane(__ballot(act && lane >= k && code != 0u));
                const uint32_t kk = kk0 < gn ? kk0 : gn;
                if (act && lane >= k && lane < kk) VF[h] = e;
                k = kk;
                if (k >= gn) break;
                e_true = __builtin_amdgcn_readlane(e, k);
            } else e_true = carry_e;
            // ---- chunk hk entered at e_true
            const uint32_t hk = h0 + k;
            const uint32_t base = hk * kSegStride, endk = base + kSegChunk, ostart = base + kSegOverlap;
            if (e_true >= len || e_true >= endk) {
                if (lane == 0u) VF[hk] = kNone;
                carry_valid = true; carry_e = e_true;
            } else if (bit(hk, e_true)) {
                if (lane == 0u) VF[hk] = e_true;
                carry_valid = false;
            } else {
                // walk the true chain until it steps on a marked token of this chunk (or leaves the chunk)
                // (windows of 2 KiB of the input and of the chunk's marks are staged in LDS, so a hop costs LDS reads)
                uint32_t p = e_true, np = 0, mg = 0, err = 0;
                while (p < endk && p < len && !mg && !err) {
                    const uint32_t ws = p;
                    __syncthreads();
                    {
                        const uint32_t avail = len - ws < kWin + 128u ? len - ws : kWin + 128u;
                        for (uint32_t i = lane * 16u; i < kWin + 128u; i += 1024u) {
                            u32x4 v = u32x4{0, 0, 0, 0};
                            if (i + 16u <= avail) v = ld16(in + ws + i);
                            else if (i < avail) { for (uint32_t b = 0; i + b < avail; ++b) v[(b >> 2) & 3u] |= (uint32_t)in[ws + i + b] << ((b & 3u) * 8u); }
                            *reinterpret_cast<u32x4*>(&wbytes[i]) = v;
                        }
                        const uint32_t w0 = (ws - base) >> 5;                       // first word of the marks the window needs
                        for (uint32_t i = lane; i < kWin / 32u + 2u; i += 64u)
                            wbits[i] = w0 + i < kSegChunkWords ? B[(size_t)hk * kSegChunkWords + w0 + i] : 0u;
                    }
                    __syncthreads();
                    if (lane == 0u) {
                        const uint32_t wb_a = lds_addr(wbytes);
                        auto rdb = [&](uint32_t q) -> uint32_t { const uint32_t r_ = q - ws; if (r_ < kWin + 128u) return (uint32_t)wbytes[r_]; return (uint32_t)in[q]; };
                        auto rd8 = [&](uint32_t q) -> uint64_t { const uint32_t r_ = q - ws; if (r_ + 8u <= kWin + 128u) return lds_ld64u(wb_a + r_); return ld8(in + q); };
                        const uint32_t bit0 = ((ws - base) >> 5) << 5;             // chunk-relative position of bit 0 of wbits[0]
                        while (p < endk && p < len && p - ws < kWin) {
                            const uint32_t rbit = p - base - bit0;
                            if (p != e_true && ((wbits[rbit >> 5] >> (rbit & 31u)) & 1u)) { mg = 1; break; }
                            patch[np++] = (uint16_t)(p - ostart);
                            uint32_t nx;
                            // the common token — lengths with at most one extension byte, everything staged, not the input's end — from
                            // one unaligned LDS word (+ one byte): the position token_next_gen returns, at a quarter of its instructions
                            {
                                uint32_t w;
                                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(wb_a + (p - ws)) : "memory");
                                const uint32_t L0 = (w >> 4) & 15u, M0 = w & 15u, b1 = (w >> 8) & 255u;
                                const uint32_t q2 = p + 1u + (L0 == 15u ? 1u + 15u + b1 : L0);       // the offset's position
                                if (!(L0 == 15u && b1 == 255u) && q2 + 3u <= len && q2 - ws + 3u <= kWin + 128u &&
                                    !(M0 == 15u && wbytes[q2 + 2u - ws] == 255u)) { p = q2 + 2u + (M0 == 15u ? 1u : 0u); continue; }
                            }
                            if (!token_next_gen(len, p, nx, rd8, rdb)) { err = 1; break; }
                            p = nx;
                        }
                    }
                    p = __builtin_amdgcn_readfirstlane(p); np = __builtin_amdgcn_readfirstlane(np);
                    mg = __builtin_amdgcn_readfirstlane(mg); err = __builtin_amdgcn_readfirstlane(err);
                }
                if (err) { failed = true; break; }
                uint32_t m = mg ? p : endk;
                // clear this chunk's marks in [ostart, m), then set the walked tokens
                {
                    const uint32_t w0 = kSegOverlap / 32u, mr = m - base;      // mr in (kSegOverlap, kSegChunk]
                    for (uint32_t w = w0 + lane; w * 32u < mr; w += 64u) {
                        LZF_GLOBAL uint32_t* wp = &B[(size_t)hk * kSegChunkWords + w];
                        if (w * 32u + 32u <= mr) *wp = 0u;
                        else *wp &= ~((1u << (mr & 31u)) - 1u);
                    }
                    __threadfence();
                    for (uint32_t i = lane; i < np; i += 64u) {
                        const uint32_t r = (uint32_t)patch[i] + kSegOverlap;
                        atomicOr((uint32_t*)&B[(size_t)hk * kSegChunkWords + (r >> 5)], 1u << (r & 31u));
                    }
                    __threadfence();
                }
                if (lane == 0u) VF[hk] = ostart;
                if (mg) carry_valid = false; else { carry_valid = true; carry_e = p; }
            }
            ++k;
        }
    }
    if (failed && lane == 0u) c.st[j].failed = 1u;
}

}  // namespace lzf

#ifdef LZF_DBG_PARSE_TIME
// Analysis only: the section sums and counts of lzf_seg_parse_kernel since the last call with `reset` (out10 may be NULL).
extern "C" int lzf_debug_parse_timers(unsigned long long* out10, int reset) {
    if (out10 && hipMemcpyFromSymbol(out10, HIP_SYMBOL(lzf::lzf_dbg_parse_cycles), sizeof(unsigned long long) * 10u) != hipSuccess) return LZF_E_HIP;
    const unsigned long long z[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(lzf::lzf_dbg_parse_cycles), z, sizeof(z)) != hipSuccess) return LZF_E_HIP;
    return LZF_OK;
}
#endif
