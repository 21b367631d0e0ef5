// lz4_seg_resolve.hip — the last stage of the segmented pipeline (lzf_seg_common.h, kernels.h): the records of lz4_seg_tiles.hip resolved,
// a pair of wavefronts per block.
#include "lzf_seg_common.h"

namespace lzf {

// =====================================================================================================================
// resolve: the dependent match copies of a block — a pair of wavefronts per block
// =====================================================================================================================
// Biased positions y = x + rb (rb = out & 15): y % 16 == 0 <=> out + x is 16-byte aligned; ring index = y & (R - 1).
// The STAGER (wave 1) does everything that is not the dependency chain: the ring's granules in from `out` (the literals are
// there), finished granules out to HBM, the few sources that are older than the ring (class 7: from HBM), sequences larger
// than a sub-batch (class 8: HBM -> HBM, then the ring's history is read back).  The RESOLVER (wave 0) runs the rounds of
// sub-batch after sub-batch: one LDS round trip per dependency level.  Both read the records (records stage) from HBM on
// their own, two batches ahead of their use.
// Tickets = sub-batches in stream order: the stager publishes ticket t with ctl[0] = t + 1 after its LDS writes, the
// resolver answers ctl[1] = t + 1 after its own; LDS executes one wave's accesses in order, so a flag is never seen before
// the data.  The stager runs at most NT tickets and NS sub-batch spans of output ahead (and loads the granules behind its fill pointer one sub-batch early);
// the records stage classed the sources with that fetch-ahead in mind.
template <int R>
__global__ __launch_bounds__(128) void lzf_seg_resolve_pair_kernel(seg_ctx c) {
    constexpr uint32_t kMask = (uint32_t)R - 1u;
    constexpr uint32_t kSpan = (uint32_t)R / 8u;       // output bytes one sub-batch may produce
    constexpr uint32_t NS = 3;                         // sub-batch spans of output the stager may be ahead (what the records stage classed the sources for)
    constexpr uint32_t NT = 32;                        // tickets it may be ahead (a text block's sub-batch is a batch, ~1 KiB: three were 6 us of slack, less than HBM answers in under load)
    // (the ring starts 64 bytes into the workgroup's LDS: an address 32 bytes in front of a ring position is never negative)
    __shared__ __attribute__((aligned(16))) uint8_t lds_all[64 + R];
    uint8_t* const ring = lds_all + 64;
    uint32_t* const ctl = reinterpret_cast<uint32_t*>(lds_all);      // [0] staged tickets, [1] resolved tickets, [3] a wave gave up
    if (blockIdx.x >= c.g_n) return;
    const uint32_t j = c.order ? c.order[c.g_off + blockIdx.x] : c.grouped ? seg_job_of(c, blockIdx.x) : blockIdx.x;
    const seg_job sj = c.st[j];
    if (!sj.eligible || sj.failed) return;
    if (c.ring_bytes != (uint32_t)R) return;           // (the records were classed for another ring: leave the job to the pair kernel)
    if (c.res_prio) __builtin_amdgcn_s_setprio(3);     // the block's chain: ahead of the throughput kernels that share the SIMD
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const lzf_decompress_job job = c.jobs[j];
    const long long t_start = clock64();
    gu8* const out = as_global(job.out);
    const uint32_t rb = (uint32_t)(reinterpret_cast<uintptr_t>(out) & 15u);
    gu8* const outb = out - rb;
    const LZF_GLOBAL u32x4* const recs = (const LZF_GLOBAL u32x4*)c.recs + sj.rec_off;
    const uint32_t n = sj.ntok, total = sj.outb;
    const uint32_t ring_a = lds_addr(ring);
    if (threadIdx.x < 4u) ctl[threadIdx.x] = 0u;
    __syncthreads();
    // the flags, by explicit DS instructions (a volatile pointer to ctl[] is a generic pointer to hipcc: FLAT accesses, which
    // wait for every global load in flight as well)
    const uint32_t ctl_a = lds_addr(ctl);
    auto flag_get = [&](uint32_t i) -> uint32_t { uint32_t v; asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(ctl_a + 4u * i) : "memory"); return __builtin_amdgcn_readfirstlane(v); };
    auto flag_set = [&](uint32_t i, uint32_t v) { asm volatile("s_waitcnt lgkmcnt(0)\n\tds_write_b32 %0, %1" ::"v"(ctl_a + 4u * i), "v"(v) : "memory"); };
    // Nap until arrived() says yes.  Bounded: a wait of ~2^22 naps (seconds; a ticket takes microseconds) can only mean a
    // defect, so the wave gives up and raises ctl[3]; both waves then leave, the job is not marked done and the pair kernel
    // (launched after this one) decodes it.  false = give up.
    auto wait_until = [&](auto arrived) -> bool {
        for (uint32_t spin = 0;; ++spin) {
            if (arrived()) return true;
            if ((spin & 63u) == 63u && (flag_get(3) != 0u || spin > (1u << 22))) { if (lane == 0u) flag_set(3, 1u); return false; }
            __builtin_amdgcn_s_sleep(1);
        }
    };
    auto flag_wait_above = [&](uint32_t i, uint32_t below) -> bool { return wait_until([&]() -> bool { return flag_get(i) > below; }); };

    // ring[d, d + nbytes) <- ring[s, s + nbytes): source final, ranges disjoint; all lanes, 8 bytes each, the last unit moved
    // back to end with the range (it overlaps its neighbour with the same bytes): one LDS round trip per 512 bytes
    auto ring_copy = [&](uint32_t d, uint32_t s_, uint32_t nbytes) {
        if (nbytes >= 8u) {
            const uint32_t nu = (nbytes + 7u) >> 3;
            for (uint32_t u = lane; u < nu; u += kWave) {
                const uint32_t o = 8u * u + 8u <= nbytes ? 8u * u : nbytes - 8u;
                const uint32_t sa = (s_ + o) & kMask, da = (d + o) & kMask;
                if (sa + 8u <= (uint32_t)R && da + 8u <= (uint32_t)R) lds_st64(ring_a + da, lds_ld64u(ring_a + sa));
                else for (uint32_t t = 0; t < 8u; ++t) ring[(da + t) & kMask] = ring[(sa + t) & kMask];
            }
        } else if (lane < nbytes) ring[(d + lane) & kMask] = ring[(s_ + lane) & kMask];
    };
    // copy_overlapping (decompress.rs:80-138) inside the ring: out[d + t] = out[d - off + t], t < M.  The bytes already
    // copied double the source every step (a multiple of the period is a period).
    auto ring_match = [&](uint32_t d, uint32_t off_, uint32_t M_) {
        uint32_t pos = 0, av = off_;
        while (pos < M_) { const uint32_t cc = av < M_ - pos ? av : M_ - pos; ring_copy(d + pos, d - off_, cc); pos += cc; av += cc; }
    };

    if (role == 0u) {
        // ================================================ RESOLVER ================================================
#ifdef LZF_SEG_TIME
        long long tm_wait = 0, tm_setup = 0, tm_asm = 0, tm_slow = 0, tm_t = clock64(); uint32_t n_rounds = 0;
#define RT(var) do { const long long t__ = clock64(); var += t__ - tm_t; tm_t = t__; } while (0)
#else
#define RT(var) do { } while (0)
#endif
        uint32_t t = 0, staged = 0;                       // tickets resolved; tickets known to be staged (the flag as last read)
        // the records come straight from HBM, two batches ahead (the only loads of this wave: they return in order and in time)
        u32x4 rA = u32x4{0, 0, 0, 0}, rB = u32x4{0, 0, 0, 0};
        if (n) { rA = recs[lane < n ? lane : n - 1u]; rB = recs[64u + lane < n ? 64u + lane : n - 1u]; }
        auto wait_staged = [&](uint32_t tt) -> bool {    // ticket tt published?  (one read of the flag usually covers several tickets)
            if (staged > tt) return true;
            return wait_until([&]() -> bool { staged = flag_get(0); return staged > tt; });
        };
        for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
            const uint32_t nb = n - i0 < 64u ? n - i0 : 64u;
            const u32x4 r = rA;
            asm volatile("" ::: "memory");
            rA = rB;
            { const uint32_t ix = i0 + 128u + lane; rB = recs[ix < n ? ix : n - 1u]; }
            asm volatile("" ::: "memory");
            RT(tm_setup);
            if (!wait_staged(t)) break;
            RT(tm_wait);
            const uint32_t M = r[0], dy = r[1], off = r[3];
            const uint32_t sub = lane < nb ? (r[2] & 0xFFu) : 0xFFu, lvl = (r[2] >> 16) & 255u, cls = lane < nb ? r[2] >> 24 : 0u;
            const uint32_t nsub = __builtin_amdgcn_readlane(r[2] & 0xFFu, (nb - 1u) & 63u) + 1u;
            const uint32_t sa = ring_a + ((dy - off) & kMask), da = ring_a + (dy & kMask);
            // two-ended pieces: A (4..7) = 4-byte pieces at 0 and M - 4; B1 (8..16) = 8-byte pieces at 0 and M - 8;
            // B2 (17..32) adds 8 and M - 16; C (33..64) adds 16, 24, M - 32, M - 24
            const uint32_t o3 = M - 8u, a1 = M - 4u;
#if !defined(LZF_SEG_NOASM) && !defined(LZF_SEG_DBG_SKIP) && !defined(LZF_SEG_NORLE)
            // classes 9..12: run-length matches (offset 1, 2 or 4) of the same four sizes — stored like 1..4, the registers filled
            // with the pattern (the first bytes read, spread by v_perm_b32; rotated for the piece that ends the match)
            const uint32_t fl = r[2] >> 8;              // (the records stage's flags; padding lanes carry none)
            const unsigned long long mA_b = __ballot((fl & 1u) != 0u), m2_b = __ballot((fl & 2u) != 0u), m3_b = __ballot((fl & 4u) != 0u),
                                     m4_b = __ballot((fl & 8u) != 0u), mS_b = __ballot((fl & 16u) != 0u), mR_b = __ballot((fl & 32u) != 0u);
            uint32_t rsel = 0, rsh = 0;                  // (only batches with run-length lanes pay for these)
            if (mR_b) { rsel = off == 1u ? 0u : off == 2u ? 0x01000100u : 0x03020100u; rsh = M & (off - 1u); }
#else
            // (the compiler's loop: the run-length classes take the general path (a) below)
            const unsigned long long mA_b = __ballot(cls == 1u), m2_b = __ballot(cls >= 2u && cls <= 4u), m3_b = __ballot(cls == 3u || cls == 4u),
                                     m4_b = __ballot(cls == 4u), mS_b = __ballot(cls == 5u || cls == 6u || (cls >= 9u && cls <= 12u));
#ifdef LZF_SEG_NORLE
            const unsigned long long mR_b = 0; const uint32_t rsel = 0, rsh = 0;
#endif
#endif
            bool gave_up = false;
            for (uint32_t s_i = 0; s_i < nsub; ++s_i, ++t) {
#ifdef LZF_ANALYSIS      // LZF_SEG_FORCE=resolver: the resolver of every odd job gives up at its third ticket (test of the hand-over)
                if (c.dbg_force == 2u && (j & 1u) && t >= 2u) { if (lane == 0u) flag_set(3, 1u); gave_up = true; break; }
#endif
                // ---- wait for the stager's ticket
                if (s_i) {
                    RT(tm_setup);
                    if (!wait_staged(t)) { gave_up = true; break; }
                    RT(tm_wait);
                }
                const unsigned long long msub = nsub == 1u ? ~0ull : __ballot(sub == s_i);
                unsigned long long todo = (mA_b | m2_b | mS_b) & msub;
#if defined(LZF_SEG_DBG_SKIP) && LZF_SEG_DBG_SKIP == 2      // analysis: no rounds at all (what a batch costs without them)
                todo = 0;
#endif
                for (uint32_t lv = 1; todo; ++lv) {
                    unsigned long long ml;
#if !defined(LZF_SEG_NOASM) && !defined(LZF_SEG_DBG_SKIP)
                    // The rounds of the two-ended classes in one hand-scheduled loop: a lone wavefront retires an instruction every
                    // 5 to 8 cycles, so a round is priced by its instruction count (about 20 scalar instructions + the DS pairs of
                    // the classes present; what hipcc makes of the loop below is 45 + 8 EXEC moves).  It returns after a level
                    // that has lanes of class 5/6 (`ts`; the level's other lanes done) for the code below.  v100..v117: the
                    // pieces in flight, fixed registers so that the halves of a pair can be named.
                    unsigned long long ts;
                    {
                        unsigned long long sv;
                        lv = __builtin_amdgcn_readfirstlane(lv);
                        // (two copies: batches without run-length and class-5/6 lanes — most of a text block's — skip those checks)
                        if ((mR_b | mS_b) & msub)
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            ".p2align 6\n\t"                                     // (the loop starts an instruction-cache line: its time must not depend on what is compiled around it)
                            "Lloop%=:\n\t"
                            "v_cmp_eq_u32_e32 vcc, %[lv], %[vl]\n\t"
                            "s_add_u32 %[lv], %[lv], 1\n\t"
                            "s_and_b64 %[ml], vcc, %[todo]\n\t"
                            "s_cbranch_scc0 Lempty%=\n\t"
#ifdef LZF_SEG_TIME
                            "s_add_u32 %[nr], %[nr], 1\n\t"
#endif
                            "s_and_b64 exec, %[ml], %[mA]\n\t"
                            "ds_read_b32 v116, %[sa]\n\t"
                            "ds_read_b32 v117, %[tsrc] offset:28\n\t"
                            "s_and_b64 exec, %[ml], %[m2]\n\t"
                            "ds_read_b64 v[100:101], %[sa]\n\t"
                            "ds_read_b64 v[106:107], %[tsrc] offset:24\n\t"
                            "s_and_b64 exec, %[ml], %[m3]\n\t"
                            "s_cbranch_execz Lr%=\n\t"
                            "ds_read_b64 v[102:103], %[sa] offset:8\n\t"
                            "ds_read_b64 v[104:105], %[tsrc] offset:16\n\t"
                            "s_and_b64 exec, %[ml], %[m4]\n\t"
                            "s_cbranch_execz Lr%=\n\t"
                            "ds_read_b64 v[108:109], %[sa] offset:16\n\t"
                            "ds_read_b64 v[110:111], %[sa] offset:24\n\t"
                            "ds_read_b64 v[112:113], %[tsrc]\n\t"
                            "ds_read_b64 v[114:115], %[tsrc] offset:8\n\t"
                            "Lr%=:\n\t"
                            "s_and_b64 exec, %[ml], %[mR]\n\t"
#ifndef LZF_SEG_DBG_NOWAIT                                         // (analysis: the round without its LDS latency; wrong bytes)
                            "s_waitcnt lgkmcnt(0)\n\t"
#endif
                            "s_cbranch_execz Lnr%=\n\t"
                            // run-length lanes: the pattern (what was read at the source, spread over the word) in every piece
                            // from the front, the pattern rotated by M mod offset in every piece that ends with the match
                            "v_perm_b32 v116, v116, v116, %[rsel]\n\t"
                            "v_perm_b32 v100, v100, v100, %[rsel]\n\t"
                            "v_alignbyte_b32 v117, v116, v116, %[rsh]\n\t"
                            "v_alignbyte_b32 v106, v100, v100, %[rsh]\n\t"
                            "v_mov_b32 v101, v100\n\t"
                            "v_mov_b32 v107, v106\n\t"
                            "v_mov_b64 v[102:103], v[100:101]\n\t"
                            "v_mov_b64 v[104:105], v[106:107]\n\t"
                            "v_mov_b64 v[108:109], v[100:101]\n\t"
                            "v_mov_b64 v[110:111], v[100:101]\n\t"
                            "v_mov_b64 v[112:113], v[106:107]\n\t"
                            "v_mov_b64 v[114:115], v[106:107]\n\t"
                            "Lnr%=:\n\t"
                            "s_and_b64 exec, %[ml], %[mA]\n\t"
                            "ds_write_b32 %[da], v116\n\t"
                            "ds_write_b32 %[tdst], v117 offset:28\n\t"
                            "s_and_b64 exec, %[ml], %[m2]\n\t"
                            "ds_write_b64 %[da], v[100:101]\n\t"
                            "ds_write_b64 %[tdst], v[106:107] offset:24\n\t"
                            "s_and_b64 exec, %[ml], %[m3]\n\t"
                            "s_cbranch_execz Lw%=\n\t"
                            "ds_write_b64 %[da], v[102:103] offset:8\n\t"
                            "ds_write_b64 %[tdst], v[104:105] offset:16\n\t"
                            "s_and_b64 exec, %[ml], %[m4]\n\t"
                            "s_cbranch_execz Lw%=\n\t"
                            "ds_write_b64 %[da], v[108:109] offset:16\n\t"
                            "ds_write_b64 %[da], v[110:111] offset:24\n\t"
                            "ds_write_b64 %[tdst], v[112:113]\n\t"
                            "ds_write_b64 %[tdst], v[114:115] offset:8\n\t"
                            "Lw%=:\n\t"
                            "s_mov_b64 exec, %[sv]\n\t"
                            "s_and_b64 %[ts], %[ml], %[mS]\n\t"
                            "s_cbranch_scc1 Lout%=\n\t"
                            "s_andn2_b64 %[todo], %[todo], %[ml]\n\t"
                            "s_cbranch_scc1 Lloop%=\n\t"
                            "s_branch Lout%=\n\t"
                            "Lempty%=:\n\t"
                            "s_mov_b64 %[ts], 0\n\t"
                            "s_cmp_le_u32 %[lv], 71\n\t"
                            "s_cbranch_scc1 Lloop%=\n\t"
                            "Lout%=:\n\t"
                            : [sv] "=&s"(sv), [ts] "=&s"(ts), [ml] "=&s"(ml), [todo] "+s"(todo), [lv] "+s"(lv)
#ifdef LZF_SEG_TIME
                              , [nr] "+s"(n_rounds)
#endif
                            : [mA] "s"(mA_b), [m2] "s"(m2_b), [m3] "s"(m3_b), [m4] "s"(m4_b), [mS] "s"(mS_b), [mR] "s"(mR_b), [vl] "v"(lvl), [rsel] "v"(rsel), [rsh] "v"(rsh),
                              [sa] "v"(sa), [tsrc] "v"(sa + M - 32u),
                              [da] "v"(da), [tdst] "v"(da + M - 32u)
                            : "memory", "vcc", "scc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113",
                              "v114", "v115", "v116", "v117");
                        else
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            "s_mov_b64 %[ts], 0\n\t"
                            ".p2align 6\n\t"                                     // (the loop starts an instruction-cache line: its time must not depend on what is compiled around it)
                            "Lloop%=:\n\t"
                            "v_cmp_eq_u32_e32 vcc, %[lv], %[vl]\n\t"
                            "s_add_u32 %[lv], %[lv], 1\n\t"
                            "s_and_b64 %[ml], vcc, %[todo]\n\t"
                            "s_cbranch_scc0 Lempty%=\n\t"
#ifdef LZF_SEG_TIME
                            "s_add_u32 %[nr], %[nr], 1\n\t"
#endif
                            "s_and_b64 exec, %[ml], %[mA]\n\t"
                            "ds_read_b32 v116, %[sa]\n\t"
                            "ds_read_b32 v117, %[tsrc] offset:28\n\t"
                            "s_and_b64 exec, %[ml], %[m2]\n\t"
                            "ds_read_b64 v[100:101], %[sa]\n\t"
                            "ds_read_b64 v[106:107], %[tsrc] offset:24\n\t"
                            "s_and_b64 exec, %[ml], %[m3]\n\t"
                            "s_cbranch_execz Lr%=\n\t"
                            "ds_read_b64 v[102:103], %[sa] offset:8\n\t"
                            "ds_read_b64 v[104:105], %[tsrc] offset:16\n\t"
                            "s_and_b64 exec, %[ml], %[m4]\n\t"
                            "s_cbranch_execz Lr%=\n\t"
                            "ds_read_b64 v[108:109], %[sa] offset:16\n\t"
                            "ds_read_b64 v[110:111], %[sa] offset:24\n\t"
                            "ds_read_b64 v[112:113], %[tsrc]\n\t"
                            "ds_read_b64 v[114:115], %[tsrc] offset:8\n\t"
                            "Lr%=:\n\t"
                            "s_waitcnt lgkmcnt(0)\n\t"
                            "s_and_b64 exec, %[ml], %[mA]\n\t"
                            "ds_write_b32 %[da], v116\n\t"
                            "ds_write_b32 %[tdst], v117 offset:28\n\t"
                            "s_and_b64 exec, %[ml], %[m2]\n\t"
                            "ds_write_b64 %[da], v[100:101]\n\t"
                            "ds_write_b64 %[tdst], v[106:107] offset:24\n\t"
                            "s_and_b64 exec, %[ml], %[m3]\n\t"
                            "s_cbranch_execz Lw%=\n\t"
                            "ds_write_b64 %[da], v[102:103] offset:8\n\t"
                            "ds_write_b64 %[tdst], v[104:105] offset:16\n\t"
                            "s_and_b64 exec, %[ml], %[m4]\n\t"
                            "s_cbranch_execz Lw%=\n\t"
                            "ds_write_b64 %[da], v[108:109] offset:16\n\t"
                            "ds_write_b64 %[da], v[110:111] offset:24\n\t"
                            "ds_write_b64 %[tdst], v[112:113]\n\t"
                            "ds_write_b64 %[tdst], v[114:115] offset:8\n\t"
                            "Lw%=:\n\t"
                            "s_mov_b64 exec, %[sv]\n\t"
                            "s_andn2_b64 %[todo], %[todo], %[ml]\n\t"
                            "s_cbranch_scc1 Lloop%=\n\t"
                            "s_branch Lout%=\n\t"
                            "Lempty%=:\n\t"
                            "s_mov_b64 %[ts], 0\n\t"
                            "s_cmp_le_u32 %[lv], 71\n\t"
                            "s_cbranch_scc1 Lloop%=\n\t"
                            "Lout%=:\n\t"
                            : [sv] "=&s"(sv), [ts] "=&s"(ts), [ml] "=&s"(ml), [todo] "+s"(todo), [lv] "+s"(lv)
#ifdef LZF_SEG_TIME
                              , [nr] "+s"(n_rounds)
#endif
                            : [mA] "s"(mA_b), [m2] "s"(m2_b), [m3] "s"(m3_b), [m4] "s"(m4_b), [mS] "s"(mS_b), [mR] "s"(mR_b), [vl] "v"(lvl), [rsel] "v"(rsel), [rsh] "v"(rsh),
                              [sa] "v"(sa), [tsrc] "v"(sa + M - 32u),
                              [da] "v"(da), [tdst] "v"(da + M - 32u)
                            : "memory", "vcc", "scc", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113",
                              "v114", "v115", "v116", "v117");
                        RT(tm_asm);
                        // (hipcc takes what an asm statement returns for divergent, whatever the register class)
                        auto uni = [](unsigned long long x) { return (unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)x) | ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32); };
                        ts = uni(ts); ml = uni(ml); todo = uni(todo); lv = __builtin_amdgcn_readfirstlane(lv);
                        if (!ts) break;                  // nothing left (or levels that do not end: not our records)
                        todo &= ~ml;                     // (a level left for its class-5/6 lanes is still in `todo`)
                        --lv;                            // (the loop's increment follows)
                    }
#else
                    ml = __ballot(lvl == lv) & todo;
                    if (!ml) { if (lv > 70u) break; continue; }
                    todo &= ~ml;
#endif
#if !defined(LZF_SEG_NOASM) && !defined(LZF_SEG_DBG_SKIP)
                    const unsigned long long mA = 0, m2 = 0, m3 = 0, m4 = 0, mS = ts;
#else
#ifdef LZF_SEG_TIME
                    ++n_rounds;
#endif
                    const unsigned long long mA = ml & mA_b, m2 = ml & m2_b, m3 = ml & m3_b, m4 = ml & m4_b, mS = ml & mS_b;
#endif
                    RT(tm_setup);
#if defined(LZF_SEG_DBG_SKIP) && LZF_SEG_DBG_SKIP == 1      // analysis: the level loop without its copies (what the control around a round costs)
                    continue;
#endif
                    if (mA | m2) {
                        uint64_t v0, v1, v2, v3, v4, v5, v6, v7; uint32_t va0, va1; unsigned long long sv;
                        asm volatile(
                            "s_mov_b64 %[sv], exec\n\t"
                            "s_mov_b64 exec, %[mA]\n\t"
                            "ds_read_b32 %[va0], %[sa]\n\t"
                            "ds_read_b32 %[va1], %[s1]\n\t"
                            "s_mov_b64 exec, %[m2]\n\t"
                            "ds_read_b64 %[v0], %[sa]\n\t"
                            "ds_read_b64 %[v3], %[s3]\n\t"
                            "s_mov_b64 exec, %[m3]\n\t"
                            "s_cbranch_execz Lr3%=\n\t"
                            "ds_read_b64 %[v1], %[sa] offset:8\n\t"
                            "ds_read_b64 %[v2], %[s16]\n\t"
                            "s_mov_b64 exec, %[m4]\n\t"
                            "s_cbranch_execz Lr3%=\n\t"
                            "ds_read_b64 %[v4], %[sa] offset:16\n\t"
                            "ds_read_b64 %[v5], %[sa] offset:24\n\t"
                            "ds_read_b64 %[v6], %[s32]\n\t"
                            "ds_read_b64 %[v7], %[s32] offset:8\n\t"
                            "Lr3%=:\n\t"
                            "s_waitcnt lgkmcnt(0)\n\t"
                            "s_mov_b64 exec, %[mA]\n\t"
                            "ds_write_b32 %[da], %[va0]\n\t"
                            "ds_write_b32 %[d1], %[va1]\n\t"
                            "s_mov_b64 exec, %[m2]\n\t"
                            "ds_write_b64 %[da], %[v0]\n\t"
                            "ds_write_b64 %[d3], %[v3]\n\t"
                            "s_mov_b64 exec, %[m3]\n\t"
                            "s_cbranch_execz Lw3%=\n\t"
                            "ds_write_b64 %[da], %[v1] offset:8\n\t"
                            "ds_write_b64 %[d16], %[v2]\n\t"
                            "s_mov_b64 exec, %[m4]\n\t"
                            "s_cbranch_execz Lw3%=\n\t"
                            "ds_write_b64 %[da], %[v4] offset:16\n\t"
                            "ds_write_b64 %[da], %[v5] offset:24\n\t"
                            "ds_write_b64 %[d32], %[v6]\n\t"
                            "ds_write_b64 %[d32], %[v7] offset:8\n\t"
                            "Lw3%=:\n\t"
                            "s_mov_b64 exec, %[sv]\n\t"
                            : [v0] "=&v"(v0), [v1] "=&v"(v1), [v2] "=&v"(v2), [v3] "=&v"(v3), [v4] "=&v"(v4), [v5] "=&v"(v5), [v6] "=&v"(v6), [v7] "=&v"(v7),
                              [va0] "=&v"(va0), [va1] "=&v"(va1), [sv] "=&s"(sv)
                            : [mA] "s"(mA), [m2] "s"(m2), [m3] "s"(m3), [m4] "s"(m4), [sa] "v"(sa), [s1] "v"(sa + a1), [s3] "v"(sa + o3), [s16] "v"(sa + M - 16u), [s32] "v"(sa + M - 32u),
                              [da] "v"(da), [d1] "v"(da + a1), [d3] "v"(da + o3), [d16] "v"(da + M - 16u), [d32] "v"(da + M - 32u)
                            : "memory");
                    }
                    RT(tm_asm);
                    if (mS) {
                        // (this path is rare: its operands pass through an empty asm statement, or hipcc computes its predicates and
                        //  addresses — some forty instructions — in the prologue of every batch)
                        uint32_t M_s = M, off_s = off, dy_s = dy;
                        asm volatile("" : "+v"(M_s), "+v"(off_s), "+v"(dy_s));
                        const uint32_t M = M_s, off = off_s, dy = dy_s;
                        const uint32_t sa = ring_a + ((dy - off) & kMask), da = ring_a + (dy & kMask);
                        const bool nowS = (mS >> lane) & 1ull;
                        const bool fits = nowS && (((dy - off) & kMask) + M <= (uint32_t)R) && ((dy & kMask) + M <= (uint32_t)R);   // neither range wraps
                        // (a) run-length matches (offset 1, 2 or 4): the pattern from one read, stores only.  Up to 64 bytes in
                        // the lane; longer ones by the whole wave, one after the other (512 bytes a step), the lane's own
                        // store finishing the odd end
                        const bool rle = fits && (off == 1u || off == 2u || off == 4u);
                        if (__ballot(rle)) {
                            uint32_t w = 0;
                            if (rle) {
                                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(sa) : "memory");
                                if (off == 1u) w = (w & 0xFFu) * 0x01010101u; else if (off == 2u) w = (w & 0xFFFFu) * 0x00010001u;
                                const uint64_t pat = (uint64_t)w | ((uint64_t)w << 32);
                                if (M >= 8u) {
                                    if (M <= 64u) for (uint32_t k = 0; k + 8u < M; k += 8u) lds_st64(da + k, pat);
                                    // the last piece ends exactly at M: its phase is (M - 8) mod off (off divides 8): rotate by bytes
                                    const uint32_t ph = (M - 8u) & (off - 1u);
                                    const uint64_t rot = ph ? (pat >> (8u * ph)) | (pat << (64u - 8u * ph)) : pat;
                                    lds_st64(da + M - 8u, rot);
                                } else {
                                    lds_st32(da, w);
                                    const uint32_t ph = (M - 4u) & (off - 1u);
                                    lds_st32(da + M - 4u, ph ? (uint32_t)(pat >> (8u * ph)) : w);
                                }
                            }
                            for (unsigned long long m = __ballot(rle && M > 64u); m; m &= m - 1ull) {
                                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                                const uint32_t qd = __builtin_amdgcn_readlane(da, q), qM = __builtin_amdgcn_readlane(M, q);
                                const uint32_t qw = __builtin_amdgcn_readlane(w, q);
                                const uint64_t qp = (uint64_t)qw | ((uint64_t)qw << 32);
                                for (uint32_t k = 8u * lane; k + 8u <= qM; k += 8u * kWave) lds_st64(qd + k, qp);
                            }
                        }
                        // (b) not overlapping, 65..160 bytes, four or more of them in the level: 32 bytes per step in the lane,
                        // the last step two-ended (fewer: the whole wave is quicker, (d))
                        const bool lngc = fits && !rle && off >= M && M <= 160u;
                        const bool lng = lngc && __builtin_popcountll(__ballot(lngc)) >= 4;
                        if (lng) {
                            uint32_t k = 0;
                            for (;;) {
                                const uint32_t kk = k + 32u <= M ? k : M - 32u;
                                uint64_t x0, x1, x2, x3;
                                lds_ld64x4(sa + kk, sa + kk + 8u, sa + kk + 16u, sa + kk + 24u, x0, x1, x2, x3);
                                lds_st64(da + kk, x0); lds_st64(da + kk + 8u, x1); lds_st64(da + kk + 16u, x2); lds_st64(da + kk + 24u, x3);
                                if (k + 32u >= M) break;
                                k += 32u;
                            }
                        }
                        // (c) overlapping, at most 64 bytes: doubling steps of its own
                        const bool dbl = fits && !rle && !lng && M <= 64u;
                        if (dbl) {
                            uint32_t pos = 0, av = off;
                            while (pos < M) { const uint32_t cc = av < M - pos ? av : M - pos; put_small_lds(da + pos, sa, cc); pos += cc; av += cc; }
                        }
                        // (d) the rest, one at a time by the whole wave
                        for (unsigned long long m = __ballot(nowS && !rle && !lng && !dbl); m; m &= m - 1ull) {
                            const uint32_t q = (uint32_t)__builtin_ctzll(m);
                            ring_match(__builtin_amdgcn_readlane(dy, q), __builtin_amdgcn_readlane(off, q), __builtin_amdgcn_readlane(M, q));
                        }
                        RT(tm_slow);
                    }
                }
                if (lane == 0u) flag_set(1, t + 1u);
            }
            if (gave_up) break;
        }
#ifdef LZF_SEG_TIME
        if (lane == 0u) flag_set(2, (uint32_t)(tm_wait >> 10));      // (to the stager, which writes the job's result: results[].reserved = this | total << 16, in units of 2^10 / 2^14 cycles)
        if (lane == 0u) { reinterpret_cast<uint16_t*>(&c.st[j].pad)[0] = (uint16_t)(n_rounds >> 4);
            c.st[j].pad2 = (unsigned long long)(uint16_t)(tm_wait >> 14) | ((unsigned long long)(uint16_t)(tm_setup >> 14) << 16) | ((unsigned long long)(uint16_t)(tm_asm >> 14) << 32) | ((unsigned long long)(uint16_t)(tm_slow >> 14) << 48); }
#endif
#undef RT
    } else {
        // ================================================= STAGER =================================================
        // History.  E0 = the biased end of the existing output, which is final (and visible) before the launch: nothing below it is ever
        // stored, so the flush pointer and the previous sequence's end start there, and the head of its granule stays what it is.
        // P = the prefix an offset can still reach (the records stage has the same rule), moved in from `prefix` by this wave.
        const uint32_t E0 = __builtin_amdgcn_readfirstlane((uint32_t)job.out_existing_len) + rb;
        const uint32_t P = __builtin_amdgcn_readfirstlane(job.out_existing_len >= kSegPrefixReach ? 0u : (uint32_t)job.prefix_len);
        cgu8* const pfx_end = as_global(job.prefix) + P;
        uint32_t fp = 0, fl = E0, safe = E0;             // filled up to (granule), flushed up to, own stores visible below
        uint32_t ticket = 0;                             // tickets published
        static_assert(NT <= 32, "the ends of the tickets in flight live in the lanes of one register");
        uint32_t endv = rb;                              // lane t % 64: biased end (rounded down to a granule) of published ticket t
        uint32_t flushed_t = 0;                          // tickets whose bytes are in HBM
        // (the split is lzf_ring_split(y0, y1, 0) of lzf_out_ring.h, the rule's one home, written out: calling it changed this kernel's code)
        auto flush_range = [&](uint32_t y0, uint32_t y1) {
            if (y1 <= y0) return;
            uint32_t nh = (16u - (y0 & 15u)) & 15u; if (nh > y1 - y0) nh = y1 - y0;
            if (nh) { if (lane < nh) outb[y0 + lane] = ring[(y0 + lane) & kMask]; y0 += nh; }
            const uint32_t ng = (y1 - y0) >> 4;
            for (uint32_t g = lane; g < ng; g += kWave)
                *reinterpret_cast<LZF_GLOBAL u32x4*>(outb + y0 + 16u * g) = *reinterpret_cast<const u32x4*>(&ring[(y0 + 16u * g) & kMask]);
            y0 += ng << 4;
            if (lane < y1 - y0) outb[y0 + lane] = ring[(y0 + lane) & kMask];
        };
        auto fill_to = [&](uint32_t g1) {
            for (uint32_t y = fp + 16u * lane; y < g1; y += 16u * kWave)
                *reinterpret_cast<u32x4*>(&ring[y & kMask]) = *reinterpret_cast<const LZF_GLOBAL u32x4*>(outb + y);
            if (g1 > fp) fp = g1;
        };
        // the granules behind the fill pointer, loaded one sub-batch early (the load's latency runs under the hand-over)
        u32x4 pfa = u32x4{0, 0, 0, 0}, pfb = u32x4{0, 0, 0, 0};
        uint32_t pf0 = 0, pf1 = 0;                       // [pf0, pf1) is held in registers
        const uint32_t fill_lim = (total + rb + 15u) & ~15u;
        auto prefetch_issue = [&](uint32_t need) {       // (the fill pointer stays within 3 KiB of what the sub-batch needed: the levels' fetch-ahead bound)
            pf0 = fp; pf1 = fp + 2048u < fill_lim ? fp + 2048u : fill_lim;
            if (pf1 <= pf0 || fp > need + 1024u) { pf0 = pf1 = 0; return; }
            const uint32_t ya = pf0 + 16u * lane, yb = ya + 1024u;
            if (ya < pf1) pfa = *reinterpret_cast<const LZF_GLOBAL u32x4*>(outb + ya);
            if (yb < pf1) pfb = *reinterpret_cast<const LZF_GLOBAL u32x4*>(outb + yb);
        };
        auto prefetch_commit = [&]() {
            if (pf1 > pf0 && pf0 == fp) {
                const uint32_t ya = pf0 + 16u * lane, yb = ya + 1024u;
                if (ya < pf1) *reinterpret_cast<u32x4*>(&ring[ya & kMask]) = pfa;
                if (yb < pf1) *reinterpret_cast<u32x4*>(&ring[yb & kMask]) = pfb;
                fp = pf1;
            }
            pf0 = pf1 = 0;
        };
        // write what the resolver has finished to HBM (whole granules), in ticket order
        auto flush_resolved = [&](uint32_t upto_t) {
            if (flushed_t < upto_t) {                    // (the ends only grow: everything up to the last resolved ticket's in one pass)
                const uint32_t e = __builtin_amdgcn_readlane(endv, (upto_t - 1u) & 63u);
                if (e > fl) { flush_range(fl, e); fl = e; }
                flushed_t = upto_t;
            }
        };
#ifdef LZF_SEG_TIME
        long long tm_swait = 0, tm_fill = 0, tm_old = 0;
        bool gave_up = false;
        auto wait_resolved = [&](uint32_t tt) { const long long t0 = clock64(); if (tt && !gave_up && !flag_wait_above(1, tt - 1u)) gave_up = true; tm_swait += clock64() - t0; };
#else
        bool gave_up = false;
        auto wait_resolved = [&](uint32_t tt) { if (tt && !gave_up && !flag_wait_above(1, tt - 1u)) gave_up = true; };
#endif
        u32x4 rA = u32x4{0, 0, 0, 0}, rB = u32x4{0, 0, 0, 0};
        if (n) { rA = recs[lane < n ? lane : n - 1u]; rB = recs[64u + lane < n ? 64u + lane : n - 1u]; }
        uint32_t prev_end = E0;                          // biased end of the previous sequence
        // The ring primed with the tail of the existing output before the first ticket, as after a class-8 sequence: everything a record
        // may have been classed "inside the ring" for — the records stage takes [fill pointer + fetch-ahead - R, ...) to be held, and the
        // fill pointer is never below E0's granule — so R - fetch-ahead bytes in front of it.  The last granule holds the block's first
        // bytes too: literals already in place, holes otherwise.
        if (E0 != rb) {
            const uint32_t keep = (uint32_t)R - (NS * kSpan + 64u);
            const uint32_t g1 = (E0 + 15u) & ~15u;
            fp = g1 > keep ? (g1 - keep) & ~15u : 0u;
            fill_to(g1);
        }
        // Sources older than the ring (class 7) of the NEXT batch's first sub-batch, loaded while this batch is staged: with the small
        // rings every sub-batch of a text block has some (offsets beyond ~20 KiB), and their round trip to HBM sat in the stager's
        // critical path — at four blocks per CU the stager spent 47 % of the block's time there and the resolver a third of its time
        // waiting for tickets (profiles/r05_seg_groups.txt, section 7).  Per lane: a match of 4..32 bytes whose source is below `safe`.
        uint64_t ov0 = 0, ov1 = 0, ov2 = 0, ov3 = 0;
        uint32_t o_for = kNone;                          // the batch (its first record) the registers were loaded for
        bool o_have = false;
        for (uint32_t i0 = 0; i0 < n && !gave_up; i0 += 64u) {
#ifdef LZF_ANALYSIS      // LZF_SEG_FORCE=stager: the stager of every odd job gives up at its third batch
            if (c.dbg_force == 1u && (j & 1u) && i0 >= 128u) { gave_up = true; if (lane == 0u) flag_set(3, 1u); break; }
#endif
            const uint32_t nb = n - i0 < 64u ? n - i0 : 64u;
            const u32x4 r = rA;
            const uint32_t M = lane < nb ? r[0] : 0u, dy = r[1], off = r[3];
            const uint32_t sub = lane < nb ? (r[2] & 0xFFu) : 0xFFu, cls = lane < nb ? r[2] >> 24 : 0u;
            const uint32_t nsub = __builtin_amdgcn_readlane(r[2] & 0xFFu, (nb - 1u) & 63u) + 1u;
            asm volatile("" ::: "memory");
            rA = rB;
            { const uint32_t ix = i0 + 128u + lane; rB = recs[ix < n ? ix : n - 1u]; }
            asm volatile("" ::: "memory");
            const uint32_t endy = dy + M;                // biased end of the sequence
            for (uint32_t s_i = 0; s_i < nsub && !gave_up; ++s_i) {
                const unsigned long long msub = __ballot(sub == s_i);
                if (!msub) { gave_up = true; if (lane == 0u) flag_set(3, 1u); break; }      // (records that do not number their sub-batches 0, 1, 2 ...: not ours)
                const uint32_t last = 63u - (uint32_t)__builtin_clzll(msub);
                const uint32_t oe = __builtin_amdgcn_readlane(endy, last);      // biased end of the sub-batch
                if (const unsigned long long mg8 = __ballot(sub == s_i && cls == 8u)) {
                    // ---- a sequence larger than a sub-batch: everything in front of it resolved and in HBM, then HBM -> HBM
                    // (it is alone in its sub-batch but for the empty sequences that pad a tile's last batch)
                    const uint32_t gl = (uint32_t)__builtin_ctzll(mg8);
                    const uint32_t g_dy = __builtin_amdgcn_readlane(dy, gl), g_M = __builtin_amdgcn_readlane(M, gl), g_off = __builtin_amdgcn_readlane(off, gl);
                    wait_resolved(ticket);
                    flush_resolved(ticket);
                    pf0 = pf1 = 0;                        // (what was loaded early may lie under the copy)
                    if (fp < ((prev_end + 15u) & ~15u)) fill_to((prev_end + 15u) & ~15u);
                    flush_range(fl, prev_end); if (prev_end > fl) fl = prev_end;
                    wave_store_fence();
                    if (g_M) {
                        // a source that starts in the prefix: its first bytes from there, byte by byte (any alignment); what is left is a
                        // match at the same offset whose source is out[0 ..]
                        uint32_t pos = 0;
                        if (P && g_off + rb > g_dy) {
                            const uint32_t pp = g_off + rb - g_dy;          // bytes of the source in front of out[0]
                            pos = pp < g_M ? pp : g_M;
                            for (uint32_t i = lane; i < pos; i += kWave) outb[g_dy + i] = pfx_end[(int32_t)i - (int32_t)pp];
                            wave_store_fence();
                        }
                        gu8* const src = outb + (g_dy - g_off + pos);       // (32-bit sum: out[0] where the source started in the prefix)
                        uint32_t av = g_off;
                        while (pos < g_M) {               // the same doubling as ring_match, through HBM
                            const uint32_t cc = av < g_M - pos ? av : g_M - pos;
                            wave_copy_long(outb + g_dy + pos, src, cc, lane);     // (cc <= the bytes between src and the destination: apart)
                            pos += cc; av += cc;
                            if (pos < g_M) wave_store_fence();
                        }
                        wave_store_fence();
                    }
                    // the ring's history is read back from HBM: [oe - (R - fetch-ahead), oe), granules
                    fl = oe; safe = oe;
                    {
                        const uint32_t keep = (uint32_t)R - (NS * kSpan + 128u);
                        const uint32_t g1 = (oe + 15u) & ~15u;
                        fp = g1 > keep ? (g1 - keep) & ~15u : 0u;
                        // (the last granule may hold bytes of the next sequence: they are in `out` already when literals, holes otherwise)
                        fill_to(g1);
                    }
                } else {
                    // ---- sub-batch: the ring filled, the sources older than the ring moved in
                    // Room: fewer than NT tickets unresolved, and the ring filled no further than two spans beyond the end of the oldest
                    // unresolved ticket r (with the 3 KiB the early loads may add: within the fetch-ahead the records stage assumed,
                    // oe_r + 3 spans + 64 — with three tickets in flight that held by itself, a sub-batch being at most a span).
                    uint32_t rs = 0;
                    {
                        const uint32_t need = (oe + 15u) & ~15u;
#ifdef LZF_SEG_TIME
                        const long long t0 = clock64();
#endif
                        // (wait_until's rule written out: as a call of it the kernel came out with two register pairs swapped, profiles/seg_split.txt)
                        for (uint32_t spin = 0; !gave_up; ++spin) {
                            rs = flag_get(1);
                            const uint32_t er = rs < ticket ? __builtin_amdgcn_readlane(endv, rs & 63u) : need;
                            if (ticket - rs < NT && need <= er + 2u * kSpan + 16u) break;
                            if ((spin & 63u) == 63u && (flag_get(3) != 0u || spin > (1u << 22))) { if (lane == 0u) flag_set(3, 1u); gave_up = true; break; }
                            __builtin_amdgcn_s_sleep(1);
                        }
#ifdef LZF_SEG_TIME
                        tm_swait += clock64() - t0;
#endif
                    }
#if defined(LZF_SEG_DBG_SKIP) && LZF_SEG_DBG_SKIP == 3      // analysis: a stager that moves no bytes (what the resolver costs on its own)
                    if (false)
#endif
                    flush_resolved(rs < ticket ? rs : ticket);
#if defined(LZF_SEG_DBG_SKIP) && LZF_SEG_DBG_SKIP == 3
                    fp = (oe + 15u) & ~15u;
#endif
#ifdef LZF_SEG_TIME
                    const long long tf0 = clock64();
#endif
                    prefetch_commit();
                    fill_to((oe + 15u) & ~15u);
#ifdef LZF_SEG_TIME
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    tm_fill += clock64() - tf0;
#endif
                    prefetch_issue((oe + 15u) & ~15u);
                    bool old = sub == s_i && cls == 7u;
#ifdef LZF_SEG_TIME
                    const long long to0 = clock64();
#endif
                    {   // the lanes whose bytes came early (two-ended pieces, as put_small_glb stores them)
                        const bool early = old && s_i == 0u && o_for == i0 && o_have;
                        if (__ballot(early)) {
                            if (early) {
                                const uint32_t d = ring_a + (dy & kMask);
                                if (M >= 8u) {
                                    lds_st64(d, ov0);
                                    if (M > 16u) { lds_st64(d + 8u, ov1); lds_st64(d + M - 16u, ov2); }
                                    lds_st64(d + M - 8u, ov3);
                                } else { lds_st32(d, (uint32_t)ov0); lds_st32(d + M - 4u, (uint32_t)ov3); }
                            }
                            old = old && !early;
                        }
                    }
                    if (__ballot(old)) {
                        // (a rare path: its operands pass through an empty asm statement, or its predicates are computed per batch)
                        uint32_t M_o = M, off_o = off, dy_o = dy;
                        asm volatile("" : "+v"(M_o), "+v"(off_o), "+v"(dy_o));
                        const uint32_t M = M_o, off = off_o, dy = dy_o;
                        const uint32_t span = M < off ? M : off;
                        const uint32_t sy = dy - off;
                        if (__ballot(old && sy + span > fl)) { wait_resolved(ticket); flush_resolved(ticket); }
                        if (__ballot(old && (sy + span > fl ? fl : sy + span) > safe)) { wave_store_fence(); safe = fl; }
                        const uint32_t di = dy & kMask;
                        const bool own = old && sy + span <= fl && M <= 64u && off >= M && di + M <= (uint32_t)R;
                        if (own) put_small_glb(ring_a + di, outb + sy, M);
                        for (unsigned long long m = __ballot(old && !own); m; m &= m - 1ull) {
                            const uint32_t q = (uint32_t)__builtin_ctzll(m);
                            const uint32_t qM = __builtin_amdgcn_readlane(M, q), qs = __builtin_amdgcn_readlane(sy, q), qd = __builtin_amdgcn_readlane(dy, q);
                            const uint32_t qo = __builtin_amdgcn_readlane(off, q);
                            // (all lanes, a byte each per step: the source lies in front of the destination, so no byte read here is one written here)
                            for (uint32_t i = lane; i < qM; i += kWave) {
                                const uint32_t y = qs + (qo < qM ? i % qo : i);
                                ring[(qd + i) & kMask] = y < fl ? (uint8_t)outb[y] : ring[y & kMask];
                            }
                        }
                    }
                    // sources in the prefix (class 13), which is final before the launch: straight into the ring, like the old sources above
                    if (P) {
                        const bool pin = sub == s_i && cls == 13u;
                        if (__ballot(pin)) {
                            uint32_t M_p = M, off_p = off, dy_p = dy;
                            asm volatile("" : "+v"(M_p), "+v"(off_p), "+v"(dy_p));
                            const uint32_t M = M_p, pp = off_p + rb - dy_p, di = dy_p & kMask;      // pp: the source starts this many bytes in front of out[0] (>= M)
                            const bool own = pin && M <= 64u && di + M <= (uint32_t)R;
                            if (own) put_small_glb(ring_a + di, pfx_end - pp, M);
                            for (unsigned long long m = __ballot(pin && !own); m; m &= m - 1ull) {
                                const uint32_t q = (uint32_t)__builtin_ctzll(m);
                                const uint32_t qM = __builtin_amdgcn_readlane(M, q), qp = __builtin_amdgcn_readlane(pp, q), qd = __builtin_amdgcn_readlane(dy_p, q);
                                for (uint32_t i = lane; i < qM; i += kWave) ring[(qd + i) & kMask] = pfx_end[(int32_t)i - (int32_t)qp];
                            }
                        }
                    }
#ifdef LZF_SEG_TIME
                    { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); tm_old += clock64() - to0; }
#endif
                }
                const uint32_t eg = oe & ~15u;
                if (lane == (ticket & 63u)) endv = eg;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the ring and the slot written; loads and stores to HBM stay in flight
                ++ticket;
                if (lane == 0u) flag_set(0, ticket);
                prev_end = oe;
            }
            // ---- the next batch's old sources, early (its records are in rA)
            o_for = kNone; o_have = false;
            if (i0 + 64u < n && !gave_up) {
                const u32x4 q = rA;
                const uint32_t nbn = n - (i0 + 64u) < 64u ? n - (i0 + 64u) : 64u;
                const uint32_t Mn = q[0], dyn = q[1], offn = q[3];
                const uint32_t syn = dyn - offn, din = dyn & kMask;
                o_have = lane < nbn && (q[2] >> 24) == 7u && (q[2] & 0xFFu) == 0u && Mn >= 4u && Mn <= 32u && offn >= Mn &&
                         din + Mn <= (uint32_t)R && syn + Mn <= safe && syn + Mn <= fl;
                o_for = i0 + 64u;
                if (o_have) {
                    cgu8* g = outb + syn;
                    if (Mn >= 8u) { ov0 = ld8(g); ov3 = ld8(g + Mn - 8u); if (Mn > 16u) { ov1 = ld8(g + 8u); ov2 = ld8(g + Mn - 16u); } }
                    else { ov0 = ld4(g); ov3 = ld4(g + Mn - 4u); }
                }
            }
        }
        wait_resolved(ticket);
        // A pair that gave up — this wave's bounded wait, the resolver's (ctl[3]), records this stage does not handle — leaves the
        // job alone: no result, done stays 0, and the pair kernel launched behind this one decodes the block from its first byte.
        if (gave_up || flag_get(3) != 0u) return;
#if !(defined(LZF_SEG_DBG_SKIP) && LZF_SEG_DBG_SKIP == 3)
        flush_resolved(ticket);
        flush_range(fl, total + rb);
#endif
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

#ifdef LZF_SEG_TIME
        if (lane == 0u) reinterpret_cast<uint16_t*>(&c.st[j].pad)[1] = (uint16_t)(tm_swait >> 14);
#endif
        if (lane == 0u) {
            c.results[j].out_len = total;
            c.results[j].status = LZF_OK;
#ifdef LZF_SEG_TIME
            // resolver's wait for tickets | stager: fills | stager: sources older than the ring | total — a byte each, in 2^17 cycles
            { auto b8 = [](long long v) -> uint32_t { const long long x = v >> 17; return x > 255 ? 255u : (uint32_t)x; };
              c.results[j].reserved = b8((long long)flag_get(2) << 10) | (b8(c.dbg_force == 8u ? tm_swait : tm_fill) << 8) | (b8(tm_old) << 16) | (b8(clock64() - t_start) << 24); }
#else
            c.results[j].reserved = (uint32_t)((clock64() - t_start) >> 10);
#endif
            c.st[j].done = 1u;
        }
    }
}
template __global__ void lzf_seg_resolve_pair_kernel<32768>(seg_ctx);
template __global__ void lzf_seg_resolve_pair_kernel<65536>(seg_ctx);
template __global__ void lzf_seg_resolve_pair_kernel<131072>(seg_ctx);

}  // namespace lzf
