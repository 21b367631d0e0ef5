// lz4_decompress_batch_phase.inc — the COPY stage shared by the batched decompress kernels (textual include
// inside the kernel's chunk loop; see lz4_decompress_batched.hip for the description of the stage).
// The stage's interface (checked below: a kernel that forgets one fails at the include):
//   objects    lane; jv (DecodeJob: the job view); rg (OutRing<RING>: the output ring, its fill / flush); sb (StagedBytes: the staged
//              window, rdb / rd4 — the parse and feed stages leave it); kSpanMax, kNearHist (a batch's output bytes, the intact history)
//   carried    o, safe, status of the kernel's loop; cstart and Tc (tokens listed) of this chunk
//   the token list, as macros the kernel defines around the include:
//     LZF_TOKEN_AT(i)     chunk offset of listed token i
//     LZF_TOKEN_WORD(i)   optional: entry i with the lengths the parser decoded (offset | L << 16 | (M - 4) << 24; the pair kernel)
//     LZF_FED_DECODE      the bitmap-fed kernel, instead of the two above: toks (window offsets, not yet verified) and the carried expect
//                         (where the chain's next token starts), fed_carry and bail; the set-up then decodes each token once and checks the
//                         chain's links before the batch writes anything (a broken link or UnexpectedEnd: bail, the loop ends with `expect` on
//                         the failing batch's first token), and a short last batch of the list may be left for the next window.
//                         Also carried: pend — out[pend, o) is still only in the ring (the DEFERRED FLUSH, below and at PHASE(3)); pend >= o:
//                         nothing is pending.  The kernel drains it wherever its loop ends.
//     LZF_FAR_LATE        optional: the far matches' loads behind the literal copy instead of in front of it
            LZF_STAGE_NEEDS(jv, DecodeJob); LZF_STAGE_NEEDS(rg.kRing, uint32_t); LZF_STAGE_NEEDS(sb.kCB, uint32_t); LZF_STAGE_NEEDS(lane, uint32_t);
            LZF_STAGE_NEEDS(o, uint32_t); LZF_STAGE_NEEDS(safe, uint32_t); LZF_STAGE_NEEDS(status, int); LZF_STAGE_NEEDS(cstart, uint32_t); LZF_STAGE_NEEDS(Tc, uint32_t);
            static_assert(kSpanMax + kNearHist == rg.kRing, "a batch's span and the intact history share the ring");
#if defined(LZF_FED_DECODE)
            LZF_STAGE_NEEDS(expect, uint32_t); LZF_STAGE_NEEDS(fed_carry, uint32_t); LZF_STAGE_NEEDS(bail, bool); LZF_STAGE_NEEDS(toks[0], uint16_t); LZF_STAGE_NEEDS(pend, uint32_t);
            // The deferred flush.  A batch does not write itself to `out` at its end: it leaves its bytes pending in the ring, and the NEXT batch
            // flushes them behind its own far phase — once its far loads have been waited for and have landed in the ring, in front of its match
            // rounds.  What it buys is the whole-line flush of the next point: with a range carried from batch to batch, the ragged ends need not
            // be written as bytes.  That took 1.2 ms of 87 off the headline call; the deferral by itself — the next wait for a load no longer waiting
            // for this flush's write acknowledgements, gfx950 counting both in one vmcnt — measured 0.2 - 0.4 %, inside the noise
            // (profiles/fed_deferred_flush.txt).
            //  - Whole 16-byte lines only (OutRing::flush_lines): the flush stops at the last 16-byte address at or below ob0 and leaves the ragged
            //    end, up to 15 bytes, pending with this batch's bytes.  A line of `out` is written once and whole, and the common flush has no
            //    head or tail bytes: only the first one behind a hand-over, a solo sequence or the job's start has a head.  So out[pend, o) is
            //    pending, and at a batch's start pend is at most 15 below the start of the batch before.  The drains write bytes, as every flush did.
            //  - The ring allows it: the batch before and the ragged end in front of it are at most kSpanMax + 15 < kNearHist bytes below ob0,
            //    inside the history this batch keeps intact — it writes the ring only at [ob0, ob0 + kSpanMax).
            //  - Nothing reads pending bytes from `out`: near_lo = ob0 - kNearHist < pend; a far source ends at or below near_lo, and the slow loop
            //    and the cooperative far loop read jv.out[s] only for s < near_lo.
            //  - `safe` (out[0, safe) is visible to this wave's loads) moves only where a full wait happened, and then to `pend`: what has
            //    been issued.  Every `need` the fence test looks at is <= near_lo < pend, so one fence always satisfies it.  Not to ob0: the batch
            //    before has not been issued yet, and a later far source may lie in it.  The price is known: a fence in front of 34 % of the batches
            //    of the Silesia stand-in instead of 24 % (72 194 against 52 391 per copy), inside the gain measured.
            //  - The solo path drains first (it writes `out` directly and re-fills the ring from it).  Every exit of the batch loop — an error status,
            //    a bail (both raised before the batch wrote anything: o is still ob0), a carried batch, the window's end — leaves the range pending for
            //    the kernel, which drains it when its window loop ends (parked, finished, failed, bailed) and carries it across windows and across
            //    the walk-mode retry of a window otherwise: the retry runs no batch before the one that flushes it.
            static_assert(kSpanMax + 16u <= kNearHist, "the batch before and the ragged end before it lie inside the history this batch keeps intact, above every far source");
#elif !defined(LZF_TOKEN_AT)
#error "lz4_decompress_batch_phase.inc: define LZF_TOKEN_AT(i) (or LZF_FED_DECODE) around the include"
#endif
            // =====================================================================
            // B. batches of up to 64 sequences: lane j owns token tidx + j
            // =====================================================================
            uint32_t tidx = 0;
            if (LZF_DBG_SKIP & 1) { tidx = Tc; o += Tc; }      // (LZF_FED_DECODE: no decode either, the chain stops after one window)
#if defined(LZF_FED_DECODE)
            if (LZF_DBG_SKIP & 1) { expect = jv.len; pend = o; }
#endif
            while (tidx < Tc && status == LZF_OK) {
#if defined(LZF_FED_DECODE)
                // a short batch at the end of the window's list waits for the next window, which starts on its first token and fills it
                // up (lzf_fed_window.h); `expect` stands on that token.  Never the window's first batch: every window runs a batch.
                if (lzf_fedw_carry(Tc, tidx, cstart + kRound, jv.len, fed_carry)) break;
#endif
                PHASE(0);
#if defined(LZF_DBG_ROUNDS) && defined(LZF_DBG_ROUNDS_HERE)
                ++dbg_batches;
#endif
#if defined(LZF_FED_DECODE) && defined(LZF_DBG_FED_COUNT)
                ++dbg_fed[0];
#endif
                const uint32_t ob0 = o;
                const uint32_t nb_try = Tc - tidx < kWave ? Tc - tidx : kWave;
#if defined(LZF_FED_DECODE)
                // the lanes with a token, as a mask built on the scalar side (nb_try >= 1): the set-up's ballots are compare masks ANDed
                // with it, its selects take it as their condition — no lane compare feeds a scalar instruction
                const unsigned long long act0 = lanes_below(nb_try);
#else
                const bool act0 = lane < nb_try;
#endif
                // ---- re-read the token (decompress.rs:61-71), per lane
                uint32_t L = 0, M = 0, src = 0;
                bool has = false;
#if defined(LZF_FED_DECODE)
                // Each token is decoded here and nowhere else.  The common token (no 0xFF length byte, offset and match-length byte staged)
                // without branches; the rest through the serial routine.  Lanes past nb_try decode lane 0's token again (masked off).
                uint32_t next;                                     // where the token's successor starts (len: the last literals)
                const uint32_t pos = toks[tidx + lane_sel(act0, lane, 0u)];
                const uint32_t tp = cstart + pos;
                uint32_t w;                                        // token + first literal-length byte (pos < kRound: staged)
                asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(sb.lds + pos) : "memory");
                const uint32_t l0 = (w >> 4) & 15u, b1 = (w >> 8) & 255u, m0 = w & 15u;
                const bool lx = l0 == 15u;
                const uint32_t lext = lx ? b1 : 0u;
                L = l0 + lext;
                src = tp + (lx ? 2u : 1u);
                const uint32_t q = src + L;                        // the offset (a missing extension byte reads as 0: q > len then)
                has = q + 2u <= jv.len;                               // :70 read_u16 fails: last literals
                const bool mx = has && m0 == 15u;
                // The offset and the match-length byte behind it in ONE unaligned read (off | m1 << 16), where all four bytes are staged
                // (rq <= pos + 2 + 270 < 2^16: no wrap).  A lane whose four bytes are not reads position 0 and ignores it: its match length,
                // if it has an extension, comes from the serial routine (mext = 255 sends it there — also the lane whose byte at q + 2 is
                // the last staged one, which read it by itself before), its offset from the rare path behind the scan.  `off` stays
                // in its register across the scan; a lane that ends up without a match or outside the batch never looks at it.
                uint32_t rq = q - cstart;
                const bool fit4 = rq + 4u <= sb.kCB;
                const uint32_t ow = lds_ld32(sb.lds + (fit4 ? rq : 0u));
                uint32_t off = ow & 0xFFFFu;
                const uint32_t mext = mx ? (fit4 ? (ow >> 16) & 255u : 255u) : 0u;
                M = has ? m0 + 4u + mext : 0u;                     // (m0 == 15: 19 + m1)
                // `need`: how far the token needs the input to reach.  :67 read_exact wants q <= len; with a match, has says q + 2 <= len
                // already, and read_lsic one byte more when m0 == 15.  need > len: UnexpectedEnd (one compare, below)
                uint32_t need = has ? q + (mx ? 3u : 2u) : q;
                next = has ? need : jv.len;
                const bool general = (lext > mext ? lext : mext) == 255u;       // (lx && b1 == 255) || (mx && (m1 not staged with the offset || m1 == 255))
                {                                                  // (a lane past nb_try holds lane 0's token: general only if lane 0 is.  The branch around
                    if (general) {                                 //  a per-lane `if` is the wave-uniform test already)  decompress.rs:61-71 without the copies, byte by byte
                        uint32_t p = tp + 1u, b = 0;
                        bool bad = false;
                        L = l0; M = 0; has = false; next = jv.len;
                        if (lx) {
                            do { if (p >= jv.len) { bad = true; break; } b = sb.rdb(p); ++p; L += b; if (L > kMaxPosB) L = kMaxPosB; } while (b == 255u);
                        }
                        src = p;
                        if (!bad && jv.len - p < L) bad = true;       // :67 read_exact
                        p += L;
                        if (!bad && jv.len - p >= 2u) {
                            has = true; p += 2u; M = m0;
                            if (m0 == 15u) {
                                do { if (p >= jv.len) { bad = true; break; } b = sb.rdb(p); ++p; M += b; if (M > kMaxPosB) M = kMaxPosB; } while (b == 255u);
                            }
                            M += 4u; next = p;
                        }
                        need = bad ? 0xFFFFFFFFu : 0u;
                        rq = sb.kCB;                               // (the offset is not where the read above looked: the rare path reads it)
                    }
                }
                // the chain: lane 0's token is where the chain goes on, every other lane's token where the lane before it ends (the
                // batch's last token is checked against its successor as lane 0 of the next batch or round)
                if ((__builtin_amdgcn_uicmp(need, jv.len, 34 /* > */) | __builtin_amdgcn_uicmp(tp, wave_prev(next, expect), 33 /* != */)) & act0) { bail = true; break; }
#else
#ifdef LZF_TOKEN_WORD
                // the parser already decoded the lengths of plain tokens (entry = offset | L << 16 | (M - 4) << 24)
                bool decode = act0;
                if (act0) {
                    const uint32_t tw = LZF_TOKEN_WORD(tidx + lane);
                    const uint32_t lc = (tw >> 16) & 255u, mc = tw >> 24;
                    if (lc != 255u && mc != 255u) {
                        decode = false;
                        L = lc; src = cstart + (tw & 0xFFFFu) + (lc >= 15u ? 2u : 1u);
                        if (mc != 254u) { has = true; M = mc + 4u; }
                    }
                }
                if (decode) {
#else
                if (act0) {
#endif
                    const uint32_t tp = cstart + LZF_TOKEN_AT(tidx + lane);
                    const uint32_t w = sb.rd4(tp);                      // token + first literal-length extension byte
                    const uint32_t tok = w & 255u;
                    uint32_t q = tp + 1u;
                    L = tok >> 4;
                    if (L == 15u) {
                        uint32_t b = (w >> 8) & 255u; ++q;
                        L += b;
                        while (b == 255u) { b = sb.rdb(q); ++q; L += b; if (L > kMaxPosB) L = kMaxPosB; }
                    }
                    src = q; q += L;
                    if (jv.len - q >= 2u) {
                        has = true; q += 2u;
                        M = tok & 15u;
                        if (M == 15u) { for (;;) { const uint32_t b = sb.rdb(q); ++q; M += b; if (M > kMaxPosB) M = kMaxPosB; if (b != 255u) break; } }
                        M += 4u;
                    }
                }
#endif
                // ---- output positions
                uint32_t tot = L + M; if (tot > kTotClamp || tot < L) tot = kTotClamp;
#if defined(LZF_FED_DECODE)
                // (first lane over the span, nb and nb - 1 by scalar instructions.  No `& act0`: the lanes past nb_try add 0, so they
                //  repeat lane nb_try - 1's sum, and min(., nb_try) gives the same lane with or without them)
                const uint32_t tot0 = lane_sel(act0, tot, 0u);
                const uint32_t incl = wave_scan_add(tot0);
                const uint32_t lo = ob0 + (incl - tot0);
                const uint32_t mo = lo + L;
                const uint32_t nb = first_lane_min(__builtin_amdgcn_uicmp(incl, kSpanMax, 34 /* > */), nb_try);       // sequences in this batch
#else
                const uint32_t incl = wave_scan_add(act0 ? tot : 0u);
                const uint32_t lo = ob0 + (incl - (act0 ? tot : 0u));
                const uint32_t mo = lo + L;
                const uint32_t c = first_lane(__ballot(act0 && incl > kSpanMax));
                const uint32_t nb = c < nb_try ? c : nb_try;       // sequences in this batch
#endif

                if (nb == 0u) {
                    // =============================================================
                    // C. solo sequence (larger than a batch): HBM -> HBM, then re-fill the ring
                    // =============================================================
#if defined(LZF_FED_DECODE)
                    expect = __builtin_amdgcn_readlane(next, 0);
                    // (drain: from here on `out` is written directly, and the ring re-filled from it.  No range until the sequence is through:
                    //  what an error exit below leaves in [pend, o) is in `out` already, not in the ring)
                    if (!(LZF_DBG_SKIP & 16)) rg.flush(pend, o);
                    pend = 0xFFFFFFFFu;
#endif
                    const uint32_t s_L = __builtin_amdgcn_readlane(L, 0);
                    const uint32_t s_M = __builtin_amdgcn_readlane(M, 0);
                    const uint32_t s_src = __builtin_amdgcn_readlane(src, 0);
                    const bool s_has = __builtin_amdgcn_readlane((uint32_t)has, 0) != 0u;
                    if (jv.cap - o < s_L) { status = LZF_OUT_CAPACITY; break; }
                    if (s_has && (uint64_t)o + s_L + s_M > jv.limit) { status = LZF_MEMORY_LIMIT_EXCEEDED; break; }   // :72-74
                    const uint32_t o_before = o;
                    wave_copy(jv.out + o, jv.in + s_src, s_L, lane);                           // literals :65-67
                    o += s_L;
                    if (s_has) {
                        const uint32_t offset = (uint32_t)jv.in[s_src + s_L] | ((uint32_t)jv.in[s_src + s_L + 1u] << 8);
                        uint32_t mlen = s_M;
                        if (offset == 0u) { status = LZF_ZERO_DEDUP_OFFSET; break; }      // :83
                        bool done = false;
                        if (offset > o) {                                                 // :84-99
                            const uint32_t need = offset - o;
                            if (need > jv.plen) { status = LZF_INVALID_DEDUP_OFFSET; break; }
                            const uint32_t nn = need < mlen ? need : mlen;
                            if (jv.cap - o < nn) { status = LZF_OUT_CAPACITY; break; }
                            wave_copy(jv.out + o, jv.prefix + (jv.plen - need), nn, lane);
                            o += nn; mlen -= nn;
                            done = mlen == 0u;
                        }
                        if (!done) {
                            if (jv.cap - o < mlen) { status = LZF_OUT_CAPACITY; break; }
                            const uint32_t src0 = o - offset;
                            const uint32_t span = mlen < offset ? mlen : offset;
                            if (src0 + span > safe) { wave_store_fence(); safe = o; }
                            cgu8* hist = jv.out + src0;
                            gu8* dst = jv.out + o;
                            if (mlen <= offset) {
                                wave_copy(dst, hist, mlen, lane);
                            } else if (offset == 1u) {
                                const uint32_t b = hist[0];
                                const uint32_t b4 = b * 0x01010101u;
                                const u32x4 v = {b4, b4, b4, b4};
                                const uint32_t bulk = mlen & ~15u;
                                for (uint32_t i = lane * 16u; i < bulk; i += kWave * 16u) st16(dst + i, v);
                                if (lane < mlen - bulk) dst[bulk + lane] = (uint8_t)b;
                            } else {
                                uint32_t r = lane % offset;
                                const uint32_t adv = kWave % offset;
                                for (uint32_t i = lane; i < mlen; i += kWave) {
                                    dst[i] = hist[r];
                                    r += adv; if (r >= offset) r -= offset;
                                }
                            }
                            o += mlen;
                        }
                    }
                    // ring <- the tail of what was just written
                    wave_store_fence(); safe = o;
                    rg.fill((o - o_before > rg.kRing) ? o - rg.kRing : o_before, o);
#if defined(LZF_FED_DECODE)
                    pend = o;
#endif
                    tidx += 1u;
                    continue;
                }

#if defined(LZF_FED_DECODE)
                // the batch's lanes as a scalar mask (nb >= 1 here); a lane of the batch has a match exactly when its M (>= 4) is not 0
                expect = __builtin_amdgcn_readlane(next, nb - 1u);
                const unsigned long long act_m = lanes_below(nb);
                L = lane_sel(act_m, L, 0u); M = lane_sel(act_m, M, 0u);
                has = M != 0u;
                const unsigned long long has_m = __builtin_amdgcn_uicmp(M, 0u, 33 /* != */);
                const bool act = lane < nb;                        // (only the exact error codes below look at it)
                // the rare path of the offset: a lane with a match whose four bytes were not all staged, or whose token the serial routine decoded
                if (__builtin_amdgcn_uicmp(rq, sb.kCB - 4u, 34 /* > */) & has_m) {
                    asm volatile("");      // (keeps hipcc from folding this uniform test into the lanes' own, which puts an EXEC region and its bookkeeping on the common path)
                    if (has && rq > sb.kCB - 4u) {
                        if (!sb.kStage) off = ld2(jv.in + src + L);
                        else if (src + L - cstart + 2u <= sb.kCB) off = lds_ld16(sb.lds + (src + L - cstart));      // (one unaligned 2-byte LDS read)
                        else off = sb.rdb(src + L) | (sb.rdb(src + L + 1u) << 8);
                    }
                }
#else
                const bool act = lane < nb;
                has = has && act;
                if (!act) { L = 0; M = 0; }
                uint32_t off = 0;
                if (has) {
                    if (!sb.kStage) off = ld2(jv.in + src + L);
                    else if (src + L - cstart + 2u <= sb.kCB) off = lds_ld16(sb.lds + (src + L - cstart));      // (one unaligned 2-byte LDS read)
                    else off = sb.rdb(src + L) | (sb.rdb(src + L + 1u) << 8);
                }
#endif
#if defined(LZF_FED_DECODE)
                // ---- errors.  What a valid batch needs is two tests; the exact codes are worked out only when one of them flags something.
                //  - Uniform, in scalar registers: E = ob0 + incl[nb - 1], where the batch ends (the flush's new `o`).  For a lane j < nb,
                //    incl[j] <= kSpanMax (nb stops in front of the first lane over it), so tot[j] <= incl[j] < kTotClamp was not clamped
                //    and did not wrap: tot = L + M exactly, and lo + L + M = ob0 + incl[j] <= E.  ob0 <= cap <= kMaxPosB (every earlier
                //    batch passed these tests; out_existing_len <= out_cap), so E <= kMaxPosB + kSpanMax < 2^32.  With E <= cap and
                //    E <= limit neither capacity test nor the limit test can fail in any lane.  E over a bound is NOT an error by
                //    itself: a valid job may end above `limit` through its last, literals-only token; the codes below decide.
                //  - Per lane, both offset errors in one compare.  It only has to be right when the uniform test passed (otherwise the codes
                //    run anyway): then mo <= E <= cap <= kMaxPosB and plen < kMaxPosB (the contract), so mo + plen < 2^32 does not wrap.
                //    off <= 0xFFFF; off == 0 gives off - 1 = 2^32 - 1 >= anything, and for off >= 1, off - 1 >= mo + plen is
                //    off > mo + plen, that is off > mo && off - mo > plen.
                static_assert(kSpanMax < kTotClamp && (uint64_t)kMaxPosB * 2u < (1ull << 32), "the bounds argument above");
                const uint32_t lim32 = jv.limit > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)jv.limit;
                const uint32_t fit = jv.cap < lim32 ? jv.cap : lim32;
                const uint32_t E = ob0 + __builtin_amdgcn_readlane(incl, nb - 1u);
                // (the uniform test as a compare mask too: as `E > fit ||` hipcc turns both tests into booleans and back, seven scalar instructions)
                const unsigned long long flagged = (__builtin_amdgcn_uicmp(off - 1u, mo + jv.plen, 35 /* >= */) & has_m) | __builtin_amdgcn_uicmp(E, fit, 34 /* > */);
                if (flagged) {
#endif
                // ---- errors, first sequence in stream order wins; inside a sequence the reference's order  (the pair and batched kernels
                // work the codes out for every batch: the two tests in front cost them scalar registers, two of them spilled in the batched kernel)
                int code = LZF_OK;
                if (act) {
                    if (lo > jv.cap || jv.cap - lo < L) code = LZF_OUT_CAPACITY;                        // our buffer (literals)
                    else if (has && (uint64_t)mo + M > jv.limit) code = LZF_MEMORY_LIMIT_EXCEEDED;    // :72-74
                    else if (has && off == 0u) code = LZF_ZERO_DEDUP_OFFSET;                       // :83
                    else if (has && off > mo && off - mo > jv.plen) code = LZF_INVALID_DEDUP_OFFSET;  // :84-89
                    else if (has && jv.cap - mo < M) code = LZF_OUT_CAPACITY;                         // our buffer (match)
                }
                const uint32_t e = first_lane(__ballot(code != LZF_OK));
                if (e < 64u) { status = __builtin_amdgcn_readlane(code, e); break; }
#if defined(LZF_FED_DECODE)
                }
#endif
                PHASE(1);

                // ---- matches (copy_overlapping, decompress.rs:80-138)
                const uint32_t near_lo = ob0 > kNearHist ? ob0 - kNearHist : 0u;
                const uint32_t span = M < off ? M : off;                  // distinct source bytes
                const bool from_prefix = has && off > mo;
                const uint32_t s0 = mo - off;                             // valid when !from_prefix
                const bool is_near = has && !from_prefix && s0 >= near_lo;
                const bool is_far = has && !from_prefix && s0 + span <= near_lo;
                const bool is_slow = has && !is_near && !is_far;          // prefix or straddling
                const uint32_t mi = RIDX(mo);
                const bool mwrap = mi + M > rg.kRing;               // destination wraps around the ring
                // HBM visibility of what far / slow lanes read back
                {
                    uint32_t need = 0;
                    if (is_far) need = s0 + M;
                    if (is_slow && !from_prefix) need = near_lo;
                    if (is_slow && from_prefix && M > off - mo) need = near_lo;
                    if (need > ob0) need = ob0;
#if defined(LZF_FED_DECODE)
                    // (the batch before is not in `out` yet: the wait covers what has been issued, out[0, pend) — and need <= near_lo <= pend)
                    if (__ballot(need > safe)) {
#if defined(LZF_DBG_FED_COUNT)
                        ++dbg_fed[5];
#endif
                        wave_store_fence(); safe = pend;
                    }
#else
                    if (__ballot(need > safe)) { wave_store_fence(); safe = ob0; }
#endif
                }
                // far (never overlapping: offset > ring history > length): HBM -> ring.  The loads of the short
                // ones are issued here and land while the literals are being copied; the stores follow below.
                const bool far_own = !(LZF_DBG_SKIP & 4) && is_far && M <= kFarShort && !mwrap;
                uint64_t fv0 = 0, fv1 = 0, fv2 = 0, fv3 = 0;
#ifndef LZF_FAR_LATE
                if (far_own) {
                    cgu8* g = jv.out + s0;
                    if (M >= 8u) {
                        fv0 = ld8(g); fv3 = ld8(g + M - 8u);
                        if (M > 16u) { fv1 = ld8(g + 8u); fv2 = ld8(g + M - 16u); }
                    } else {
                        fv0 = ld4(g); fv3 = ld4(g + M - 4u);
                    }
                }
#endif
                // ---- literals -> ring (decompress.rs:65-67)
                if (!(LZF_DBG_SKIP & 8) && __ballot(L > 0u)) {
                    const uint32_t n1 = L < kShort ? L : kShort;            // the lane's own share
                    const uint32_t ri = RIDX(lo);
                    if (n1 > 0u) {
                        if (ri + n1 > rg.kRing) {                     // wraps around the ring: bytes
                            for (uint32_t t = 0; t < n1; ++t) rg.ring[RIDX(lo + t)] = (uint8_t)sb.rdb(src + t);
                        } else if (sb.kStage && src - cstart + n1 <= sb.kCB) {
                            put_small_lds(rg.lds + ri, sb.lds + (src - cstart), n1);
                        } else {
                            put_small_glb(rg.lds + ri, jv.in + src, n1);
                        }
                    }
                    for (unsigned long long m = __ballot(L > kShort); m; m &= m - 1ull) {      // long runs: all lanes
                        const uint32_t j = (uint32_t)__builtin_ctzll(m);
                        const uint32_t jl = __builtin_amdgcn_readlane(L, j);
                        const uint32_t js = __builtin_amdgcn_readlane(src, j);
                        const uint32_t jo = __builtin_amdgcn_readlane(lo, j);
                        for (uint32_t i = kShort + lane; i < jl; i += 4u * kWave) {
                            const uint32_t i1 = i + kWave, i2 = i + 2u * kWave, i3 = i + 3u * kWave;
                            const uint8_t b0 = jv.in[js + i];
                            const uint8_t b1 = i1 < jl ? jv.in[js + i1] : (uint8_t)0;
                            const uint8_t b2 = i2 < jl ? jv.in[js + i2] : (uint8_t)0;
                            const uint8_t b3 = i3 < jl ? jv.in[js + i3] : (uint8_t)0;
                            rg.ring[RIDX(jo + i)] = b0;
                            if (i1 < jl) rg.ring[RIDX(jo + i1)] = b1;
                            if (i2 < jl) rg.ring[RIDX(jo + i2)] = b2;
                            if (i3 < jl) rg.ring[RIDX(jo + i3)] = b3;
                        }
                    }
                }
                PHASE(2);

#ifdef LZF_FAR_LATE      // (the loads here instead of in front of the literals: eight registers fewer across the literal copy)
                if (far_own) {
                    cgu8* g = jv.out + s0;
                    if (M >= 8u) {
                        fv0 = ld8(g); fv3 = ld8(g + M - 8u);
                        if (M > 16u) { fv1 = ld8(g + 8u); fv2 = ld8(g + M - 16u); }
                    } else {
                        fv0 = ld4(g); fv3 = ld4(g + M - 4u);
                    }
                }
#endif
                if (far_own) {
                    const uint32_t dsta = rg.lds + mi;
                    if (M >= 8u) {
                        lds_st64(dsta, fv0);
                        if (M > 16u) { lds_st64(dsta + 8u, fv1); lds_st64(dsta + M - 16u, fv2); }
                        lds_st64(dsta + M - 8u, fv3);
                    } else {
                        lds_st32(dsta, (uint32_t)fv0); lds_st32(dsta + M - 4u, (uint32_t)fv3);
                    }
                }
                if (!(LZF_DBG_SKIP & 4) && __ballot(is_far && !far_own)) {
                    if (is_far && M <= kShort && mwrap) { for (uint32_t t = 0; t < M; ++t) rg.ring[RIDX(mo + t)] = jv.out[s0 + t]; }
                    if (is_far && M > kFarShort && M <= kShort && !mwrap) put_small_glb(rg.lds + mi, jv.out + s0, M);   // 33..64 bytes: own loads now
                    for (unsigned long long m = __ballot(is_far && M > kShort); m; m &= m - 1ull) {
                        const uint32_t j = (uint32_t)__builtin_ctzll(m);
                        const uint32_t jm = __builtin_amdgcn_readlane(M, j);
                        const uint32_t js = __builtin_amdgcn_readlane(s0, j);
                        const uint32_t jo = __builtin_amdgcn_readlane(mo, j);
                        for (uint32_t i = lane; i < jm; i += 4u * kWave) {
                            const uint32_t i1 = i + kWave, i2 = i + 2u * kWave, i3 = i + 3u * kWave;
                            const uint8_t b0 = jv.out[js + i];
                            const uint8_t b1 = i1 < jm ? jv.out[js + i1] : (uint8_t)0;
                            const uint8_t b2 = i2 < jm ? jv.out[js + i2] : (uint8_t)0;
                            const uint8_t b3 = i3 < jm ? jv.out[js + i3] : (uint8_t)0;
                            rg.ring[RIDX(jo + i)] = b0;
                            if (i1 < jm) rg.ring[RIDX(jo + i1)] = b1;
                            if (i2 < jm) rg.ring[RIDX(jo + i2)] = b2;
                            if (i3 < jm) rg.ring[RIDX(jo + i3)] = b3;
                        }
                    }
                }
                PHASE(3);
#if defined(LZF_FED_DECODE)
                // ---- the batch before: ring -> HBM (pend <= ob0; an empty range after a solo sequence or a hand-over)
                // (The wait first: every load of this batch has been consumed by now, or was never issued — but hipcc's wait insertion carries the far
                //  loads as pending past the EXEC branch around their LDS stores, and then puts a vmcnt(0) behind the flush where their registers are
                //  used again: a wait for the stores' acknowledgement.  Here it waits for nothing, and nothing is pending behind it.)
                __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0), the other counters left alone
                if (LZF_DBG_SKIP & 128) { rg.flush_dry(pend, ob0); pend = ob0; }      // (analysis: the ring reads and addresses without the stores;
                else if (LZF_DBG_SKIP & 16) pend = ob0;                               //  no flush at all)
                else pend = rg.flush_lines(pend, ob0);
#endif
                unsigned long long unresolved = __ballot(is_near || is_slow);
                const unsigned long long slow_mask = __ballot(is_slow);
                // Rounds in stream order.  H = start of the first unresolved match: every output byte below H is
                // final, so each round moves, all lanes at once, every short non-overlapping near match whose
                // source ends at or below H (on typical data most matches go in the first round; ~6 rounds per
                // batch on the Silesia stand-in).  When the first unresolved match is not of that kind (long,
                // overlapping, wrapping, prefix / straddling source) the wave moves that one cooperatively.
                // LDS runs one wave's accesses in order, so no wait separates dependent rounds.
                {
                    const uint32_t si = RIDX(s0);
                    const bool solo_ok = is_near && M <= off && M <= kShort && !mwrap && !(si + M > rg.kRing);
                    const unsigned long long solo_mask = __ballot(solo_ok);
                    uint32_t src_end = solo_ok ? s0 + span : 0xFFFFFFFFu;     // ~0 once the lane's match has been moved
                    if (LZF_DBG_SKIP & 2) unresolved = 0;
                    while (unresolved) {
#if defined(LZF_DBG_ROUNDS) && defined(LZF_DBG_ROUNDS_HERE)   // analysis: iterations of this loop (match rounds + cooperative matches) and batches, per job
                        ++dbg_rounds;
#endif
#if defined(LZF_FED_DECODE) && defined(LZF_DBG_FED_COUNT)
                        ++dbg_fed[3];
#endif
                        const uint32_t f = (uint32_t)__builtin_ctzll(unresolved);
                        const unsigned long long bit = 1ull << f;
                        if (solo_mask & bit) {
                            const uint32_t H = __builtin_amdgcn_readlane(mo, f);
                            const bool mine = src_end <= H;                    // includes lane f
                            if (mine) { put_match_lds(rg.lds + mi, rg.lds + si, M); src_end = 0xFFFFFFFFu; }
#if defined(LZF_DBG_ROUNDS) && defined(LZF_DBG_ROUNDS_HERE) && LZF_DBG_ROUNDS >= 3      // analysis: active lanes of the rounds (s_bcnt1 of the lanes that move)
                            { const uint32_t nl = (uint32_t)__builtin_popcountll(__ballot(mine));
                              dbg_lane_stat += LZF_DBG_ROUNDS == 3 ? nl : LZF_DBG_ROUNDS == 4 ? 1u : LZF_DBG_ROUNDS == 5 ? (nl == 1u) : LZF_DBG_ROUNDS == 6 ? (nl >= 2u && nl <= 4u)
                                             : LZF_DBG_ROUNDS == 7 ? (nl >= 5u && nl <= 16u) : (nl >= 17u); }
#endif
                            unresolved &= ~__ballot(mine);
                            continue;
                        }
                        unresolved &= ~bit;
                        if (slow_mask & bit) {
                            // prefix / straddling source: one lane, byte-serial, three sources
                            if (lane == f) {
                                for (uint32_t t = 0; t < M; ++t) {
                                    uint8_t v;
                                    if (off > mo + t) v = jv.prefix[jv.plen - (off - mo) + t];                // :91-93
                                    else {
                                        const uint32_t s = mo + t - off;
                                        v = s < near_lo ? jv.out[s] : rg.ring[RIDX(s)];
                                    }
                                    rg.ring[RIDX(mo + t)] = v;
                                }
                            }
                            continue;
                        }
                        const uint32_t jm = __builtin_amdgcn_readlane(M, f);
                        const uint32_t js = __builtin_amdgcn_readlane(s0, f);
                        const uint32_t jo = __builtin_amdgcn_readlane(mo, f);
                        const uint32_t joff = __builtin_amdgcn_readlane(off, f);
                        if (jm <= joff) {                                   // non-overlapping: 4 bytes in flight per lane
                            for (uint32_t i = lane; i < jm; i += 4u * kWave) {
                                const uint32_t i1 = i + kWave, i2 = i + 2u * kWave, i3 = i + 3u * kWave;
                                const uint8_t b0 = rg.ring[RIDX(js + i)];
                                const uint8_t b1 = i1 < jm ? rg.ring[RIDX(js + i1)] : (uint8_t)0;
                                const uint8_t b2 = i2 < jm ? rg.ring[RIDX(js + i2)] : (uint8_t)0;
                                const uint8_t b3 = i3 < jm ? rg.ring[RIDX(js + i3)] : (uint8_t)0;
                                rg.ring[RIDX(jo + i)] = b0;
                                if (i1 < jm) rg.ring[RIDX(jo + i1)] = b1;
                                if (i2 < jm) rg.ring[RIDX(jo + i2)] = b2;
                                if (i3 < jm) rg.ring[RIDX(jo + i3)] = b3;
                            }
#if defined(LZF_FED_DECODE)
                        } else if ((LZF_DBG_SKIP & 64) && joff <= 8u && ((0x116u >> joff) & 1u)) {      // (analysis: what the moves of these matches cost; wrong output)
#endif
                        } else {                                            // overlapping: period-`offset` addressing
#if defined(LZF_FED_DECODE) && !defined(LZF_FED_NO_PERIODIC)
                            // (an offset that is a power of two — 1, 2, 4 and 8 are 95 % of these matches on the Silesia stand-in — needs neither
                            //  of the two divisions: lane % joff is a mask, and kWave % joff is 0 up to 64 and kWave beyond, the same mask of kWave)
                            uint32_t rr = lane & (joff - 1u), adv = kWave & (joff - 1u);
                            if ((joff & (joff - 1u)) != 0u) {
                                asm volatile("");      // (both divisions stay in here: hipcc otherwise starts them in front of the test)
                                rr = lane % joff; adv = kWave % joff;
                            }
#if defined(LZF_DBG_FED_COUNT)
                            dbg_fed[4] += (joff & (joff - 1u)) == 0u ? 1u : 0u;
#endif
#else
                            uint32_t rr = lane % joff;
                            const uint32_t adv = kWave % joff;
#endif
                            for (uint32_t i = lane; i < jm; i += kWave) {
                                rg.ring[RIDX(jo + i)] = rg.ring[RIDX(js + rr)];
                                rr += adv; if (rr >= joff) rr -= joff;
                            }
                        }
                    }
                }
                PHASE(4);
                o = ob0 + __builtin_amdgcn_readlane(incl, (nb - 1u) & 63u);
#if defined(LZF_FED_DECODE)
                // (out[ob0, o) stays in the ring behind what is pending already: the next batch flushes it, or the kernel when its loop ends)
#else
                // ---- flush the batch ring -> HBM
                if (!(LZF_DBG_SKIP & 16)) rg.flush(ob0, o);
#endif
                tidx += nb;
                PHASE(5);
            }
