// lz4_decompress_feed_phase.inc — the FEED stage of the bitmap-fed decompress kernels (lz4_decompress_fed.hip): what the PARSE
// stage of lz4_decompress_parse_phase.inc produces for a chunk — the token list of the chunk — taken from the token bit map the
// hop parse of the segmented pipeline wrote for the whole batch (lzf_seg_parse_kernel, lz4_seg_front.hip) instead of being
// worked out in the kernel.  Textual include inside the kernel's window loop.
//
// A WINDOW is kRound = 32 * W bytes of compressed input from cstart, the 32-aligned position at or below `expect`, the chain's next
// token (lzf_fed_window.h; -DLZF_FED_FIXED_ROUNDS: from the kRound-aligned position instead) — W bit-map words, one per lane, each
// taken from the row of the chunk that owns it.
//
// Nothing of the bit map is trusted: the listed tokens are accepted only as a VERIFIED CHAIN.  The first token of the job
// must sit at position 0, and every listed token must sit where its predecessor ends — worked out from the predecessor's own
// bytes (decompress.rs:61-71 without the copies); the carry between batches and windows is `expect`.  By induction the accepted
// tokens are exactly the tokens decompress_raw visits.  The copy stage checks the links of a batch as it decodes the batch's
// tokens (lz4_decompress_batch_phase.inc, LZF_FED_DECODE), before it writes anything of the batch; here only the list is made.
// `expect` also says from where a chunk's marks are the true tokens (what the seam stage works out for the segmented pipeline): a
// chunk's parse starts at an arbitrary byte, its marks below the position where the true chain enters its share are not the
// chain's — and they lie below `expect`, so clearing the window's bits below `expect` removes them.
// When the map is wrong about a window all the same — the chunk's chain has not fallen in step with the true one yet (0.4 % of
// the chunk boundaries of the Silesia stand-in), or the map is damaged: no mark at `expect`, a link that does not verify, more
// marks than TOKCAP — the copy stage leaves with `bail` before it has written anything of the failing batch, and the kernel does
// the window again from the last verified `expect` in WALK MODE (fed_walk): lane 0 steps through the window's tokens with the
// general routine and lists them, the batches run over that list through the same set-up and the same checks.  A failure in walk
// mode (a token whose body leaves the input: UnexpectedEnd) is a real one: the job is left to the pair kernel, which decodes it
// from its first byte and reports the reference's status.  The next window tries the map again.
//
// The stage's interface (checked below): lane, jv (DecodeJob); cstart (window start) and expect (uniform, cstart <= expect < cstart + 32 —
// kRound with fixed rounds) of the kernel's loop; fed_walk (uniform); cbuf / cbuf_a (kCB staged bytes), toks (uint16_t[TOKCAP]), fed_bits (the
// job's rows of seg_ctx::bits), the constants W, TOKCAP, kRound, kCB.  Leaves: sb (StagedBytes over the window), Tc (tokens listed for this
// window), bail (uniform).  Token-list entry = the token's offset in the window (< kRound), two aligned bytes.
// (Three-byte entries of offset and pre-decoded lengths were measured: 97.5 -> 110 ms per call, misaligned DS accesses.)
            LZF_STAGE_NEEDS(jv, DecodeJob); LZF_STAGE_NEEDS(lane, uint32_t); LZF_STAGE_NEEDS(cstart, uint32_t); LZF_STAGE_NEEDS(expect, uint32_t);
            LZF_STAGE_NEEDS(fed_walk, bool); LZF_STAGE_NEEDS(cbuf[0], uint8_t); LZF_STAGE_NEEDS(toks[0], uint16_t); LZF_STAGE_NEEDS(fed_bits[0] + 0u, uint32_t);
            static_assert(kRound == 32u * (uint32_t)W && kCB >= kRound && TOKCAP > 0, "the window's geometry");
            uint32_t Tc = 0;
            bool bail = false;
            const StagedBytes<true, kCB> sb{cbuf_a, cstart, jv.len, jv.in};      // the staged window, for walk mode and for the copy stage
            {
                // ---- F0. stage in[cstart, cstart + kCB) (zeros beyond the input) and fetch the window's words of the bit map
                // (Asking for the next round one round ahead — held in registers, or one load per 64 bytes to bring its lines into
                // L2 — changed nothing at five or at six waves per SIMD: the other wavefronts already cover this round trip,
                // profiles/fed_residency_prefetch.txt section 3.)
                {
                    const uint32_t avail = jv.len - cstart < kCB ? jv.len - cstart : kCB;
                    cgu8* g = jv.in + cstart;
                    constexpr uint32_t kPieces = (kCB + 1023u) / 1024u;
                    u32x4 v[kPieces];
#pragma unroll
                    for (uint32_t k = 0; k < kPieces; ++k) {
                        const uint32_t i = k * 1024u + lane * 16u;
                        v[k] = u32x4{0, 0, 0, 0};
                        if (i + 16u <= avail) v[k] = ld16(g + i);
                        else if (i < avail) { for (uint32_t t = 0; i + t < avail; ++t) v[k][(t >> 2) & 3u] |= (uint32_t)g[i + t] << ((t & 3u) * 8u); }
                    }
                    // every lane's word from the row of the chunk of the segmented parse that owns it (lzf_fed_window.h: chunk 0 owns the
                    // first kSegChunk bytes, chunk h >= 1 the kSegStride bytes from h * kSegStride + kSegOverlap on)
                    uint32_t w = 0;
                    const uint32_t wpos = cstart + lane * 32u;                 // position of bit 0
                    if (!fed_walk && lane < (uint32_t)W && wpos < jv.len) {
                        const uint32_t h = lzf_fedw_chunk(wpos);
                        w = fed_bits[(size_t)h * kSegChunkWords + lzf_fedw_word(wpos, h)];
                        if (expect >= wpos + 32u) w = 0u;                      // marks below the chain's position are not the chain's
                        else if (expect > wpos) w &= ~((1u << (expect - wpos)) - 1u);
                        if (jv.len - wpos < 32u) w &= (1u << (jv.len - wpos)) - 1u;
                    }
#pragma unroll
                    for (uint32_t k = 0; k < kPieces; ++k) {
                        const uint32_t i = k * 1024u + lane * 16u;
                        if (i < kCB) *reinterpret_cast<u32x4*>(&cbuf[i]) = v[k];
                    }
                    PHASE(6);
                    if (!fed_walk) {
                        // ---- F1. bit map -> token positions in stream order
                        const uint32_t cnt = (uint32_t)__popc(w);
                        const uint32_t incl = wave_scan_add(cnt);
                        uint32_t k = incl - cnt;
                        Tc = __builtin_amdgcn_readlane(incl, 63);              // <= kRound / 3 + 1 would hold for a true chain; TOKCAP >= kRound is not needed:
                        if (Tc > (uint32_t)TOKCAP) { bail = true; Tc = 0; }    // more marks than any chain has (tokens are >= 1 byte apart only in a damaged map)
                        else while (w) { const uint32_t b = (uint32_t)__builtin_ctz(w); toks[k++] = lane * 32u + b; w &= w - 1u; }
                        if (Tc == 0u) bail = true;                             // the chain has a token in this window (at `expect`) and none is marked
                    } else {
                        // ---- F1'. walk mode: lane 0 lists the tokens of the true chain that start in the window, from `expect` on
                        // (decompress.rs:61-71 without the copies; at most kRound / 3 + 1 <= TOKCAP of them, and the loop is held to that)
                        uint32_t np = 0, werr = 0;
                        if (lane == 0u) {
                            uint32_t p = expect;
                            while (p - cstart < kRound && p < jv.len && np < (uint32_t)TOKCAP) {
                                toks[np++] = (uint16_t)(p - cstart);
                                const uint32_t tok = sb.rdb(p);
                                uint32_t q = p + 1u, L = tok >> 4, b = 0;
                                if (L == 15u) { do { if (q >= jv.len) { werr = 1u; break; } b = sb.rdb(q); ++q; L += b; if (L > kMaxPosB) L = kMaxPosB; } while (b == 255u); }
                                if (werr || jv.len - q < L) { werr = 1u; break; }      // :67 read_exact
                                q += L;
                                if (jv.len - q < 2u) { p = jv.len; break; }               // :70 read_u16 fails: last literals
                                q += 2u;
                                if ((tok & 15u) == 15u) { do { if (q >= jv.len) { werr = 1u; break; } b = sb.rdb(q); ++q; } while (b == 255u); }
                                if (werr) break;
                                p = q;
                            }
                        }
                        Tc = __builtin_amdgcn_readfirstlane(np);
                        if (__builtin_amdgcn_readfirstlane(werr) || Tc == 0u) { bail = true; Tc = 0; }
                    }
                }
                PHASE(7);
            }
